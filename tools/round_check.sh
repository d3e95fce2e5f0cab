#!/bin/bash
# End-of-session record on one GPU box (repo root): gpu tests, smoke, the
# default bench (with cpu_baseline) and the mode benches.  Usage: TAG=r02u bash tools/round_check.sh
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}   # where this script's records go
mkdir -p $OUT
T=${TAG:-r02u}
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/${T}_pytest.txt 2>&1 || { tail -20 $OUT/${T}_pytest.txt; exit 1; }
tail -1 $OUT/${T}_pytest.txt
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${T}_smoke.txt 2>&1 || exit 3
timeout -k 10 300 python bench.py --full > $OUT/${T}_bench_n1.json 2> $OUT/${T}_bench_n1.err || exit 4
for m in adversarial keyed rsa; do
  timeout -k 10 300 python bench.py --mode $m --steps 3 --cpu-sample 0 > $OUT/${T}_bench_$m.json 2> $OUT/${T}_bench_$m.err || exit 5
done
timeout -k 10 300 python bench.py --mode rlc --steps 3 --cpu-sample 0 > $OUT/${T}_bench_rlc.json 2> $OUT/${T}_bench_rlc.err || exit 6
timeout -k 10 300 python bench.py --mode rlc --forged-count 4 --steps 3 --cpu-sample 0 > $OUT/${T}_bench_rlc_forged4.json 2> $OUT/${T}_bench_rlc_forged4.err || exit 7
for f in $OUT/${T}_bench_*.json; do python3 -c "import json,sys; d=json.load(open('$f')); print('$f', round(d['value']), d.get('verdicts_ok'))"; done
