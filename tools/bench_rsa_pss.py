"""RSASSA-PSS verification (ring's RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512) on one MI355X against
RSASSA-PKCS1-v1_5 over the same keys and messages, in one process.

Workload: --n (default 1,048,576) device-resident records, POOL distinct signed records per configuration
tiled to fill the batch (signing in Python is slow), messages of 32 B and 1 KiB, all valid and 1 % invalid
(first message byte changed: MISMATCH), each of the three digests, over three key tables (--tables):
  16        16 keys of 2048 bits (e = 65537): the key-uniform lists (k_rsa_count / _scan / _scatter,
            k_rsa_verify_2048u[m])
  16+3072   the same 16 keys and records, with one 3072-bit key added to the table that no record uses: a
            table with a loop-form key takes the unsorted lists (k_rsa_classify, k_rsa_verify_2048[m])
  65536     2^16 distinct 2048-bit moduli p_i q_j from 256 + 256 primes (--make-grid), also the unsorted lists
            (more than 4096 keys); the records are signed under the 256 keys p_i q_i and so use 256 rows
            spread evenly over the 2^16-row table, not all of them: signing under every key is out of reach
            of CPython's pow
Per configuration, after --warmup calls of each, cess_rsa_verify_pss_batch_device and
cess_rsa_verify_digest_batch_device (PKCS#1 v1.5 signatures of the same messages under the same keys)
alternate --reps times.  A call's time is the sum of its stages' device-event times (CESS_BLS_F_PROFILE:
k_rsa_digest, k_rsa_classify, k_rsa_verify and, for PSS, k_rsa_pss); the host clock around the call and its
synchronise is recorded beside it.  Codes: popcount of OK over the whole batch against the construction,
and a sample of records exactly against the plain-Python model (tests/rsa_pss_model.py).

`--lib PATH` runs the PKCS#1 calls alone in two child processes, one on this build and one on another build
of the library (the parent commit's), and compares those two: same process layout, same call sequence.  The
PKCS#1 kernels are the same objects in both, so a difference beyond the spread is a finding.  (The PKCS#1
figures of the main process, where PSS calls alternate with them, are not comparable with a PKCS#1-only run.)

The signed pools are made once without a GPU (`--make-pool`, `--make-grid`: a few minutes on several cores)
and cached (--pool, --grid, default bench_out/rsa_pss_pool.npz and rsa_pss_grid.npz).

`--stats-from DB --stats-out FILE` reduces the database that `rocprofv3 --kernel-trace --stats` writes for a
run of this tool to one line per kernel (its top_kernels view: calls, total and average duration, share).

Usage:  python tools/bench_rsa_pss.py --make-pool && python tools/bench_rsa_pss.py --make-grid
        python tools/bench_rsa_pss.py [--n N] [--reps R] [--tables 16,16+3072,65536] [--lib PARENT.so] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DIGESTS = {"SHA256": (0, "3031300d060960864801650304020105000420"),
           "SHA384": (1, "3041300d060960864801650304020205000430"),
           "SHA512": (2, "3051300d060960864801650304020305000440")}
LENGTHS = (32, 1024)
POOL, KEYS, GRID = 256, 16, 256
# SHA compressions of k_rsa_pss per record at 2048 bits: MGF1 blocks + the final hash
PSS_COMPRESSIONS = {"SHA256": 7 + 2, "SHA384": 5 + 1, "SHA512": 3 + 2}


def make_pool(path):
    import rsa_pss_model as model
    from oracle import rsa_oracle as o
    rng = random.Random(0x505353)
    keys = [o.gen_key(2048, 65537, rng) for _ in range(KEYS)]
    out = {"pkcs1": np.array([o.encode_pkcs1(n, e).hex() for n, e, _ in keys])}
    for ln in LENGTHS:
        msgs = np.frombuffer(bytes(rng.randrange(256) for _ in range(POOL * ln)), dtype=np.uint8).reshape(POOL, ln)
        out[f"msgs{ln}"] = msgs
        for name, (_, prefix) in DIGESTS.items():
            H = model.HASH[name]
            pss = np.zeros((POOL, 256), dtype=np.uint8)
            v15 = np.zeros((POOL, 256), dtype=np.uint8)
            for i in range(POOL):
                n, _, d = keys[i % KEYS]
                m = msgs[i].tobytes()
                em = model.encode(name, m, bytes(rng.randrange(256) for _ in range(H().digest_size)), 2048)
                pss[i] = np.frombuffer(pow(int.from_bytes(em, "big"), d, n).to_bytes(256, "big"), dtype=np.uint8)
                v15[i] = np.frombuffer(o.sign_raw(n, d, bytes.fromhex(prefix) + H(m).digest()), dtype=np.uint8)
            out[f"pss_{name}_{ln}"], out[f"v15_{name}_{ln}"] = pss, v15
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **out)
    print("pool written:", path)


def _prime(seed):
    from oracle import rsa_oracle as o
    rng = random.Random(seed)
    while True:                                            # as oracle.rsa_oracle.gen_key draws its primes
        c = rng.getrandbits(1024) | (3 << 1022) | 1
        if o._is_probable_prime(c, rng) and (c - 1) % 65537:
            return c


def make_grid(path):
    """256 + 256 primes -> 2^16 moduli; POOL records per configuration signed under the diagonal keys"""
    import multiprocessing
    import rsa_pss_model as model
    from oracle import rsa_oracle as o
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as mp:
        primes = mp.map(_prime, [0x47524944 + i for i in range(2 * GRID)], chunksize=8)
    assert len(set(primes)) == 2 * GRID
    ps, qs = primes[:GRID], primes[GRID:]
    rng = random.Random(0x475249)
    out = {"p": np.array(["%x" % v for v in ps]), "q": np.array(["%x" % v for v in qs])}
    for ln in LENGTHS:
        msgs = np.frombuffer(bytes(rng.randrange(256) for _ in range(POOL * ln)), dtype=np.uint8).reshape(POOL, ln)
        out[f"msgs{ln}"] = msgs
        for name, (_, prefix) in DIGESTS.items():
            H = model.HASH[name]
            pss = np.zeros((POOL, 256), dtype=np.uint8)
            v15 = np.zeros((POOL, 256), dtype=np.uint8)
            for i in range(POOL):
                p, q = ps[i % GRID], qs[i % GRID]
                n, d = p * q, pow(65537, -1, (p - 1) * (q - 1))
                assert n.bit_length() == 2048
                m = msgs[i].tobytes()
                em = model.encode(name, m, bytes(rng.randrange(256) for _ in range(H().digest_size)), 2048)
                pss[i] = np.frombuffer(pow(int.from_bytes(em, "big"), d, n).to_bytes(256, "big"), dtype=np.uint8)
                v15[i] = np.frombuffer(o.sign_raw(n, d, bytes.fromhex(prefix) + H(m).digest()), dtype=np.uint8)
            out[f"pss_{name}_{ln}"], out[f"v15_{name}_{ln}"] = pss, v15
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **out)
    print("grid written:", path)


def table_of(args, table):
    """(pool, DER keys of the table, table row of the key that signed pool record i)"""
    import rsa_pss_model as model
    from oracle import rsa_oracle as o
    if table == "65536":
        pool = np.load(args.grid)
        ps, qs = [int(str(v), 16) for v in pool["p"]], [int(str(v), 16) for v in pool["q"]]
        ders = [o.encode_pkcs1(p * q, 65537) for p in ps for q in qs]
        return pool, ders, np.array([(i % GRID) * (GRID + 1) for i in range(POOL)], dtype=np.uint32)
    pool = np.load(args.pool)
    ders = [bytes.fromhex(str(h)) for h in pool["pkcs1"]]
    if table == "16+3072":
        fx = model.load_fixture("rsa_pss_edges.json.gz")
        ders.append(bytes.fromhex(fx["table"][[k["name"] for k in fx["keys"]].index("k3072")]["der"]))
    return pool, ders, np.array([i % KEYS for i in range(POOL)], dtype=np.uint32)


def kernel_stats(db, dst):
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, total_calls, total_duration, average, percentage from top_kernels")
    lines = ["# the top_kernels view of the database written by `rocprofv3 --kernel-trace --stats -- python "
             "tools/bench_rsa_pss.py ...`,", "# reduced by `tools/bench_rsa_pss.py --stats-from`: kernel names without "
             "their argument lists, durations in microseconds",
             "%-34s %6s %14s %12s %7s" % ("kernel", "calls", "total_us", "average_us", "pct")]
    lines += ["%-34s %6d %14.1f %12.1f %7.2f" % (n.split("(")[0], c, t, a, p) for n, c, t, a, p in rows]
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")


def stage_sum(ctx, pss):
    st = {k: v[0] for k, v in ctx.stage_stats(reset=True).items() if v[1] > 0}
    if pss:
        st.update({k: v[0] for k, v in ctx.rsa_pss_stage_stats(reset=True).items() if v[1] > 0})
    return st


def run(args, table):
    """Every configuration of one key table in this process: one JSON line each, the records returned."""
    import rsa_pss_model as model
    from cess_amd import bls
    pool, ders, row_of = table_of(args, table)
    n = args.n
    ctx = bls.Context(max_batch=4096, profile=True)
    assert ctx.rsa_keys_load(ders, bls.RSA_KEY_PKCS1, bls.RSA_POLICY_RING_2048_8192) == [0] * len(ders)
    keys = {int(r): model.ring_key(ders[int(r)]) for r in set(row_of)}
    have_pss = not args.child and hasattr(bls.load_library(), "cess_rsa_verify_pss_batch")   # a child: PKCS#1 calls only
    rng = np.random.default_rng(0x5253)
    pick = np.arange(n) % POOL
    idx = row_of[pick]
    d_idx = ctx.to_device(idx)
    d_so = ctx.to_device(np.arange(n + 1, dtype=np.uint64) * 256)
    dc = ctx.device_alloc(n)
    records = []
    for ln in LENGTHS:
        d_mo = ctx.to_device(np.arange(n + 1, dtype=np.uint64) * ln)
        for frac in (0, 100):
            msgs = pool[f"msgs{ln}"][pick].copy()
            bad = rng.choice(n, size=n // frac, replace=False) if frac else np.zeros(0, dtype=np.int64)
            msgs[bad, 0] ^= 0xFF
            d_msgs = ctx.to_device(msgs)
            sample = list(bad[:8]) + list(rng.choice(n, size=24, replace=False))
            for name, (dg, _) in DIGESTS.items():
                sigs = {"pss": pool[f"pss_{name}_{ln}"][pick], "pkcs1": pool[f"v15_{name}_{ln}"][pick]}
                d_sigs = {k: ctx.to_device(np.ascontiguousarray(v)) for k, v in sigs.items() if k != "pss" or have_pss}
                calls = {"pkcs1": lambda: ctx.rsa_verify_digest_batch_device(dg, n, d_idx, d_sigs["pkcs1"], d_so,
                                                                             d_msgs, d_mo, dc)}
                if have_pss:
                    calls["pss"] = lambda: ctx.rsa_verify_pss_batch_device(dg, n, d_idx, d_sigs["pss"], d_so, d_msgs,
                                                                           d_mo, dc)
                res = {k: {"device_ms": [], "host_ms": [], "stages_ms": []} for k in calls}
                for it in range(args.warmup + args.reps):
                    for k, call in calls.items():                      # the two alternate
                        ctx.stage_stats(reset=True)
                        if have_pss:
                            ctx.rsa_pss_stage_stats(reset=True)
                        t0 = time.perf_counter()
                        call()
                        ctx.synchronize()
                        dt = (time.perf_counter() - t0) * 1e3
                        st = stage_sum(ctx, have_pss)
                        if it >= args.warmup:
                            res[k]["device_ms"].append(sum(st.values()))
                            res[k]["host_ms"].append(dt)
                            res[k]["stages_ms"].append(st)
                        if it == args.warmup + args.reps - 1:             # codes of the last call
                            codes = np.frombuffer(ctx.from_device(dc, n), dtype=np.uint8)
                            res[k]["ok_count"] = int((codes == 0).sum())
                            res[k]["popcount_ok"] = res[k]["ok_count"] == n - len(bad) and \
                                int((codes == 4).sum()) == len(bad)
                            if k == "pss":
                                want = [model.verify_code(name, *keys[int(idx[i])], msgs[i].tobytes(), sigs["pss"][i].tobytes())
                                        for i in sample]
                                res[k]["sample_ok"] = [int(codes[i]) for i in sample] == want
                for p in d_sigs.values():
                    ctx.device_free(p)
                rec = {"table": table, "digest": name, "msg_bytes": ln, "invalid_frac": 0.01 if frac else 0.0, "records": n,
                       "table_keys": len(ders), "keys_used": len(keys)}
                for k, v in res.items():
                    ms = v["device_ms"]
                    rec[k] = {"device_ms": ms, "median_ms": float(np.median(ms)),
                              "spread_frac": (max(ms) - min(ms)) / float(np.median(ms)),
                              "host_ms_median": float(np.median(v["host_ms"])),
                              "stage_ms_median": {s: float(np.median([x.get(s, 0.0) for x in v["stages_ms"]]))
                                                  for s in v["stages_ms"][0]},
                              "ok_count": v["ok_count"], "popcount_ok": v["popcount_ok"],
                              **({"sample_ok": v["sample_ok"]} if "sample_ok" in v else {})}
                if have_pss:
                    rec["pss_over_pkcs1"] = rec["pss"]["median_ms"] / rec["pkcs1"]["median_ms"]
                    st = rec["pss"]["stage_ms_median"]      # k_rsa_pss: unsorted lists, k_rsa_pss_u: key-uniform ones
                    rec["lists"] = "key-uniform" if "k_rsa_pss_u" in st else "unsorted"
                    pss_ms = st.get("k_rsa_pss", 0.0) + st.get("k_rsa_pss_u", 0.0)
                    rec["k_rsa_pss_ms"] = pss_ms
                    blocks = -(-(ln + 1 + (8 if name == "SHA256" else 16)) // (64 if name == "SHA256" else 128))
                    rec["k_rsa_pss_ns_per_compression"] = pss_ms * 1e6 / (n * PSS_COMPRESSIONS[name])
                    rec["k_rsa_digest_ns_per_compression"] = rec["pss"]["stage_ms_median"]["k_rsa_digest"] * 1e6 / (n * blocks)
                    rec["digest_compressions_per_msg"] = blocks
                print(json.dumps(rec), flush=True)
                records.append(rec)
            ctx.device_free(d_msgs)
        ctx.device_free(d_mo)
    ctx.close()
    ok = all(v.get("popcount_ok") and v.get("sample_ok", True) for r in records for v in r.values() if isinstance(v, dict))
    return records, ok, hashlib.sha256(open(bls.LIB_PATH, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-pool", action="store_true")
    ap.add_argument("--make-grid", action="store_true")
    ap.add_argument("--pool", default=os.path.join(ROOT, "bench_out", "rsa_pss_pool.npz"))
    ap.add_argument("--grid", default=os.path.join(ROOT, "bench_out", "rsa_pss_grid.npz"))
    ap.add_argument("--tables", default="16,16+3072,65536")
    ap.add_argument("--stats-from", help="a rocprofv3 --kernel-trace --stats database of a run of this tool")
    ap.add_argument("--stats-out")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", help="another build of the library: its PKCS#1 calls, in a child process")
    ap.add_argument("--out", help="write the whole record (JSON) here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420)
    args = ap.parse_args()
    if args.make_pool:
        return make_pool(args.pool)
    if args.make_grid:
        return make_grid(args.grid)
    if args.stats_from:
        return kernel_stats(args.stats_from, args.stats_out)
    tables = args.tables.split(",")
    for t in tables:
        need = args.grid if t == "65536" else args.pool
        if t not in ("16", "16+3072", "65536") or not os.path.exists(need):
            sys.exit(f"table {t}: unknown, or {need} missing (run with --make-pool / --make-grid first, no GPU needed)")
    records, ok, sha = [], True, None
    for t in tables:
        r, o_, sha = run(args, t)
        records += r
        ok = ok and o_
    if args.child:
        return 0 if ok else 1
    out = {"workload": f"{args.n} device-resident records, 2048-bit keys (e = 65537), {POOL} distinct signed records per "
                       "configuration tiled; tables: 16 keys (key-uniform lists), 16 keys + one unused 3072-bit key "
                       "(unsorted lists), 65536 keys of which the records use 256 (unsorted lists)",
           "warmup": args.warmup, "reps": args.reps,
           "time": "sum of the stages' device-event times per call (gaps between launches excluded; the k_rsa_pss "
                   "stage includes the launch that marks 1024-bit-class records, about 4 us on these tables)",
           "lib_sha256": sha, "codes_ok": ok, "configurations": records}
    if args.lib and ok:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--warmup", str(args.warmup),
               "--reps", str(args.reps), "--pool", args.pool, "--grid", args.grid, "--tables", args.tables]
        child = {}
        for which, env in (("this", dict(os.environ)), ("other", dict(os.environ, CESS_BLS_LIB=os.path.abspath(args.lib)))):
            try:
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                sys.exit(f"the PKCS#1-only run on {which} library timed out: stopping")
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                sys.exit(f"the PKCS#1-only run on {which} library failed with {p.returncode}: stopping")
            child[which] = [json.loads(line) for line in p.stdout.strip().splitlines() if line.startswith("{")]
        records, other = child["this"], child["other"]
        out["pkcs1_only_this_lib"] = {"lib_sha256": sha, "configurations": records}
        out["other_lib"] = {"lib_sha256": hashlib.sha256(open(args.lib, "rb").read()).hexdigest(), "configurations": other}
        out["pkcs1_this_over_other"] = [
            {"table": a["table"], "digest": a["digest"], "msg_bytes": a["msg_bytes"], "invalid_frac": a["invalid_frac"],
             "ratio": a["pkcs1"]["median_ms"] / b["pkcs1"]["median_ms"],
             "spread_this": a["pkcs1"]["spread_frac"], "spread_other": b["pkcs1"]["spread_frac"]}
            for a, b in zip(records, other)]
        print(json.dumps(out["pkcs1_this_over_other"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main() or 0)
