"""GPU: the final-exponentiation programs (bls/staged.hpp: four products per
a^|x|, the verdict-only hard part through 3 h) in k_final2 (default, a lane
pair per signature) and k_final (CESS_BLS_FINAL=lane), on the six-kernel
pipeline (CESS_BLS_SMALL_BATCH=0).

Per-signature verify at n = 1, 33, 129, 257 (one lane pair; one wave of 32
signatures plus one; one 128-signature block plus one; two blocks plus one)
with forgeries at 0, 31, 32, 127, 128 and n - 1, one record that stage 1
rejects and one (O, O) record inside a wave of valid ones: codes and verdict
bitmap words exact.  Gt output at n = 33: bytes equal to the fixtures, with a
record that takes the degenerate chain (Miller value in Fp6, m = 1, z2 = z3 =
0; tests/test_gpu_subfield.py) in the same wave as ordinary records.

The kernel choice is read once per process (host.cpp final_pair), so each
mode runs all its batches in one child process."""
import json
import os
import subprocess
import sys

import pytest

import oracle.bls_oracle as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 33, 129, 257)
FORGED_AT = (0, 31, 32, 127, 128)
BAD_AT, OO_AT, DEGEN_AT = 5, 9, 5
N_GT = 33

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from cess_amd import bls
job = json.load(open(sys.argv[2]))
ctx = bls.Context(max_batch=1 << 12)
out = {"verify": [], "gt": []}
for recs in job["verify"]:
    recs = [tuple(bytes.fromhex(x) for x in r) for r in recs]
    offs = [0]
    for r in recs:
        offs.append(offs[-1] + len(r[1]))
    codes, words = ctx.verify_fixed(b"".join(r[0] for r in recs), b"".join(r[2] for r in recs),
                                    b"".join(r[1] for r in recs), offs)
    out["verify"].append([list(codes), [int(w) for w in words]])
for recs in job["gt"]:
    codes, gts = ctx.gt([tuple(bytes.fromhex(x) for x in r) for r in recs])
    out["gt"].append([list(codes), [g.hex() for g in gts]])
ctx.close()
print(json.dumps(out))
"""


def _rec(c):
    return (c["sig"], c["msg"], c["pk"])


def _verify_batch(vectors, n, forge=True):
    """n records (hex triples) and their codes: golden valid records in turn,
    golden forgeries at FORGED_AT and n - 1, a bad signature encoding at
    BAD_AT and an (O, O) record at OO_AT where the batch has those indices."""
    by_name = {c["name"]: c for c in vectors["cases"]}
    valid = [c for c in vectors["cases"] if c["code"] == 0 and not c["name"].startswith("identity")]
    forged = [c for c in vectors["cases"] if c["name"].startswith("forged")]
    assert len(valid) >= 12 and len(forged) >= 6
    cases = [valid[i % len(valid)] for i in range(n)]
    if n > OO_AT:
        cases[BAD_AT] = by_name["sig_offcurve_0"]
        cases[OO_AT] = by_name["identity_pair_2"]
    if forge:
        for j, i in enumerate(sorted({i for i in FORGED_AT + (n - 1,) if i < n})):
            cases[i] = forged[j % len(forged)]
    return [_rec(c) for c in cases], [c["code"] for c in cases]


def _gt_batch(vectors):
    """N_GT records with golden Gt bytes in turn, and at DEGEN_AT the
    signature H(m) under the key G2 (secret key 1): Gt = 1."""
    g = [c for c in vectors["cases"] if "gt" in c]
    assert len(g) >= 8
    cases = [g[i % len(g)] for i in range(N_GT)]
    recs = [_rec(c) for c in cases]
    codes = [c["code"] for c in cases]
    gts = [c["gt"] for c in cases]
    msg = b"subfield miller value"
    recs[DEGEN_AT] = (o.g1_to_compressed(o.hash_to_g1(msg)).hex(), msg.hex(), o.g2_to_compressed(o.G2_GEN).hex())
    codes[DEGEN_AT] = 0
    gts[DEGEN_AT] = o.gt_to_bytes(o.F12_ONE).hex()
    return recs, codes, gts


@pytest.fixture(scope="module")
def job(vectors):
    verify = [_verify_batch(vectors, n) for n in SIZES] + [_verify_batch(vectors, 1, forge=False)]
    gt = _gt_batch(vectors)
    return {"verify": verify, "gt": gt}


@pytest.fixture(scope="module", params=["pair", "lane"])
def outputs(request, job, tmp_path_factory):
    path = tmp_path_factory.mktemp("final_program") / "job.json"
    path.write_text(json.dumps({"verify": [recs for recs, _ in job["verify"]], "gt": [job["gt"][0]]}))
    env = dict(os.environ, CESS_BLS_SMALL_BATCH="0")
    env.pop("CESS_BLS_FINAL", None)
    if request.param == "lane":
        env["CESS_BLS_FINAL"] = "lane"
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=env, capture_output=True, text=True,
                         timeout=180)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _bitmap_words(codes):
    words = [0] * ((len(codes) + 63) // 64)
    for i, c in enumerate(codes):
        if c == 0:
            words[i // 64] |= 1 << (i % 64)
    return words


@pytest.mark.parametrize("k", range(len(SIZES) + 1), ids=[f"n{n}" for n in SIZES] + ["n1_valid"])
def test_verify_codes_and_bitmap(outputs, job, k):
    _, want = job["verify"][k]
    codes, words = outputs["verify"][k]
    n = len(want)
    if k < len(SIZES):
        assert n == SIZES[k]
        assert all(want[i] == 5 for i in FORGED_AT + (n - 1,) if i < n)
        if n > OO_AT:
            assert want[BAD_AT] == 2 and want[OO_AT] == 0 and want.count(0) > n // 2
    assert codes == want
    assert words == _bitmap_words(want)


def test_gt_bytes(outputs, job):
    _, want_codes, want_gts = job["gt"]
    codes, gts = outputs["gt"][0]
    assert len(codes) == N_GT and DEGEN_AT // 32 == (DEGEN_AT + 1) // 32
    assert codes == want_codes
    assert gts == want_gts
