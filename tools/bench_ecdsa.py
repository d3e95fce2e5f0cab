#!/usr/bin/env python3
"""Throughput of the ECDSA P-256 batch verifier (include/cess_ecdsa.h) on one
GPU: 2^log2n records of 32-byte messages (default 2^20) under 16 keys and under
as many distinct keys as records, all valid and with 1 % invalid records placed
at wave and block edges.  Every code is checked exactly against the expected
one and a sample against tests/ecdsa_model.py.  Writes profiles/ecdsa_bench.json
with the rates, the per-kernel times from cess_ecdsa_stage_stats, the counted
multiply-adds per record, the resulting fraction of the multiply-add peak that
DESIGN.md uses, the shader clock sampled while batches run and the library's
SHA-256.  --quick (16 keys, valid records) and CESS_BLS_LIB compare two builds.

TEST DATA ONLY: keys and nonces are incremental (Q_i = Q_0 + i G, k_i = k_0 +
i), so that a record costs one or two point additions in Python.  Nonces that
are related like this give the private key away; nothing here is a signer.
"""
import argparse
import hashlib
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ecdsa_model as m  # noqa: E402

MAD_PEAK = 32.5e12            # v_mad_u64_u32 per second (tools/mad_peak.hip)
MUL_Q, SQR_Q, MUL_N, SQR_N = 170, 125, 200, 155


def counted_mads():
    inv_mul = 7 + bin(0xbce6faada7179e84f3b9cac2fc63254f).count("1")
    inv = 255 * SQR_N + inv_mul * MUL_N
    scal = 3 * MUL_N                                   # to Montgomery, u1, u2
    dbl = 256 * (3 * MUL_Q + 5 * SQR_Q)
    add = 130 * 15 / 16 * (8 * MUL_Q + 3 * SQR_Q)      # 65 digits of each scalar, one in 16 zero
    fin = SQR_Q + 2 * MUL_Q
    return {"inverse": inv, "scalars": scal, "doublings": dbl, "additions": round(add), "final": fin,
            "total": round(inv + scal + dbl + add + fin)}


def make(n, nkeys, alg, rng):
    """n valid records under nkeys keys: (keys, idx, msgs, sigs)"""
    d0, k0 = rng.randrange(1, m.N // 2), rng.randrange(1, m.N // 2)
    keys, q = [], m.mul(d0, m.G)
    for _ in range(nkeys):
        keys.append(m.key_bytes(q))
        q = m.add(q, m.G)
    idx, msgs, sigs = [], [], []
    rp = m.mul(k0, m.G)
    for i in range(n):
        j = i % nkeys
        msg = hashlib.sha256(b"bench %d" % i).digest()
        e = m.digest_scalar(alg, msg)
        k = k0 + i
        r = rp[0] % m.N
        s = pow(k, -1, m.N) * (e + r * (d0 + j)) % m.N
        idx.append(j), msgs.append(msg), sigs.append(m.encode_sig(alg, r, s))
        rp = m.add(rp, m.G)
    return keys, idx, msgs, sigs


def spoil(n, msgs, sigs, idx, nkeys, alg):
    """1 % invalid records at wave and block edges; returns the expected codes"""
    want = [m.OK] * n
    edges = [p for b in range(0, n, 256) for p in (b, b + 63, b + 64, b + 255) if p < n]
    count = min(len(edges), max(1, n // 100))
    for t, p in enumerate(sorted({edges[j * len(edges) // count] for j in range(count)})):
        kind = t % 4
        if kind == 0:
            msgs[p] = msgs[p][:-1] + bytes([msgs[p][-1] ^ 1]); want[p] = m.MISMATCH
        elif kind == 1:
            sigs[p] = sigs[p][:-1]; want[p] = m.SIG_FORMAT
        elif kind == 2:
            sigs[p] = m.encode_sig(alg, m.N, 1); want[p] = m.SIG_RANGE
        else:
            idx[p] = nkeys + 5; want[p] = m.KEY
    return want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alg", type=int, default=m.ALG_P256_SHA256_FIXED)
    ap.add_argument("--quick", action="store_true", help="16 keys, valid records only (A/B of two builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecdsa_bench.json"))
    a = ap.parse_args()
    from cess_amd import bls
    n, rng = 1 << a.log2n, random.Random(256)
    lib_path = bls.LIB_PATH
    res = {"records": n, "message_bytes": 32, "alg": a.alg, "reps": a.reps, "mads_per_record": counted_mads(),
           "mad_peak_per_s": MAD_PEAK, "library": os.path.relpath(lib_path, ROOT), "library_sha256": hashlib.sha256(open(lib_path, "rb").read()).hexdigest(),
           "test_data": "incremental keys and nonces: test data only", "runs": []}
    ctx = bls.Context(max_batch=n, profile=True)
    for nkeys in ((16,) if a.quick else (16, n)):
        t0 = time.time()
        keys, idx, msgs, sigs = make(n, nkeys, a.alg, rng)
        print("made %d records under %d keys in %.0f s" % (n, nkeys, time.time() - t0), flush=True)
        for invalid in ((False,) if a.quick else (False, True)):
            ii, mm, ss = list(idx), list(msgs), list(sigs)
            want = spoil(n, mm, ss, ii, nkeys, a.alg) if invalid else [m.OK] * n
            t0 = time.time()
            assert ctx.ecdsa_keys_load(keys) == [0] * nkeys
            t_keys = time.time() - t0
            ctx.ecdsa_verify_batch(ii, mm, ss, alg=a.alg)              # warm-up
            ctx.ecdsa_stage_stats(reset=True)
            ctx.stage_stats(reset=True) if hasattr(ctx, "stage_stats") else None
            times = []
            for _ in range(a.reps):
                t0 = time.time()
                codes = ctx.ecdsa_verify_batch(ii, mm, ss, alg=a.alg)
                times.append(time.time() - t0)
                assert list(codes) == want, "codes differ"
            for p in random.Random(1).sample(range(n), 64) + [i for i, c in enumerate(want) if c][:64]:
                key = keys[ii[p]] if ii[p] < nkeys else None
                assert m.verify_code(a.alg, key, mm[p], ss[p]) == want[p] == codes[p]
            st = ctx.ecdsa_stage_stats(reset=True)
            kern = {k: v[0] / max(v[1], 1) for k, v in st.items()}
            run = {"keys": nkeys, "invalid_percent": 100.0 * sum(1 for c in want if c) / n,
                   "host_call_s": sorted(times), "records_per_s_host_call": n / sorted(times)[len(times) // 2],
                   "keys_load_s": t_keys, "kernel_ms_per_launch": kern}
            if kern.get("k_ecdsa_verify"):
                rate = n / (kern["k_ecdsa_verify"] / 1e3)
                run["records_per_s_verify_kernel"] = rate
                run["fraction_of_mad_peak"] = rate * res["mads_per_record"]["total"] / MAD_PEAK
            print(json.dumps(run), flush=True)
            res["runs"].append(run)
            if "clock_under_load" not in res:
                # the shader clock while batches run: the query (read-only) is started, and batches are
                # verified until it has answered
                try:
                    q = subprocess.Popen(["rocm-smi", "--showclocks"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                         text=True)
                    busy = 0
                    while q.poll() is None and busy < 200:
                        ctx.ecdsa_verify_batch(ii, mm, ss, alg=a.alg)
                        busy += 1
                    out = q.communicate(timeout=30)[0]
                    res["clock_under_load"] = {"sclk": [ln.strip() for ln in out.splitlines() if "sclk" in ln][:1],
                                               "batches_verified_meanwhile": busy}
                except Exception as e:  # noqa: BLE001
                    res["clock_under_load"] = "unavailable: %s" % e
                ctx.ecdsa_stage_stats(reset=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"ecdsa_bench": a.out, "records": n}))


if __name__ == "__main__":
    main()
