"""Throughput of the Ed25519 batch signer (include/cess_ed25519_sign.h) on one MI355X.

Workload: 1,048,576 device-resident records with 32-byte messages, under 16
signers and under 1,048,576 signers (seeds drawn from a fixed generator), signed
through the device-resident entry.

Legs (16 / 1M signers), each a fresh child process under its own time limit,
stopped at the first failure.  Correctness inside every leg: the signatures of
the last step go through the GPU verifier (the signers' public keys loaded as
its key table) and the popcount of the verdict bitmap must equal n; a sample of
1,024 records must equal tests/ed25519_model.py's sign().  Rates are host-clock
signatures/s around steps that end in a device synchronise (signer loading is
outside the steps and timed on its own); stage times are HIP events around the
launches (CESS_BLS_F_PROFILE), averaged per step.

The bound: by the operation counts k_ed25519_sign_r does about a
quarter of k_ed25519_verify's field work; with a factor of two allowed for its
colder 61 KB table, its stage time must be at most half of k_ed25519_verify's
for the same n, both measured in the same process.  Both values and the verdict
are in the record; a leg that misses the bound fails.

Usage:  python tools/bench_ed25519_sign.py [--n N] [--steps K] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MSG_BYTES = 32
SAMPLE = 1024
MAD_PEAK_PER_S = 32.5e12          # v_mad_u64_u32, measured (bls/field.hpp, tools/mad_peak)
# counted multiply-adds of k_ed25519_sign_r: 64 additions of 7 multiplies, the inversion
# (254 squares, 11 multiplies) and 2 multiplies of the encoding: squares x 55 + multiplies x 100
MADS_SIGN_R = 254 * 55 + (448 + 11 + 2) * 100
LEGS = ("16", "1M")


def leg(args):
    """One leg in this process: prints one JSON line."""
    import ed25519_model as model
    from bench_ed25519 import ClockSampler
    from cess_amd import bls
    n = args.n
    nsigners = 16 if args.signers == "16" else n
    rng = np.random.default_rng(0x5EED25519)
    seeds = np.frombuffer(rng.bytes(32 * nsigners), dtype=np.uint8).reshape(nsigners, 32)
    msgs = np.frombuffer(rng.bytes(n * MSG_BYTES), dtype=np.uint8).reshape(n, MSG_BYTES)
    idx = (np.arange(n) % nsigners).astype(np.uint32)
    ctx = bls.Context(max_batch=4096, profile=True)
    seed_list = [s.tobytes() for s in seeds]
    t0 = time.perf_counter()
    pubs, status = ctx.ed25519_signers_load(seed_list)
    load_s = time.perf_counter() - t0
    assert not any(status)
    st = ctx.ed25519_sign_stage_stats(reset=True)
    comb_ms, signers_ms = st["k_ed25519_comb"][0], st["k_ed25519_signers"][0]
    d = [ctx.to_device(idx), ctx.to_device(msgs), ctx.to_device(np.arange(n + 1, dtype=np.uint64) * MSG_BYTES)]
    ds, dc = ctx.device_alloc(64 * n), ctx.device_alloc(n)
    for _ in range(args.warmup):
        ctx.ed25519_sign_batch_device(n, *d, ds, dc)
    ctx.synchronize()
    ctx.stage_stats(reset=True)
    ctx.ed25519_sign_stage_stats(reset=True)
    clock = ClockSampler()
    clock.start()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctx.ed25519_sign_batch_device(n, *d, ds, dc)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    clock.stop.set()
    stages = {k: v[0] / args.steps for k, v in ctx.ed25519_sign_stage_stats(reset=True).items() if v[1] > 0}
    stages["k_rsa_digest"] = ctx.stage_stats(reset=True)["k_rsa_digest"][0] / args.steps
    codes = np.frombuffer(ctx.from_device(dc, n), dtype=np.uint8)
    # the last step's signatures through the GPU verifier, where they lie
    assert ctx.ed25519_keys_load(pubs) == [0] * nsigners
    dso, dv = ctx.to_device(np.arange(n + 1, dtype=np.uint64) * 64), ctx.device_alloc(n)
    ctx.ed25519_stage_stats(reset=True)
    ctx.ed25519_verify_batch_device(n, d[0], ds, dso, d[1], d[2], dv)
    ctx.synchronize()
    verify_ms = ctx.ed25519_stage_stats(reset=True)["k_ed25519_verify"][0]
    verdict = np.frombuffer(ctx.from_device(dv, n), dtype=np.uint8)
    popcount = int(np.unpackbits(np.packbits(verdict == 0)).sum())
    sigs = np.frombuffer(ctx.from_device(ds, 64 * n), dtype=np.uint8).reshape(n, 64)
    pick = np.linspace(0, n - 1, SAMPLE).astype(np.int64)
    sample_ok = all(model.sign(seed_list[int(idx[i])], msgs[i].tobytes()) == sigs[i].tobytes() for i in pick)
    for p in d + [ds, dc, dso, dv]:
        ctx.device_free(p)
    ctx.close()
    clock.join(timeout=15)
    sign_r_ms = stages.get("k_ed25519_sign_r", 0.0)
    bound_met = bool(sign_r_ms and verify_ms and sign_r_ms <= 0.5 * verify_ms)
    ok = bool(popcount == n and sample_ok and not codes.any())
    print(json.dumps({"signers": nsigners, "records": n, "steps": args.steps,
                      "signatures_per_s": n * args.steps / dt, "ms_per_step": dt / args.steps * 1e3,
                      "stage_ms_per_step": stages, "signers_load_s": load_s, "k_ed25519_signers_ms": signers_ms,
                      "k_ed25519_comb_ms": comb_ms, "verify_popcount": popcount, "sample_records": SAMPLE,
                      "sample_equals_model": bool(sample_ok), "k_ed25519_sign_r_ms": sign_r_ms,
                      "k_ed25519_verify_ms_same_n": verify_ms, "sign_r_over_verify": sign_r_ms / verify_ms if verify_ms else None,
                      "bound": "k_ed25519_sign_r <= 0.5 * k_ed25519_verify", "bound_met": bound_met,
                      "mads_sign_r": MADS_SIGN_R,
                      "sign_r_fraction_of_mad_peak":
                          n * MADS_SIGN_R / (sign_r_ms / 1e3) / MAD_PEAK_PER_S if sign_r_ms else None,
                      "sclk_mhz_max_seen": clock.mhz,
                      "lib_sha256": hashlib.sha256(open(bls.LIB_PATH, "rb").read()).hexdigest()}))
    return 0 if ok and bound_met else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ed25519_sign_bench.json"),
                    help="write the whole record (JSON) here")
    ap.add_argument("--leg-timeout", type=int, default=200)
    ap.add_argument("--signers", choices=LEGS)
    args = ap.parse_args()
    if args.signers:
        return leg(args)
    runs = []
    for signers in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--signers", signers, "--n", str(args.n), "--steps",
               str(args.steps), "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"leg {signers} timed out after {args.leg_timeout}s: stopping")
        lines = p.stdout.strip().splitlines()
        if lines and lines[-1].startswith("{"):
            runs.append(json.loads(lines[-1]))
            print(lines[-1], flush=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"workload": f"{args.n} device-resident records, {MSG_BYTES}-byte messages", "runs": runs}, f, indent=1)
        f.write("\n")
    return 0 if len(runs) == len(LEGS) and all(r["bound_met"] and r["verify_popcount"] == r["records"] and
                                               r["sample_equals_model"] for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main() or 0)
