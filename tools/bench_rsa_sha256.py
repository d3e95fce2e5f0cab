"""Throughput of the hashed RSA mode (RSASSA-PKCS1-v1_5 / SHA-256, hashing on
the GPU) on one MI355X, against the raw path over T precomputed on the host.

Workload: 1,048,576 device-resident records, 16 keys of 2048 bits (e = 65537),
1,024 distinct signed records tiled to fill the batch (signing in Python is
slow), 1 % of the records tampered (first message byte flipped: MISMATCH),
message lengths 64 B and 1,024 B.

Legs, each a fresh child process under its own time limit, stopped at the
first failure:
  hashed L   cess_rsa_verify_sha256_batch_device on the messages (length L)
  raw L      cess_rsa_verify_batch_device on the same records with T_i =
             DigestInfo || SHA-256(msg_i) computed by hashlib (the baseline)
Every leg is repeated --reps times, hashed and raw alternating, so the
run-to-run spread is in the record.  `--lib PATH` runs the raw legs on another
build of the library as well (the parent commit's, for the A/B of the
unchanged raw path).  Rates are host-clock records/s around steps that end in
a device synchronise; stage times are HIP events around the launches
(CESS_BLS_F_PROFILE), averaged per step.

The signed pool is made once without a GPU (`--make-pool`, about a minute of
CPython pow) and cached (--pool, default bench_out/rsa_sha256_pool.npz).

`--digest sha384|sha512` runs the same protocol with that digest (hashed legs:
cess_rsa_verify_digest_batch_device; T of 67 / 83 bytes in the raw legs) on a
pool of its own (the same keys and messages, signed for that digest; default
bench_out/rsa_<digest>_pool.npz).  The default, sha256, is the tool as it was.

Usage:  python tools/bench_rsa_sha256.py --make-pool
        python tools/bench_rsa_sha256.py [--digest D] [--n N] [--steps K] [--reps R] [--lib PARENT.so] [--out FILE]
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
PREFIX = bytes.fromhex("3031300d060960864801650304020105000420")
# --digest: (CESS_RSA_DIGEST_*, DigestInfo prefix, hashlib constructor, block bytes, length-field bytes)
DIGESTS = {"sha256": (0, PREFIX, hashlib.sha256, 64, 8),
           "sha384": (1, bytes.fromhex("3041300d060960864801650304020205000430"), hashlib.sha384, 128, 16),
           "sha512": (2, bytes.fromhex("3051300d060960864801650304020305000440"), hashlib.sha512, 128, 16)}
LENGTHS = (64, 1024)
POOL, KEYS = 1024, 16
# floors of the digest stage (MI355X_MICROARCH.md): achievable HBM bandwidth, and
# one VALU wave-instruction per SIMD every 4 cycles on 256 CUs x 4 SIMDs
HBM_BYTES_PER_S = 6.3e12
CUS, SIMDS, CYCLES_PER_VALU = 256, 4, 4


def make_pool(path, digest="sha256"):
    _, prefix, h, _, _ = DIGESTS[digest]
    from oracle import rsa_oracle as o
    rng = random.Random(0x53484132)
    keys = [o.gen_key(2048, 65537, rng) for _ in range(KEYS)]
    out = {"spki": np.array([o.encode_spki(n, e).hex() for n, e, _ in keys])}
    for ln in LENGTHS:
        msgs = np.frombuffer(bytes(rng.randrange(256) for _ in range(POOL * ln)), dtype=np.uint8).reshape(POOL, ln)
        sigs = np.zeros((POOL, 256), dtype=np.uint8)
        for i in range(POOL):
            n, _, d = keys[i % KEYS]
            t = prefix + h(msgs[i].tobytes()).digest()
            sigs[i] = np.frombuffer(o.sign_raw(n, d, t), dtype=np.uint8)
        out[f"msgs{ln}"], out[f"sigs{ln}"] = msgs, sigs
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **out)
    print("pool written:", path)


def leg(args):
    """One leg in this process: prints one JSON line."""
    from cess_amd import bls
    pool = np.load(args.pool)
    ln, n = args.length, args.n
    dg, prefix, h, _, _ = DIGESTS[args.digest]
    ctx = bls.Context(max_batch=4096, profile=True)
    assert ctx.rsa_keys_load([bytes.fromhex(str(h)) for h in pool["spki"]]) == [0] * KEYS
    rng = np.random.default_rng(0x5253)
    pick = np.arange(n) % POOL
    idx = (pick % KEYS).astype(np.uint32)
    msgs = pool[f"msgs{ln}"][pick].copy()
    bad = rng.choice(n, size=max(1, n // 100), replace=False)
    msgs[bad, 0] ^= 0xFF
    expect = np.zeros(n, dtype=np.uint8)
    expect[bad] = 4
    if args.leg == "raw":      # T on the host: 1,024 pool digests and as many tampered ones
        t_pool = np.array([list(prefix + h(m.tobytes()).digest()) for m in pool[f"msgs{ln}"]], dtype=np.uint8)
        payload = t_pool[pick].copy()
        for i in bad:
            payload[i] = np.frombuffer(prefix + h(msgs[i].tobytes()).digest(), dtype=np.uint8)
        call = ctx.rsa_verify_batch_device
    else:
        payload = msgs
        call = ctx.rsa_verify_sha256_batch_device
        if args.digest != "sha256":
            def call(*a):
                return ctx.rsa_verify_digest_batch_device(dg, *a)
    width = payload.shape[1]
    d = [ctx.to_device(idx), ctx.to_device(pool[f"sigs{ln}"][pick].copy()),
         ctx.to_device(np.arange(n + 1, dtype=np.uint64) * 256), ctx.to_device(payload),
         ctx.to_device(np.arange(n + 1, dtype=np.uint64) * width)]
    dc = ctx.device_alloc(n)
    for _ in range(args.warmup):
        call(n, *d, dc)
    ctx.synchronize()
    ctx.stage_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        call(n, *d, dc)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    st = {k: v[0] / args.steps for k, v in ctx.stage_stats(reset=True).items() if v[1] > 0}
    ok = bool((np.frombuffer(ctx.from_device(dc, n), dtype=np.uint8) == expect).all())
    for p in d + [dc]:
        ctx.device_free(p)
    ctx.close()
    extra = {} if args.digest == "sha256" else {"digest": args.digest}
    print(json.dumps({**extra, "leg": args.leg, "msg_bytes": ln, "records": n, "steps": args.steps, "records_per_s": n * args.steps / dt,
                      "ms_per_step": dt / args.steps * 1e3, "stage_ms_per_step": st, "codes_ok": ok,
                      "lib": os.environ.get("CESS_BLS_LIB", "this build"),
                      "lib_sha256": hashlib.sha256(open(bls.LIB_PATH, "rb").read()).hexdigest()}))
    return 0 if ok else 1


def floors(n, ln, valu_per_compression, clock_ghz, digest="sha256"):
    _, _, _, block, length_field = DIGESTS[digest]
    blocks = (ln + 1 + length_field + block - 1) // block
    hbm_ms = n * ln / HBM_BYTES_PER_S * 1e3
    # a wave compresses 64 messages' blocks in lock step: waves x blocks x instructions, 4 cycles each per SIMD
    valu_ms = None
    if valu_per_compression:
        valu_ms = (n / 64) * blocks * valu_per_compression * CYCLES_PER_VALU / (CUS * SIMDS) / (clock_ghz * 1e9) * 1e3
    return {"compressions_per_msg": blocks, "hbm_floor_ms": hbm_ms, "valu_floor_ms": valu_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-pool", action="store_true")
    ap.add_argument("--digest", choices=tuple(DIGESTS), default="sha256")
    ap.add_argument("--pool", help="default bench_out/rsa_<digest>_pool.npz")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", help="another build of the library: the raw legs run on it too")
    ap.add_argument("--out", help="write the whole record (JSON) here")
    ap.add_argument("--leg-timeout", type=int, default=150)
    ap.add_argument("--valu-per-compression", type=int, default=0,
                    help="VALU instructions of one compression in k_rsa_digest's disassembly (for the VALU floor)")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="shader clock assumed by the VALU floor")
    ap.add_argument("--leg", choices=("hashed", "raw"))
    ap.add_argument("--length", type=int, default=64)
    args = ap.parse_args()
    if not args.pool:
        args.pool = os.path.join(ROOT, "bench_out", f"rsa_{args.digest}_pool.npz")
    if args.make_pool:
        return make_pool(args.pool, args.digest)
    if not os.path.exists(args.pool):
        sys.exit(f"{args.pool} missing: run with --make-pool first (no GPU needed)")
    if args.leg:
        return leg(args)
    runs = []
    plan = []
    for rep in range(args.reps):
        for ln in LENGTHS:
            plan += [("hashed", ln, None), ("raw", ln, None)] + ([("raw", ln, args.lib)] if args.lib else [])
    for name, ln, lib in plan:
        env = dict(os.environ)
        if lib:
            env["CESS_BLS_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--length", str(ln), "--n", str(args.n),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--pool", args.pool, "--digest", args.digest]
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"leg {name} {ln} timed out after {args.leg_timeout}s: stopping")
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            sys.exit(f"leg {name} {ln} failed with {p.returncode}: stopping")
        rec = json.loads(p.stdout.strip().splitlines()[-1])
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    summary = {}
    for ln in LENGTHS:
        for name, lib in (("hashed", "this build"), ("raw", "this build")) + ((("raw", os.path.abspath(args.lib)),) if args.lib else ()):
            sel = [r for r in runs if r["leg"] == name and r["msg_bytes"] == ln and r["lib"] == lib]
            rates = [r["records_per_s"] for r in sel]
            key = f"{name}_{ln}" + ("" if lib == "this build" else "_other_lib")
            summary[key] = {"records_per_s": rates, "median": float(np.median(rates)),
                            "spread_frac": (max(rates) - min(rates)) / float(np.median(rates)),
                            "stage_ms_per_step_median": {k: float(np.median([r["stage_ms_per_step"].get(k, 0) for r in sel]))
                                                         for k in sel[0]["stage_ms_per_step"]}}
        summary[f"digest_floors_{ln}"] = floors(args.n, ln, args.valu_per_compression, args.clock_ghz, args.digest)
    out = {**({} if args.digest == "sha256" else {"digest": args.digest}), "workload": f"{args.n} device-resident records, {KEYS} x 2048-bit keys (e = 65537), {POOL} distinct signed records tiled, "
                       "1% tampered", "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "clock_ghz_assumed": args.clock_ghz, "summary": summary, "runs": runs}
    print(json.dumps(out["summary"], indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
