"""Throughput of the Ed25519 batch verifier (include/cess_ed25519.h) on one MI355X.

Workload: 1,048,576 device-resident records with 32-byte messages, under 16
keys (1,024 distinct signed records tiled) and under 1,048,576 distinct keys,
each all-valid and with 1 % of the records invalid, spread evenly over the
codes SIG_LEN, SIG_RANGE, KEY (index outside the table) and MISMATCH.

Legs (keys x validity), each a fresh child process under its own time limit,
stopped at the first failure.  Every leg compares every code with the
expectation before it reports.  Rates are host-clock records/s around steps
that end in a device synchronise (key loading is outside the steps and timed
on its own); stage times are HIP events around the launches
(CESS_BLS_F_PROFILE), averaged per step.  Next to each rate: the counted
32 x 32 + 64 multiply-adds per record (ed25519.hpp: 55 per square, 100 per
multiply) and the fraction of the measured v_mad_u64_u32 peak
(bls/field.hpp, tools/mad_peak) that the verify kernel's time makes of them.
The shader clock is sampled with `rocm-smi --showclocks` while the steps run
(best effort; the highest sclk seen is reported).

The signed pool is made without a GPU (`--make-pool`): keys a0 + i and nonces
r0 + i, so a record costs two point additions, not two scalar multiplications;
about a minute of CPython for the million-key pool.  Cached under --pool-dir
(default bench_out/).

Usage:  python tools/bench_ed25519.py --make-pool
        python tools/bench_ed25519.py [--n N] [--steps K] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MSG_BYTES = 32
MAD_PEAK_PER_S = 32.5e12          # v_mad_u64_u32, measured (bls/field.hpp, tools/mad_peak)
# counted multiply-adds: squares x 55 + multiplies x 100
MADS_PER_RECORD = 1262 * 55 + 1664 * 100
MADS_PER_KEY = 509 * 55 + 131 * 100
LEGS = (("16", "valid"), ("16", "invalid"), ("1M", "valid"), ("1M", "invalid"))


def make_pool(path, nkeys, n):
    """n signed records under nkeys keys (record i under key i % nkeys): pub (nkeys, 32), msg (n, 32), sig (n, 64)"""
    import ed25519_model as m
    P, L = m.P, m.L
    ext = lambda p: (p[0], p[1], 1, p[0] * p[1] % P)   # noqa: E731
    Bx = ext(m.B)

    def walk(start, count):
        """affine start * B, (start + 1) * B, ...: one addition each and a shared inversion per 1,024"""
        q, out = ext(m.mul(start, m.B)), []
        for base in range(0, count, 1024):
            pts = []
            for _ in range(min(1024, count - base)):
                pts.append(q)
                q = m._ext_add(q, Bx)
            pre, run = [], 1
            for p in pts:
                pre.append(run)
                run = run * p[2] % P
            inv = pow(run, P - 2, P)
            enc = [None] * len(pts)
            for j in range(len(pts) - 1, -1, -1):
                zi = inv * pre[j] % P
                inv = inv * pts[j][2] % P
                x, y = pts[j][0] * zi % P, pts[j][1] * zi % P
                enc[j] = (y | (x & 1) << 255).to_bytes(32, "little")
            out += enc
        return out

    a0 = int.from_bytes(hashlib.sha512(b"bench_ed25519 a0").digest(), "little") % L
    r0 = int.from_bytes(hashlib.sha512(b"bench_ed25519 r0").digest(), "little") % L
    pubs, rs = walk(a0, nkeys), walk(r0, n)
    msgs = np.frombuffer(np.random.default_rng(0xED25519).bytes(n * MSG_BYTES), dtype=np.uint8).reshape(n, MSG_BYTES)
    sigs = bytearray(64 * n)
    for i in range(n):
        k = i % nkeys
        h = int.from_bytes(hashlib.sha512(rs[i] + pubs[k] + msgs[i].tobytes()).digest(), "little")
        sigs[64 * i:64 * i + 32] = rs[i]
        sigs[64 * i + 32:64 * i + 64] = ((r0 + i + h * (a0 + k)) % L).to_bytes(32, "little")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, pub=np.frombuffer(b"".join(pubs), dtype=np.uint8).reshape(nkeys, 32), msg=msgs,
             sig=np.frombuffer(bytes(sigs), dtype=np.uint8).reshape(n, 64))
    print("pool written:", path, nkeys, "keys", n, "records", flush=True)


def pool_path(args, keys):
    return os.path.join(args.pool_dir, "ed25519_pool_16.npz" if keys == "16" else f"ed25519_pool_{args.n}.npz")


class ClockSampler(threading.Thread):
    """highest sclk (MHz) that `rocm-smi --showclocks` shows while running; None where the tool is missing"""

    def __init__(self):
        super().__init__(daemon=True)
        self.stop, self.mhz = threading.Event(), None

    def run(self):
        while not self.stop.is_set():
            try:
                out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
            except (OSError, subprocess.TimeoutExpired):
                return
            for v in re.findall(r"sclk clock level:?\s*\d*:?\s*\((\d+)Mhz\)", out):
                self.mhz = max(self.mhz or 0, int(v))
            self.stop.wait(0.2)   # a few samples per leg, not a process storm on a shared machine


def leg(args):
    """One leg in this process: prints one JSON line."""
    from cess_amd import bls
    pool = np.load(pool_path(args, args.keys))
    n = args.n
    pubs = pool["pub"]
    nkeys = len(pubs)
    pick = np.arange(n) % len(pool["sig"])
    idx = (pick % nkeys).astype(np.uint32)
    msgs, sigs = pool["msg"][pick].copy(), pool["sig"][pick].copy()
    expect = np.zeros(n, dtype=np.uint8)
    lens = np.full(n, 64, dtype=np.uint64)
    if args.validity == "invalid":
        bad = np.random.default_rng(0xBAD).choice(n, size=max(4, n // 100), replace=False)
        for code, sel in zip((1, 2, 3, 4), np.array_split(bad, 4)):
            expect[sel] = code
            if code == 1:
                lens[sel] = 63                       # SIG_LEN: the last byte is dropped below
            elif code == 2:
                sigs[sel, 63] |= 0xF0                # SIG_RANGE: S >= 2^255
            elif code == 3:
                idx[sel] = nkeys                     # KEY: index outside the table
            else:
                msgs[sel, 0] ^= 0xFF                 # MISMATCH
    keep = np.ones((n, 64), dtype=bool)
    keep[lens == 63, 63] = False
    ctx = bls.Context(max_batch=4096, profile=True)
    t0 = time.perf_counter()
    status = ctx.ed25519_keys_load([p.tobytes() for p in pubs])
    load_s = time.perf_counter() - t0
    assert not any(status)
    key_ms = ctx.ed25519_stage_stats(reset=True)["k_ed25519_keys"][0]
    d = [ctx.to_device(idx), ctx.to_device(sigs[keep]),
         ctx.to_device(np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)), ctx.to_device(msgs),
         ctx.to_device(np.arange(n + 1, dtype=np.uint64) * MSG_BYTES)]
    dc = ctx.device_alloc(n)
    for _ in range(args.warmup):
        ctx.ed25519_verify_batch_device(n, *d, dc)
    ctx.synchronize()
    ctx.stage_stats(reset=True)
    ctx.ed25519_stage_stats(reset=True)
    clock = ClockSampler()
    clock.start()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctx.ed25519_verify_batch_device(n, *d, dc)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    clock.stop.set()
    st = {k: v[0] / args.steps for k, v in ctx.ed25519_stage_stats(reset=True).items() if v[1] > 0}
    st["k_rsa_digest"] = ctx.stage_stats(reset=True)["k_rsa_digest"][0] / args.steps
    got = np.frombuffer(ctx.from_device(dc, n), dtype=np.uint8)
    ok = bool((got == expect).all())
    for p in d + [dc]:
        ctx.device_free(p)
    ctx.close()
    clock.join(timeout=15)
    verify_s = st.get("k_ed25519_verify", 0) / 1e3
    print(json.dumps({"keys": nkeys, "validity": args.validity, "records": n, "steps": args.steps,
                      "records_per_s": n * args.steps / dt, "ms_per_step": dt / args.steps * 1e3,
                      "stage_ms_per_step": st, "codes_ok": ok,
                      "code_counts": {str(c): int((expect == c).sum()) for c in range(5)},
                      "keys_load_s": load_s, "k_ed25519_keys_ms": key_ms, "mads_per_record": MADS_PER_RECORD,
                      "mads_per_key": MADS_PER_KEY,
                      "verify_kernel_fraction_of_mad_peak":
                          n * MADS_PER_RECORD / verify_s / MAD_PEAK_PER_S if verify_s else None,
                      "keys_kernel_fraction_of_mad_peak":
                          nkeys * MADS_PER_KEY / (key_ms / 1e3) / MAD_PEAK_PER_S if key_ms else None,
                      "sclk_mhz_max_seen": clock.mhz,
                      "lib_sha256": hashlib.sha256(open(bls.LIB_PATH, "rb").read()).hexdigest()}))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-pool", action="store_true")
    ap.add_argument("--pool-dir", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", help="write the whole record (JSON) here")
    ap.add_argument("--leg-timeout", type=int, default=150)
    ap.add_argument("--keys", choices=("16", "1M"))
    ap.add_argument("--validity", choices=("valid", "invalid"), default="valid")
    args = ap.parse_args()
    if args.make_pool:
        make_pool(pool_path(args, "16"), 16, 1024)
        make_pool(pool_path(args, "1M"), args.n, args.n)
        return 0
    for k in ((args.keys,) if args.keys else ("16", "1M")):
        if not os.path.exists(pool_path(args, k)):
            sys.exit(f"{pool_path(args, k)} missing: run with --make-pool first (no GPU needed)")
    if args.keys:
        return leg(args)
    runs = []
    for keys, validity in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--keys", keys, "--validity", validity, "--n", str(args.n),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--pool-dir", args.pool_dir]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"leg {keys} {validity} timed out after {args.leg_timeout}s: stopping")
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(f"leg {keys} {validity} failed with {p.returncode}: stopping")
        rec = json.loads(p.stdout.strip().splitlines()[-1])
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"workload": f"{args.n} device-resident records, {MSG_BYTES}-byte messages", "runs": runs}, f,
                      indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
