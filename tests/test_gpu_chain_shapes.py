"""GPU: the device-resident entry point at the batch sizes where a block of the
staged kernels is partial -- n = 129 (one full 128-signature block of the
lane-pair kernels k_miller2 / k_final2 plus a block of one signature) and
n = 257 (one full 256-thread block of the light kernels plus one lane).

Every fixed-length record of tests/golden/vectors.json stands at both ends of
a batch (first and last records, so in the full block's first lanes and in the
partial block), with records signed by the library's own keygen and sign
kernels between them.  A batch of n = 129 cannot hold all 66 golden records
twice and still keep signed ones, so each n runs ceil(66 / (n // 3)) batches,
each with the next n // 3 golden records at its front and again at its end.
Codes are compared with the golden codes (0 for the signed records), and the
verdict bitmap with the codes.  The `ctx` fixture runs both execution shapes;
"pipeline" is the six-kernel path of the large batches.

tests/test_gpu_final_program.py runs the same two sizes through the host-buffer
entry point with golden valid and forged records; this file adds the
device-resident entry point, records signed by the library, and every golden
record (malformed and non-subgroup ones included) at the batch ends."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@pytest.mark.parametrize("n", [129, 257])
def test_verify_device_partial_blocks(ctx, vectors, n):
    cases = [(bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"]), c["code"])
             for c in vectors["cases"] if len(c["sig"]) == 96 and len(c["pk"]) == 192]
    assert len(cases) == 66
    rng = random.Random(n)
    sks = [rng.randrange(1, R).to_bytes(32, "big") for _ in range(n)]
    smsgs = [rng.randbytes(32) for _ in range(n)]
    ssigs, spks = ctx.sign(sks, smsgs), ctx.public_keys(sks)
    per = min(len(cases), n // 3)
    wpr = (n + 63) // 64
    seen = 0
    for lo in range(0, len(cases), per):
        part = cases[lo:lo + per]
        recs = [(ssigs[i], smsgs[i], spks[i], 0) for i in range(n)]
        recs[:len(part)] = part
        recs[n - len(part):] = part
        assert sum(1 for r in recs[len(part):n - len(part)] if r[3] == 0) >= n - 2 * per
        S, M, P = (b"".join(r[k] for r in recs) for k in (0, 1, 2))
        offs = np.concatenate([[0], np.cumsum([len(r[1]) for r in recs])]).astype(np.uint64)
        bufs = [ctx.to_device(S), ctx.to_device(P), ctx.to_device(M or b"\0"), ctx.to_device(offs),
                ctx.device_alloc(wpr * 64), ctx.device_alloc(wpr * 8)]
        try:
            ctx.verify_device(n, *bufs)
            ctx.synchronize()
            codes = ctx.from_device(bufs[4], n)
            words = np.frombuffer(ctx.from_device(bufs[5], wpr * 8), dtype=np.uint64)
        finally:
            for d in bufs:
                ctx.device_free(d)
        assert list(codes) == [r[3] for r in recs]
        bits = [(int(words[i >> 6]) >> (i & 63)) & 1 for i in range(n)]
        assert bits == [int(c == 0) for c in codes]
        assert int(words[-1]) >> (n - 64 * (wpr - 1)) == 0      # no bits set past the last record
        seen += len(part)
    assert seen == len(cases)
