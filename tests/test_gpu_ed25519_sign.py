"""GPU: the Ed25519 signer (include/cess_ed25519_sign.h) through every entry point, against ring's own
vectors (tests/golden/ring_ed25519.json, byte for byte) and the edge fixture
(tests/golden/ed25519_sign_edges.json); what it signs goes back through the library's verifier."""
import ctypes
import json
import os

import numpy as np
import pytest

import ed25519_model as model
from test_ed25519_sign import edges, ring  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGN_BLOCK = 256


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=1024)
    yield c
    c.close()


def device_sign(c, idx, msgs, with_codes=True):
    M = b"\xa5" + b"".join(msgs)          # messages start at an odd device address
    mo = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    n = len(idx)
    d = [c.to_device(np.array(idx, dtype=np.uint32)), c.to_device(M), c.to_device(mo)]
    ds, dc = c.device_alloc(64 * n), c.device_alloc(n)
    try:
        c.ed25519_sign_batch_device(n, d[0], d[1] + 1, d[2], ds, dc if with_codes else 0)
        c.synchronize()
        raw = c.from_device(ds, 64 * n)
        return [raw[64 * i:64 * (i + 1)] for i in range(n)], (c.from_device(dc, n) if with_codes else None)
    finally:
        for p in d + [ds, dc]:
            c.device_free(p)


def test_gpu_reference_rows(ctx, ring):
    """323 signers, each row's own message: the keys and signatures are ring's; the verifier accepts them."""
    from cess_amd import bls
    seeds, pubs, msgs, sigs = (list(col) for col in zip(*ring))
    got_pubs, st = ctx.ed25519_signers_load(seeds, expected_pubs=pubs)
    assert st == [0] * 323 and got_pubs == pubs
    got, codes = ctx.ed25519_sign_batch(list(range(323)), msgs, with_codes=True)
    assert got == sigs and codes == bytes(323)
    assert ctx.ed25519_keys_load(got_pubs) == [0] * 323
    assert ctx.ed25519_verify_batch(list(range(323)), msgs, got) == bytes(323)
    for i in range(0, 323, 40):
        assert ctx.sign_ed25519(seeds[i], msgs[i], with_public_key=True) == (sigs[i], pubs[i])
        assert bls.sign_ed25519(seeds[i], msgs[i], ctx=ctx) == sigs[i]
    key = bls.Ed25519PrivateKey.from_seed(seeds[7], ctx=ctx)
    assert key.public_key() == pubs[7] and key.sign(msgs[7]) == sigs[7]
    # the single-record entry used a table of its own: the loaded one is still in place
    assert ctx.ed25519_sign_batch([5, 6], msgs[5:7]) == sigs[5:7]
    with pytest.raises(bls.BlsInfraError) as ei:
        ctx.sign_ed25519(seeds[0][:31], b"m")
    assert ei.value.status == bls.E_BAD_KEY


def test_gpu_edges(ctx, edges):
    rows = edges["rows"]
    seeds = list(dict.fromkeys(r[1] for r in rows))
    pub_of = {r[1]: r[2] for r in rows}
    pubs, st = ctx.ed25519_signers_load(seeds)
    assert st == [0] * 4 and pubs == [pub_of[s] for s in seeds]
    idx = [seeds.index(r[1]) for r in rows]
    msgs, want = [r[3] for r in rows], [r[4] for r in rows]
    got = ctx.ed25519_sign_batch(idx, msgs)
    assert got == want, [r[0] for r, g in zip(rows, got) if g != r[4]]
    assert device_sign(ctx, idx, msgs) == (want, bytes(len(rows)))
    for name, seed, pub, msg, sig in rows[::5]:
        assert ctx.sign_ed25519(seed, msg, with_public_key=True) == (sig, pub), name


@pytest.fixture(scope="module")
def sixteen(ring):
    """16 signers from the reference rows and, per batch size, messages cycled from them with the
    model's signatures (computed once)"""
    seeds = [r[0] for r in ring[:16]]
    cache = {}

    def recs(n):
        idx = [(7 * i) % 16 for i in range(n)]
        msgs = [ring[(i % 20) * 16][2] for i in range(n)]
        for s, m in zip(idx, msgs):
            if (s, m) not in cache:
                cache[(s, m)] = model.sign(seeds[s], m)
        return idx, msgs, [cache[(s, m)] for s, m in zip(idx, msgs)]
    return seeds, recs


@pytest.mark.parametrize("n", [1, 63, 64, 65, SIGN_BLOCK - 1, SIGN_BLOCK, SIGN_BLOCK + 1])
def test_gpu_batch_sizes(ctx, ring, sixteen, n):
    seeds, recs = sixteen
    pubs, st = ctx.ed25519_signers_load(seeds)
    assert st == [0] * 16 and pubs == [r[1] for r in ring[:16]]
    idx, msgs, want = recs(n)
    got, codes = ctx.ed25519_sign_batch(idx, msgs, with_codes=True)
    assert got == want and codes == bytes(n)


def test_gpu_codes_in_neighbouring_lanes(ctx, ring):
    """Signer indices at and past the table's end and signers that did not load, between good ones: code 1
    and 64 zero bytes for them, the good neighbours exact."""
    from cess_amd import bls
    seeds = [r[0] for r in ring[:8]]
    table = seeds[:4] + [seeds[4][:31]] + seeds[5:8] + [b""]
    expected = [r[1] for r in ring[:8]] + [bytes(32)]
    expected[6] = bytes([expected[6][5] ^ 0x10]) * 32
    pubs, st = ctx.ed25519_signers_load(table, expected_pubs=expected)
    assert st == [0, 0, 0, 0, bls.E_BAD_KEY, 0, bls.ED25519_E_INCONSISTENT, 0, bls.E_BAD_KEY]
    assert pubs == [r[1] for r in ring[:4]] + [bytes(32)] + [r[1] for r in ring[5:8]] + [bytes(32)]
    idx, msgs, want, codes = [], [], [], []
    for i in range(70):
        kind = i % 5
        s = (4, 6, 9, 0xFFFFFFFF)[kind - 1] if kind else (0, 1, 2, 3, 5, 7)[i % 6]
        msg = ring[i][2]
        idx.append(s)
        msgs.append(msg)
        want.append(bytes(64) if kind else model.sign(seeds[s], msg))
        codes.append(1 if kind else 0)
    idx[1] = 8                                          # the empty seed at the table's last row
    got, got_codes = ctx.ed25519_sign_batch(idx, msgs, with_codes=True)
    assert list(got_codes) == codes and got == want
    assert device_sign(ctx, idx, msgs) == (want, bytes(codes))


def test_gpu_table_replacement_and_other_schemes(ctx, ring):
    from cess_amd import bls
    seeds, pubs, msgs, sigs = (list(col) for col in zip(*ring[:20]))
    assert ctx.ed25519_signers_load(seeds[:10])[1] == [0] * 10
    assert ctx.ed25519_sign_batch([3, 9], [msgs[3], msgs[9]]) == [sigs[3], sigs[9]]
    # a second load replaces the first: index 3 is another signer, index 9 is past the end
    assert ctx.ed25519_signers_load(seeds[10:15]) == (pubs[10:15], [0] * 5)
    got, codes = ctx.ed25519_sign_batch([3, 9, 0], [msgs[13], msgs[9], msgs[10]], with_codes=True)
    assert got == [sigs[13], bytes(64), sigs[10]] and list(codes) == [0, 1, 0]
    # k = 0 empties the table
    assert ctx.ed25519_signers_load([]) == ([], [])
    assert ctx.ed25519_sign_batch([0], [b"x"], with_codes=True) == ([bytes(64)], b"\x01")
    assert ctx.ed25519_signers_load(seeds[10:15])[1] == [0] * 5
    # the verifier's key table is not the signers': the BLS, RSA and Ed25519-verify sides still answer
    assert ctx.ed25519_keys_load(pubs[:3]) == [0] * 3
    v = _load("vectors.json")["cases"]
    case = next(c for c in v if c["code"] == 0 and len(c["sig"]) == 96)
    assert list(ctx.verify_codes([tuple(bytes.fromhex(case[k]) for k in ("sig", "msg", "pk"))])) == [0]
    row = next(r for r in _load("ring_rsa_pkcs1_sha256.json")["rows"] if r["code"] == 0 and r["key_status"] == "ok")
    assert ctx.verify_rsa_sha256(bytes.fromhex(row["key"]), bytes.fromhex(row["msg"]), bytes.fromhex(row["sig"]),
                                 bls.RSA_KEY_PKCS1) is True
    assert list(ctx.ed25519_verify_batch([0, 1, 2], msgs[:3], sigs[:3])) == [0, 0, 0]
    assert ctx.ed25519_sign_batch([3], [msgs[13]]) == [sigs[13]]
    assert ctx.verify_ed25519(pubs[13], msgs[13], ctx.sign_ed25519(seeds[13], msgs[13])) is True


def test_gpu_device_entry(ctx, ring, sixteen):
    from cess_amd import bls
    lib = bls.load_library()
    seeds, recs = sixteen
    assert ctx.ed25519_signers_load(seeds)[1] == [0] * 16
    idx, msgs, want = recs(130)
    host = ctx.ed25519_sign_batch(idx, msgs)
    assert host == want
    assert device_sign(ctx, idx, msgs) == (host, bytes(130))
    assert device_sign(ctx, idx, msgs, with_codes=False) == (host, None)          # NULL d_codes
    # n = 0: OK, nothing touched, whatever the pointers; NULL codes_out on the host entry
    assert lib.cess_ed25519_sign_batch_device(ctx.handle, 0, None, None, None, None, None, None) == 0
    sig = (ctypes.c_uint8 * 64)(*([0xEE] * 64))
    assert lib.cess_ed25519_sign_batch(ctx.handle, 0, None, None, None, sig, None) == 0 and sig[0] == 0xEE
    assert ctx.ed25519_sign_batch([], []) == []
    a_idx = (ctypes.c_uint32 * 1)(idx[0])
    assert lib.cess_ed25519_sign_batch(ctx.handle, 1, a_idx, bls._buf(msgs[0]), bls._offsets([len(msgs[0])]), sig,
                                       None) == 0
    assert bytes(sig) == want[0]


def test_gpu_two_device_context(ctx, ring, sixteen):
    from cess_amd import bls
    seeds, recs = sixteen
    assert ctx.ed25519_signers_load(seeds)[1] == [0] * 16
    idx, msgs, want = recs(200)
    idx[50], idx[150] = 16, 99
    want[50] = want[150] = bytes(64)
    one = ctx.ed25519_sign_batch(idx, msgs, with_codes=True)
    m = bls.Context(max_batch=1024, devices=[0, 0])
    try:
        assert m.ed25519_signers_load(seeds) == ([r[1] for r in ring[:16]], [0] * 16)
        two = m.ed25519_sign_batch(idx, msgs, with_codes=True)
        assert m.sign_ed25519(ring[0][0], ring[0][2]) == ring[0][3]
    finally:
        m.close()
    assert one[0] == want and list(one[1]) == [1 if i in (50, 150) else 0 for i in range(200)]
    assert two == one


def test_gpu_profile_stages(ring, sixteen):
    from cess_amd import bls
    seeds, recs = sixteen
    idx, msgs, want = recs(70)
    names = ["k_ed25519_comb", "k_ed25519_signers", "k_ed25519_sign_pack", "k_ed25519_sign_r", "k_ed25519_sign_s"]
    c = bls.Context(max_batch=1024, profile=True)
    try:
        before = c.stage_stats(reset=True)
        ed_before = c.ed25519_stage_stats(reset=True)
        assert list(ed_before) == ["k_ed25519_keys", "k_ed25519_pack", "k_ed25519_verify"]
        assert list(c.ed25519_sign_stage_stats(reset=True)) == names
        c.ed25519_signers_load(seeds)
        st = c.ed25519_sign_stage_stats(reset=True)
        assert list(st) == names and [st[k][1] for k in names] == [1, 1, 0, 0, 0]
        assert st["k_ed25519_comb"][0] > 0 and st["k_ed25519_signers"][0] > 0
        assert c.stage_stats(reset=True)["k_rsa_digest"][1] == 1
        c.ed25519_signers_load(seeds)                                   # the comb table is built once per context
        assert [v[1] for v in c.ed25519_sign_stage_stats(reset=True).values()] == [0, 1, 0, 0, 0]
        c.stage_stats(reset=True)
        assert c.ed25519_sign_batch(idx, msgs) == want
        st = c.ed25519_sign_stage_stats(reset=True)
        assert [st[k][1] for k in names] == [0, 0, 2, 1, 1] and all(st[k][0] > 0 for k in names[2:])
        legacy = c.stage_stats(reset=True)
        assert list(legacy) == list(before) and legacy["k_rsa_digest"][1] == 2
        assert [k for k, v in legacy.items() if v[1] and k != "k_rsa_digest"] == []
        # the verifier's list is as it was, and the signer left nothing in it
        ed = c.ed25519_stage_stats(reset=True)
        assert list(ed) == list(ed_before) and all(v == (0.0, 0) for v in ed.values())
        assert c.ed25519_sign_stage_stats(reset=True)["k_ed25519_sign_r"] == (0.0, 0)
    finally:
        c.close()
