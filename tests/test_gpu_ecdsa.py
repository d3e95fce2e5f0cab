"""ECDSA P-256 on the GPU (include/cess_ecdsa.h): every fixture row -- ring's 58,
the crafted ones and the records that steer the ladder into a doubling or a
cancel (tests/golden/ecdsa_ladder.json), these also at the wave's edges among
ordinary and early-leaving records -- through the host batch, the device batch, the
single-record call and, where the machine has two devices, a two-device
context; codes and bitmaps exactly; batch sizes around the wave and the block;
key tables with bad keys in the middle and at both ends; the other families'
tables after an ECDSA load."""
import ctypes

import numpy as np
import pytest

import ecdsa_ladder_model as lm
import ecdsa_model as model
from test_ecdsa import LADDER, ROWS

pytestmark = pytest.mark.gpu
OK = model.OK


@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=1024)
    yield c
    c.close()


def bitmap_of(codes):
    words = [0] * ((len(codes) + 63) // 64)
    for i, c in enumerate(codes):
        if c == OK:
            words[i >> 6] |= 1 << (i & 63)
    return words


def by_alg(alg):
    return [r for r in ROWS if r[1] == alg]


def table_of(rows):
    """distinct keys of the rows and the rows as (index, msg, sig, code) columns; a missing key is an index past the table"""
    keys = list(dict.fromkeys(r[2] for r in rows if r[2] is not None))
    pos = {k: i for i, k in enumerate(keys)}
    idx = [len(keys) + 7 if r[2] is None else pos[r[2]] for r in rows]
    return keys, idx, [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows]


def device_codes(c, alg, idx, msgs, sigs):
    S = b"\x5a\x5a\x5a" + b"".join(sigs)  # signatures and messages start at odd device addresses
    M = b"\xa5" + b"".join(msgs)
    so = np.cumsum([0] + [len(s) for s in sigs]).astype(np.uint64)
    mo = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    d = [c.to_device(np.array(idx, dtype=np.uint32)), c.to_device(S), c.to_device(so), c.to_device(M), c.to_device(mo)]
    dc = c.device_alloc(len(idx))
    try:
        c.ecdsa_verify_batch_device(alg, len(idx), d[0], d[1] + 3, d[2], d[3] + 1, d[4], dc)
        c.synchronize()
        return c.from_device(dc, len(idx))
    finally:
        for p in d + [dc]:
            c.device_free(p)


def load(c, keys):
    from cess_amd import bls
    st = c.ecdsa_keys_load(keys)
    assert st == [0 if model.key_point(k) is not None else bls.E_BAD_KEY for k in keys]


@pytest.mark.parametrize("alg", [0, 1, 2])
def test_every_row_host_and_device(ctx, alg):
    rows = by_alg(alg)
    keys, idx, msgs, sigs, want = table_of(rows)
    load(ctx, keys)
    codes, words = ctx.ecdsa_verify_batch(idx, msgs, sigs, alg=alg, with_bitmap=True)
    assert list(codes) == want, [r[0] for r, c in zip(rows, codes) if c != r[5]]
    assert words == bitmap_of(want) and words[-1] >> ((len(want) - 1) % 64 + 1) == 0
    assert list(device_codes(ctx, alg, idx, msgs, sigs)) == want


def test_every_row_single_call(ctx):
    from cess_amd import bls
    for name, alg, key, msg, sig, code in ROWS:
        if key is None:
            continue
        if model.key_point(key) is not None:
            assert ctx.verify_ecdsa(key, msg, sig, alg) == (code == OK), name
        else:
            with pytest.raises(bls.BlsInfraError) as ei:
                ctx.verify_ecdsa(key, msg, sig, alg)
            assert ei.value.status == bls.E_BAD_KEY
            assert bls.verify_ecdsa(sig, msg, key, alg, ctx=ctx) is False


def test_two_devices():
    from cess_amd import bls
    lib = bls.load_library()
    if lib.cess_bls_device_count() < 2:
        pytest.skip("one device")
    c = bls.Context(max_batch=1024, devices=[0, 1])
    try:
        for alg in range(3):
            keys, idx, msgs, sigs, want = table_of(by_alg(alg))
            load(c, keys)
            codes, words = c.ecdsa_verify_batch(idx, msgs, sigs, alg=alg, with_bitmap=True)
            assert list(codes) == want and words == bitmap_of(want)
    finally:
        c.close()


def cycled(alg, n, nkeys):
    """n records cycled from the valid rows of at most nkeys keys, every fifth with another row's message"""
    good = [r for r in by_alg(alg) if r[5] == OK]
    keys = list(dict.fromkeys(r[2] for r in good))[:nkeys]
    good = [r for r in good if r[2] in keys]
    rows = [good[i % len(good)] for i in range(n)]
    rows = [(r[0], alg, r[2], r[3] + b"#", r[4], model.MISMATCH) if i % 5 == 4 else r for i, r in enumerate(rows)]
    return rows


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_batch_sizes(ctx, n):
    alg = n % 3
    keys, idx, msgs, sigs, want = table_of(cycled(alg, n, 16))
    load(ctx, keys)
    codes, words = ctx.ecdsa_verify_batch(idx, msgs, sigs, alg=alg, with_bitmap=True)
    assert list(codes) == want
    assert words == bitmap_of(want) and words[-1] >> ((n - 1) % 64 + 1) == 0


EDGE_LANES = (0, 31, 32, 63)


def ladder_pool(alg):
    """the valid records of tests/golden/ecdsa_ladder.json under `alg`, each with the (round, addend, kind) that
    the ladder takes on it -- traced here on scalars from the fixture's d, not read from its name -- and the twins"""
    ok, twins = [], []
    for r in LADDER["rows"]:
        if r["alg"] != alg:
            continue
        row = (r["name"], alg, bytes.fromhex(r["key"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"])
        assert row in ROWS
        if r["code"] != OK:
            twins.append(row)
            continue
        rr, ss = (int.from_bytes(b, "big") for b in model.split_sig(alg, row[4]))
        w = lm.inv(ss)
        events, _ = lm.trace(model.digest_scalar(alg, row[3]) * w % model.N, rr * w % model.N, int(r["d"], 16))
        target = (r["round"], r["addend"], r["kind"])
        assert target in events, r["name"]
        ok.append((row, target))
    return ok, twins


@pytest.mark.parametrize("n", [64, 65, 257])
@pytest.mark.parametrize("alg", [0, 1, 2])
def test_ladder_rows_at_wave_edges_among_ordinary_and_early_rows(ctx, n, alg):
    """Valid records of tests/golden/ecdsa_ladder.json -- a doubling or a cancel inside the ladder, each traced
    above to the event it takes -- at lanes 0, 31, 32 and 63 of every wave.  Around them valid ordinary records,
    the ladder records' twins (one more message byte), and records that leave before the ladder (KEY,
    SIG_FORMAT).  One batch per rotation of the ladder records over the edge lanes, so that every edge lane of
    every wave holds every one of them once: both kinds, both additions, rounds 0 and 1, and round 2 under the
    fixed-length algorithm.  Codes from the fixtures, and the bitmap."""
    ok, twins = ladder_pool(alg)
    rest = [r for r in by_alg(alg) if not r[0].startswith("ladder: ")]
    valid = [r for r in rest if r[5] == OK]
    early = {code: [r for r in rest if r[5] == code] for code in (model.KEY, model.SIG_FORMAT)}
    assert len(ok) >= 8 and len(twins) == len(ok) and len(valid) >= 8 and all(early.values())
    edges = [i for i in range(n) if i % 64 in EDGE_LANES]
    seen = {i: set() for i in edges}
    for rot in range(len(ok)):
        recs = []
        for i in range(n):
            if i in seen:
                row, target = ok[(edges.index(i) + rot) % len(ok)]
                seen[i].add(target)
                recs.append(row)
            elif i % 8 == 1:
                recs.append(early[model.KEY][(i // 8 + rot) % len(early[model.KEY])])
            elif i % 8 == 2:
                recs.append(early[model.SIG_FORMAT][(i // 8 + rot) % len(early[model.SIG_FORMAT])])
            elif i % 8 == 5:
                recs.append(twins[(i // 8 + rot) % len(twins)])
            else:
                recs.append(valid[(i + rot) % len(valid)])
        keys, idx, msgs, sigs, want = table_of(recs)
        assert {OK, model.MISMATCH, model.KEY, model.SIG_FORMAT} <= set(want) and all(want[i] == OK for i in edges)
        load(ctx, keys)
        codes, words = ctx.ecdsa_verify_batch(idx, msgs, sigs, alg=alg, with_bitmap=True)
        assert list(codes) == want, (rot, [(i, r[0]) for i, (r, c) in enumerate(zip(recs, codes)) if c != r[5]])
        assert words == bitmap_of(want) and words[-1] >> ((n - 1) % 64 + 1) == 0
        assert list(device_codes(ctx, alg, idx, msgs, sigs)) == want, rot
    # what every edge lane has held: each (round, addend, kind) of this algorithm's records
    every = {t for _, t in ok}
    assert every >= {(k, a, kind) for k in (0, 1) for a in lm.ADDENDS for kind in lm.KINDS}
    assert alg != model.ALG_P256_SHA256_FIXED or {(2, "Q", "dbl"), (2, "Q", "cancel")} <= every
    assert {i % 64 for i in edges} == set(EDGE_LANES) and all(seen[i] == every for i in edges)


# tables of 1, 3 and 65 keys: a bad key in the middle among good ones, bad keys at both ends around good
# ones, and for comparison no bad key and (one key) only a bad one
@pytest.mark.parametrize("k,bad", [(1, ()), (1, (0,)), (3, ()), (3, (1,)), (3, (0, 2)), (65, (32,)), (65, (0, 64)),
                                   (65, (0, 32, 64))])
def test_key_tables_with_bad_keys(ctx, k, bad):
    from cess_amd import bls
    alg = 1
    good = [r for r in by_alg(alg) if r[5] == OK]
    pool = list(dict.fromkeys(r[2] for r in good))
    keys = [pool[i % len(pool)] for i in range(k)]
    bad = set(bad)
    for j in bad:
        keys[j] = keys[j][:64] + bytes([keys[j][64] ^ 1])
    st = ctx.ecdsa_keys_load(keys)
    assert st == [bls.E_BAD_KEY if j in bad else 0 for j in range(k)]
    first = {}
    for r in good:
        first.setdefault(r[2], r)
    idx = list(range(k)) + [k, 2 ** 32 - 1]
    recs = [first[pool[j % len(pool)]] for j in range(k)] + [good[0], good[0]]
    want = [model.KEY if j in bad else OK for j in range(k)] + [model.KEY, model.KEY]
    codes, words = ctx.ecdsa_verify_batch(idx, [r[3] for r in recs], [r[4] for r in recs], alg=alg, with_bitmap=True)
    assert list(codes) == want and words == bitmap_of(want)
    # the table replaced: the same indices now mean other keys
    ctx.ecdsa_keys_load(pool[1:2])
    assert list(ctx.ecdsa_verify_batch([0, 1], [recs[0][3]] * 2, [recs[0][4]] * 2, alg=alg)) == [
        OK if pool[1] == recs[0][2] else model.MISMATCH, model.KEY]
    ctx.ecdsa_keys_load([])
    assert list(ctx.ecdsa_verify_batch([0], [recs[0][3]], [recs[0][4]], alg=alg)) == [model.KEY]


def test_empty_batch_and_null_outputs(ctx):
    from cess_amd import bls
    lib = bls.load_library()
    codes = (ctypes.c_uint8 * 1)(0xEE)
    words = (ctypes.c_uint64 * 1)(0x1234)
    assert lib.cess_ecdsa_verify_batch(ctx.handle, 1, 0, None, None, None, None, None, codes, words) == 0
    assert codes[0] == 0xEE and words[0] == 0x1234
    assert lib.cess_ecdsa_verify_batch_device(ctx.handle, 1, 0, None, None, None, None, None, None, None) == 0
    assert ctx.ecdsa_verify_batch([], [], []) == b""
    assert lib.cess_ecdsa_verify_batch(ctx.handle, 3, 0, None, None, None, None, None, codes, words) == bls.E_INVALID_ARG
    n = 65
    keys, idx, msgs, sigs, want = table_of(cycled(1, n, 4))
    load(ctx, keys)
    a_idx = (ctypes.c_uint32 * n)(*idx)
    S, M = bls._buf(b"".join(sigs)), bls._buf(b"".join(msgs))
    so, mo = bls._offsets([len(s) for s in sigs]), bls._offsets([len(m) for m in msgs])
    codes = (ctypes.c_uint8 * n)(*([0xEE] * n))
    words = (ctypes.c_uint64 * 2)(2 ** 64 - 1, 2 ** 64 - 1)
    assert lib.cess_ecdsa_verify_batch(ctx.handle, 1, n, a_idx, S, so, M, mo, codes, None) == 0
    assert list(codes) == want
    assert lib.cess_ecdsa_verify_batch(ctx.handle, 1, n, a_idx, S, so, M, mo, None, words) == 0
    assert list(words) == bitmap_of(want)


def test_other_tables_survive_and_stage_stats(ctx):
    """The RSA and Ed25519 tables, loaded before the ECDSA table, still answer after an ECDSA load and an ECDSA
    batch (which runs the digest kernel the hashed RSA mode shares)."""
    import json
    import os

    import ed25519_model as ed
    from cess_amd import bls
    here = os.path.dirname(os.path.abspath(__file__))
    load_json = lambda name: json.load(open(os.path.join(here, "golden", name)))  # noqa: E731
    k, m_, s = [bytes.fromhex(load_json("ring_ed25519.json")["rows"][0][f]) for f in ("pub", "msg", "sig")]
    assert ed.verify_code(k, m_, s) == 0
    rsa = [r for r in load_json("ring_rsa_pkcs1_sha256.json")["rows"] if r["key_status"] == "ok"]
    r_ok = next(r for r in rsa if r["code"] == 0)
    r_bad = next(r for r in rsa if r["code"] != 0)
    ders = [bytes.fromhex(r_ok["key"]), bytes.fromhex(r_bad["key"])]
    r_idx, r_msgs = [0, 1], [bytes.fromhex(r_ok["msg"]), bytes.fromhex(r_bad["msg"])]
    r_sigs, r_want = [bytes.fromhex(r_ok["sig"]), bytes.fromhex(r_bad["sig"])], [r_ok["code"], r_bad["code"]]
    assert ctx.rsa_keys_load(ders, bls.RSA_KEY_PKCS1, policy=bls.RSA_POLICY_RING_2048_8192) == [0, 0]
    assert list(ctx.rsa_verify_sha256_batch(r_idx, r_msgs, r_sigs)) == r_want
    assert ctx.ed25519_keys_load([k]) == [0]
    for alg in range(3):
        keys, idx, msgs, sigs, want = table_of(cycled(alg, 8, 2))
        load(ctx, keys)
        assert list(ctx.ecdsa_verify_batch(idx, msgs, sigs, alg=alg)) == want
        assert list(ctx.rsa_verify_sha256_batch(r_idx, r_msgs, r_sigs)) == r_want
        assert list(ctx.ed25519_verify_batch([0], [m_], [s])) == [0]
    assert ctx.verify_rsa_sha256(ders[0], r_msgs[0], r_sigs[0], bls.RSA_KEY_PKCS1) is True
    assert ctx.verify_rsa_sha256(ders[1], r_msgs[1], r_sigs[1], bls.RSA_KEY_PKCS1) is False
    # and the ECDSA table is untouched by the other families' calls
    assert list(ctx.ecdsa_verify_batch(idx, msgs, sigs, alg=2)) == want
    assert set(ctx.ecdsa_stage_stats()) == {"k_ecdsa_keys", "k_ecdsa_pack", "k_ecdsa_verify"}
