"""GPU: RSASSA-PSS under ring's RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512 (include/cess_rsa.h).  Every
code is compared with the plain-Python model (tests/rsa_pss_model.py) or with the codes the fixtures
recorded from it: ring's padding rows through the EM check alone, ring's verify rows and the crafted edge
fixture through the host-buffer, device-resident and one-record entries, batch sizes around the wave, the
key-uniform and the unsorted list paths, a two-device context and the profiling stage."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rsa_pss_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
OK, SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH, KEY = range(6)
DIGESTS = ("SHA256", "SHA384", "SHA512")
E_BAD_KEY, E_UNSUPPORTED = -7, -10


@pytest.fixture(scope="module")
def ring():
    return model.load_fixture("ring_rsa_pss.json.gz")


@pytest.fixture(scope="module")
def edges():
    fx = model.load_fixture("rsa_pss_edges.json.gz")
    fx["ders"] = [bytes.fromhex(t["der"]) for t in fx["table"]]
    for k in fx["keys"]:
        for f_ in ("n", "e", "d"):
            if f_ in k:
                k[f_] = int(k[f_], 16)
    fx["recs"] = {d: [(r["key"], bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"], r["case"])
                      for r in fx["rows"] if r["digest"] == d] for d in DIGESTS}
    return fx


@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=4096, profile=True)      # (stage statistics tell which list path a call took)
    yield c
    c.close()


def _cols(recs):
    return [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]


def _bitmap_of(codes):
    words = [0] * ((len(codes) + 63) // 64)
    for i, c in enumerate(codes):
        if c == OK:
            words[i // 64] |= 1 << (i % 64)
    return words


def _device_codes(c, dg, recs):
    S = b"".join(r[2] for r in recs)
    M = b"\xa5" + b"".join(r[1] for r in recs)          # messages start at an odd device address
    so = np.cumsum([0] + [len(r[2]) for r in recs]).astype(np.uint64)
    mo = np.cumsum([0] + [len(r[1]) for r in recs]).astype(np.uint64)
    d = [c.to_device(np.array([r[0] for r in recs], dtype=np.uint32)), c.to_device(S), c.to_device(so),
         c.to_device(M), c.to_device(mo)]
    dc = c.to_device(bytes([0xee]) * len(recs))         # every code must be written
    try:
        c.rsa_verify_pss_batch_device(dg, len(recs), d[0], d[1], d[2], d[3] + 1, d[4], dc)
        c.synchronize()
        return list(c.from_device(dc, len(recs)))
    finally:
        for p in d + [dc]:
            c.device_free(p)


def _load(c, ders):
    from cess_amd import bls
    return c.rsa_keys_load(ders, bls.RSA_KEY_PKCS1, bls.RSA_POLICY_RING_2048_8192)


def test_ring_padding_rows_em_batch(ctx, ring):
    """ring's padding rows up to 4096 bits through k_rsa_pss alone, one launch per digest: lanes of one
    wave differ in em_len, byte phase and MGF1 trip count."""
    seen = set()
    for name in DIGESTS:
        rows = [r for r in ring["padding"] if r["digest"] == name and r["bits"] <= 4096]
        ems = [bytes.fromhex(r["em"]) for r in rows]
        dgs = [model.HASH[name](bytes.fromhex(r["msg"])).digest() for r in rows]
        got = ctx.rsa_pss_em_batch(model.DIGEST_ID[name], [r["bits"] for r in rows], ems, dgs)
        assert list(got) == [r["code"] for r in rows], name
        assert len(rows) >= 14 and OK in got          # (ring's failing SHA-512 rows are all above 4096 bits)
        seen |= {(r["bits"], r["code"]) for r in rows}
    assert {b for b, _ in seen} == {256, 512, 2048, 2049, 2055, 2056, 2057, 4095, 4096}
    assert {c for _, c in seen} == {OK, MISMATCH}


def test_ring_verify_rows_three_entries(ctx, ring):
    from cess_amd import bls
    for name in DIGESTS:
        dg = model.DIGEST_ID[name]
        rows = [r for r in ring["verify"] if r["digest"] == name]
        ders = sorted({r["key"] for r in rows})
        assert _load(ctx, [bytes.fromhex(d) for d in ders]) == [0] * len(ders)
        recs = [(ders.index(r["key"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"])) for r in rows]
        want = [r["code"] for r in rows]
        assert len(rows) == 18 and OK in want and MISMATCH in want
        codes, bitmap = ctx.rsa_verify_pss_batch(dg, *_cols(recs), with_bitmap=True)
        assert list(codes) == want and bitmap == _bitmap_of(want), name
        assert _device_codes(ctx, dg, recs) == want, name
        for r, w in zip(rows, want):
            got = ctx.verify_rsa_pss(dg, bytes.fromhex(r["key"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]),
                                     bls.RSA_KEY_PKCS1)
            assert got == (w == OK) == (r["result"] == "P"), r["comment"]


@pytest.mark.parametrize("name", DIGESTS)
def test_edge_fixture_batch_and_device(ctx, edges, name):
    """the whole edge fixture of one digest in one batch (every key size in one table, so the unsorted lists
    and the loop-form kernel), host-buffer and device-resident, codes and bitmap"""
    st = _load(ctx, edges["ders"])
    assert st == [{"ok": 0, "bad_key": E_BAD_KEY, "unsupported": E_UNSUPPORTED}[t["status"]] for t in edges["table"]]
    recs = edges["recs"][name]
    want = [r[3] for r in recs]
    assert {OK, SIG_LEN, SIG_RANGE, MISMATCH, KEY} == set(want)
    codes, bitmap = ctx.rsa_verify_pss_batch(model.DIGEST_ID[name], *_cols(recs), with_bitmap=True)
    bad = [(r[4], r[0], g, w) for r, g, w in zip(recs, codes, want) if g != w]
    assert not bad, bad
    assert bitmap == _bitmap_of(want)
    assert _device_codes(ctx, model.DIGEST_ID[name], recs) == want


@pytest.mark.parametrize("name", DIGESTS)
def test_edge_fixture_one_record_entry(ctx, edges, name):
    from cess_amd import bls
    dg = model.DIGEST_ID[name]
    for ki, msg, sig, code, case in edges["recs"][name]:
        if ki >= len(edges["ders"]):
            continue
        status = edges["table"][ki]["status"]
        if status == "ok":
            assert ctx.verify_rsa_pss(dg, edges["ders"][ki], msg, sig, bls.RSA_KEY_PKCS1) == (code == OK), case
        else:
            with pytest.raises(bls.BlsInfraError) as ei:
                ctx.verify_rsa_pss(dg, edges["ders"][ki], msg, sig, bls.RSA_KEY_PKCS1)
            assert ei.value.status == (E_BAD_KEY if status == "bad_key" else E_UNSUPPORTED), case


def _sign(key, name, msg, rng):
    h = model.HASH[name]().digest_size
    em = model.encode(name, msg, bytes(rng.randrange(256) for _ in range(h)), key["bits"])
    return pow(int.from_bytes(em, "big"), key["d"], key["n"]).to_bytes((key["bits"] + 7) // 8, "big")


@pytest.fixture(scope="module")
def two_keys(edges):
    """per digest, for the two 2048-bit keys: valid records (the fixture's and a few signed here) and the
    fixture's invalid ones that reach the kernels, as (key, msg, sig), with the model's code of each"""
    rng = random.Random(0x2048)
    out = {}
    for name in DIGESTS:
        valid, invalid = {0: [], 1: []}, {0: [], 1: []}
        for ki, msg, sig, code, case in edges["recs"][name]:
            if ki in (0, 1):
                (valid if code == OK else invalid)[ki].append((ki, msg, sig))
        for ki in (0, 1):
            for ln in (1, 33, 200):
                msg = bytes(rng.randrange(256) for _ in range(ln))
                valid[ki].append((ki, msg, _sign(edges["keys"][ki], name, msg, rng)))
            assert len(invalid[ki]) >= 5
        out[name] = (valid, invalid)
    return out


def _model_codes(edges, name, recs):
    return [model.verify_code(name, edges["keys"][ki]["n"], edges["keys"][ki]["e"], msg, sig) for ki, msg, sig in recs]


def _mixed(two, count, bad_at):
    """`count` records alternating between the two keys' valid pools, an invalid one at each index of bad_at"""
    valid, invalid = two
    recs = []
    for i in range(count):
        ki = i & 1
        pool = invalid[ki] if i in bad_at else valid[ki]
        recs.append(pool[(i // 2) % len(pool)])
    return recs


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_batch_sizes_around_the_wave(ctx, edges, two_keys, count):
    assert _load(ctx, edges["ders"][:2]) == [0, 0]
    bad_at = {i for i in (0, 62, 63, 64, 127, 128, 255, 256) if i < count}
    for name in DIGESTS:
        recs = _mixed(two_keys[name], count, bad_at)
        want = _model_codes(edges, name, recs)
        assert [w != OK for w in want] == [i in bad_at for i in range(count)]
        codes, bitmap = ctx.rsa_verify_pss_batch(model.DIGEST_ID[name], *_cols(recs), with_bitmap=True)
        assert list(codes) == want and bitmap == _bitmap_of(want), (name, count)
        if count in (1, 65):
            assert _device_codes(ctx, model.DIGEST_ID[name], recs) == want


@pytest.mark.parametrize("name", DIGESTS)
def test_key_uniform_and_unsorted_paths(ctx, edges, two_keys, name):
    """two 2048-bit keys with 300 records each (above the key-uniform threshold of 256 per key), 1 % of them
    invalid; then the same records with a 3072-bit key added to the table, which sends them down the
    unsorted lists.  For the valid records the PKCS#1 v1.5 entry over the same (key, msg, sig) is MISMATCH."""
    dg = model.DIGEST_ID[name]
    bad_at = {0, 63, 64, 191, 320, 599}
    recs = _mixed(two_keys[name], 600, bad_at)
    want = _model_codes(edges, name, recs)
    assert sum(w != OK for w in want) == 6 and MISMATCH in want
    assert _load(ctx, edges["ders"][:2]) == [0, 0]
    ctx.rsa_pss_stage_stats(reset=True)
    codes, bitmap = ctx.rsa_verify_pss_batch(dg, *_cols(recs), with_bitmap=True)
    st = ctx.rsa_pss_stage_stats(reset=True)
    assert st["k_rsa_pss_u"][1] == 1 and st["k_rsa_pss"][1] == 0          # the key-uniform lists
    assert list(codes) == want and bitmap == _bitmap_of(want)
    assert _device_codes(ctx, dg, recs) == want
    pk = ctx.rsa_verify_digest_batch(dg, *_cols(recs))
    assert all(p == MISMATCH for p, w in zip(pk, want) if w == OK)
    i3072 = next(i for i, k in enumerate(edges["keys"]) if k["name"] == "k3072")
    assert _load(ctx, edges["ders"][:2] + [edges["ders"][i3072]]) == [0, 0, 0]
    big = next(r for r in edges["recs"][name] if r[0] == i3072 and r[3] == OK)
    recs2 = recs + [(2, big[1], big[2])]
    ctx.rsa_pss_stage_stats(reset=True)
    codes = ctx.rsa_verify_pss_batch(dg, *_cols(recs2))
    st = ctx.rsa_pss_stage_stats(reset=True)
    assert st["k_rsa_pss"][1] == 1 and st["k_rsa_pss_u"][1] == 0          # the unsorted lists
    assert list(codes) == want + [OK]
    assert _device_codes(ctx, dg, recs2) == want + [OK]


def test_unknown_digest_is_invalid_arg(ctx, edges):
    from cess_amd import bls
    _load(ctx, edges["ders"][:1])
    ki, msg, sig = edges["recs"]["SHA256"][0][:3]
    for dg in (3, -1, 0x100):
        with pytest.raises(bls.BlsInfraError) as ei:
            ctx.rsa_verify_pss_batch(dg, [ki], [msg], [sig])
        assert ei.value.status == bls.E_INVALID_ARG
        with pytest.raises(bls.BlsInfraError) as ei:
            ctx.verify_rsa_pss(dg, edges["ders"][0], msg, sig, bls.RSA_KEY_PKCS1)
        assert ei.value.status == bls.E_INVALID_ARG
        with pytest.raises(bls.BlsInfraError) as ei:
            ctx.rsa_pss_em_batch(dg, [2048], [bytes(256)], [bytes(64)])
        assert ei.value.status == bls.E_INVALID_ARG


def test_keys_below_rings_floor_in_another_policys_table(ctx, edges):
    """the batch entries run over whatever table is loaded: under the rsa crate's policy a 2040-bit key (2048-bit
    size class) and a 1024-bit key load, and every ring PSS algorithm rejects both: KEY, beside a 2048-bit key's OK"""
    import oracle.rsa_oracle as o
    from cess_amd import bls
    i2040 = next(i for i, r in enumerate(edges["rows"]) if r["case"] == "key_2040_bits")
    der2040 = edges["ders"][edges["rows"][i2040]["key"]]
    n1024 = o.gen_key(1024, 65537, random.Random(0x1024))[0]
    ders = [der2040, o.encode_pkcs1(n1024, 65537), edges["ders"][0]]
    assert ctx.rsa_keys_load(ders, bls.RSA_KEY_PKCS1, bls.RSA_POLICY_RSA_CRATE) == [0, 0, 0]
    for name in DIGESTS:
        ok = next(r for r in edges["recs"][name] if r[0] == 0 and r[3] == OK)
        recs = [(0, b"m", bytes(254) + b"\x02"), (1, b"m", bytes(127) + b"\x02"), (2, ok[1], ok[2])]
        assert list(ctx.rsa_verify_pss_batch(model.DIGEST_ID[name], *_cols(recs))) == [KEY, KEY, OK]
        assert _device_codes(ctx, model.DIGEST_ID[name], recs) == [KEY, KEY, OK]


def test_two_device_context(edges):
    from cess_amd import bls
    name = "SHA384"
    recs = edges["recs"][name]
    want = [r[3] for r in recs]
    m = bls.Context(max_batch=1024, devices=[0, 0])
    try:
        m.rsa_keys_load(edges["ders"], bls.RSA_KEY_PKCS1, bls.RSA_POLICY_RING_2048_8192)
        codes, bitmap = m.rsa_verify_pss_batch(model.DIGEST_ID[name], *_cols(recs), with_bitmap=True)
        ok = next(r for r in recs if r[3] == OK)
        one = m.verify_rsa_pss(model.DIGEST_ID[name], edges["ders"][ok[0]], ok[1], ok[2], bls.RSA_KEY_PKCS1)
    finally:
        m.close()
    assert len(recs) > 64                                       # both shards hold records
    assert list(codes) == want and bitmap == _bitmap_of(want) and one is True


def test_pss_stage(edges):
    from cess_amd import bls
    recs = edges["recs"]["SHA512"][:40]
    c = bls.Context(max_batch=4096, profile=True)
    try:
        c.rsa_keys_load(edges["ders"], bls.RSA_KEY_PKCS1, bls.RSA_POLICY_RING_2048_8192)
        legacy = list(c.stage_stats(reset=True))
        assert list(c.rsa_pss_stage_stats(reset=True)) == ["k_rsa_pss", "k_rsa_pss_u"]
        c.rsa_verify_pss_batch(model.DIGEST_ID["SHA512"], *_cols(recs))
        st = c.rsa_pss_stage_stats(reset=True)
        assert st["k_rsa_pss"][1] == 1 and st["k_rsa_pss"][0] > 0 and st["k_rsa_pss_u"] == (0.0, 0)
        old = c.stage_stats(reset=True)
        assert list(old) == legacy and "k_rsa_pss" not in old
        assert old["k_rsa_digest"][1] == 1 and old["k_rsa_verify"][1] == 1 and old["k_rsa_classify"][1] == 1
        assert c.rsa_pss_stage_stats()["k_rsa_pss"] == (0.0, 0)
    finally:
        c.close()
