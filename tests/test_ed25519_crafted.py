"""Crafted Ed25519 inputs judged by ring's own C code.

tests/golden/ring_ed25519_crafted.json (tests/golden/gen_ring_ed25519_crafted.py)
holds records under torsion and mixed-order keys, non-canonical encodings of
keys and of R, edge values of S, and sc_reduce inputs; every expected code,
"decodes" flag, x and reduced scalar in it was returned by
third_party/fiat/curve25519.c of the reference tree behind
oracle/ring_ed25519_driver.c, not by this project's reading of ring.

CPU: the plain-Python model, the host build of ed25519.hpp and (in
tests/test_ed25519.py) the stand-alone sanitizer program reproduce every row;
where the reference tree and gcc are present the oracle is rebuilt and every
row re-derived from it.
GPU: the rows through the batch entry, the device entry (also with the first
message offset not zero) and, for a sample, the single-record entry.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import ed25519_model as model
import ed25519_probe_model as pm
from test_ed25519 import _emu, bitmap_of, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = model.P, model.L
OK, SIG_LEN, SIG_RANGE, KEY, MISMATCH = range(5)
GROUPS = {"torsion_key", "mixed_key", "noncanonical", "scalar"}


def load_crafted():
    with open(os.path.join(ROOT, "tests", "golden", "ring_ed25519_crafted.json")) as f:
        d = json.load(f)
    rows = [(r["name"], r["group"], bytes.fromhex(r["key"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"])
            for r in d["rows"]]
    keys = [(bytes.fromhex(k["key"]), k["loads"], None if k["x"] is None else int.from_bytes(bytes.fromhex(k["x"]), "little"))
            for k in d["keys"]]
    red = [(bytes.fromhex(r["x"]), bytes.fromhex(r["out"]), r["subs"]) for r in d["reduce"]]
    return {"rows": rows, "keys": keys, "reduce": red}


@pytest.fixture(scope="module")
def crafted():
    return load_crafted()


@pytest.fixture(scope="module")
def emu():
    return _emu()


def test_fixture_shape(crafted):
    rows, keys = crafted["rows"], crafted["keys"]
    assert 300 <= len(rows) <= 600 and {r[1] for r in rows} == GROUPS
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ring_ed25519_crafted.json")) < 200 * 1000
    assert all(len(r[3]) <= 4 and len(r[4]) == 64 and len(r[2]) == 32 for r in rows)
    assert [k[0] for k in keys] == list(dict.fromkeys(r[2] for r in rows))
    by_group = {g: [r for r in rows if r[1] == g] for g in GROUPS}
    for g in ("torsion_key", "mixed_key", "noncanonical", "scalar"):
        assert {OK, MISMATCH} <= {r[5] for r in by_group[g]}, g
    assert KEY in {r[5] for r in by_group["noncanonical"]}
    # the torsion keys: orders 1, 2, 4, 4, 8, 8, 8, 8, then the further encodings of the same points
    tkeys = list(dict.fromkeys(r[2] for r in by_group["torsion_key"]))
    pts = [model.decode_point(k) for k in tkeys]
    assert sorted(pm.order_of(p) for p in {p for p in pts}) == [1, 2, 4, 4, 8, 8, 8, 8]
    assert len(tkeys) > 8 and all(p is not None for p in pts)
    noncanon = [k for k in tkeys if int.from_bytes(k, "little") & (2**255 - 1) >= P]
    sign_zero = [k for k, p in zip(tkeys, pts) if p[0] == 0 and k[31] >> 7]
    assert len(noncanon) >= 3 and len(sign_zero) >= 2
    # y and y + p for y in 0..18 with both sign bits
    nk = {r[2] for r in by_group["noncanonical"]}
    for y in range(19):
        for v in (y, y + P):
            assert {v.to_bytes(32, "little"), (v | 1 << 255).to_bytes(32, "little")} <= nk, y
    # R re-encoded is compared as bytes: never accepted
    for r in by_group["noncanonical"]:
        if " as " in r[0]:
            assert r[5] == MISMATCH, r[0]
    s_vals = {int.from_bytes(r[4][32:], "little") for r in by_group["scalar"] if r[5] == OK}
    assert s_vals == set(pm.S_SET)
    assert {r[2] for r in crafted["reduce"]} == {0, 1, 2, 3}
    assert [int.from_bytes(r[0], "little") for r in crafted["reduce"]] == pm.reduce_inputs()


def test_model_on_crafted(crafted):
    for name, _, key, msg, sig, code in crafted["rows"]:
        assert model.verify_code(key, msg, sig) == code, name
    for key, loads, x in crafted["keys"]:
        pt = model.decode_point(key)
        assert (pt is not None) == loads, key.hex()
        if loads:
            assert pt == (x, (int.from_bytes(key, "little") & (2**255 - 1)) % P), key.hex()
    for x, out, subs in crafted["reduce"]:
        v = int.from_bytes(x, "little")
        assert int.from_bytes(out, "little") == v % L, x.hex()
        assert pm.sc_reduce_subtractions(v) == subs, x.hex()


def test_host_on_crafted(emu, crafted):
    for name, _, key, msg, sig, code in crafted["rows"]:
        assert emu.emu_ed_verify(key, len(key), msg, len(msg), sig, len(sig)) == code, name
    tab = (ctypes.c_uint32 * 240)()
    for key, loads, x in crafted["keys"]:
        assert emu.emu_ed_key_table(key, 32, tab) == (0 if loads else 2), key.hex()
        if loads:
            got = [tuple(pm.value_of(tab[30 * i + 10 * j:30 * i + 10 * j + 10]) % P for j in range(3)) for i in range(8)]
            assert got == model.neg_multiples(key), key.hex()
            y = (int.from_bytes(key, "little") & (2**255 - 1)) % P
            assert got[0] == pm.entry_of((-x % P, y)), key.hex()       # ring's x, not the model's
    out = ctypes.create_string_buffer(32)
    for x, want, _ in crafted["reduce"]:
        emu.emu_ed_sc_reduce(x, out)
        assert out.raw == want, x.hex()
    hi, lo = ctypes.c_uint64(), ctypes.c_uint64()
    emu.emu_ed_col_max(hi, lo, 0)
    assert hi.value == 0


def test_oracle_rebuild(crafted):
    """ring's C, rebuilt from the reference tree, gives every code, flag, x and reduced scalar of the fixture"""
    from oracle import ring_ed25519_ref
    if not ring_ed25519_ref.available():
        pytest.skip("the reference tree or gcc is not here")
    oracle = ring_ed25519_ref.load()
    for name, _, key, msg, sig, code in crafted["rows"]:
        assert oracle.verify_code(key, msg, sig) == code, name
        assert model.verify_code(key, msg, sig) == code, name
    for key, loads, x in crafted["keys"]:
        got = oracle.decode(key)
        assert (got is not None) == loads and (not loads or got[0] == x), key.hex()
        assert got == model.decode_point(key), key.hex()
    for x, out, _ in crafted["reduce"]:
        assert oracle.sc_reduce(x) == out, x.hex()
    # precedence and lengths, which the fixture's 32-byte keys and 64-byte signatures do not reach
    k, m, s = crafted["rows"][0][2:5]
    bad_s = s[:32] + L.to_bytes(32, "little")
    bad_key = next(key for key, loads, _ in crafted["keys"] if not loads)
    for key, sig in ((k[:31], s[:63]), (k, s[:63]), (k, bad_s), (bad_key, bad_s), (bad_key, s), (bad_key, s[:63])):
        assert oracle.verify_code(key, m, sig) == model.verify_code(key, m, sig)


# --- GPU ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=1024)
    yield c
    c.close()


def device_codes(c, idx, msgs, sigs, prefix):
    """the device entry with `prefix` junk bytes in front of the messages, inside
    the same allocation: msg_offsets[0] = len(prefix)"""
    S = b"".join(sigs)
    M = prefix + b"".join(msgs) + b"\x5a" * 3
    so = np.cumsum([0] + [len(s) for s in sigs]).astype(np.uint64)
    mo = (np.cumsum([0] + [len(m) for m in msgs]) + len(prefix)).astype(np.uint64)
    d = [c.to_device(np.array(idx, dtype=np.uint32)), c.to_device(S), c.to_device(so), c.to_device(M), c.to_device(mo)]
    dc = c.device_alloc(len(idx))
    try:
        c.ed25519_verify_batch_device(len(idx), d[0], d[1], d[2], d[3], d[4], dc)
        c.synchronize()
        return c.from_device(dc, len(idx))
    finally:
        for p in d + [dc]:
            c.device_free(p)


@pytest.mark.gpu
def test_gpu_crafted_rows(ctx, crafted):
    from cess_amd import bls
    rows = crafted["rows"]
    loads = {k: ld for k, ld, _ in crafted["keys"]}
    keys, idx, msgs, sigs = table_of([r[2:5] for r in rows])
    assert keys == [k for k, _, _ in crafted["keys"]]
    st = ctx.ed25519_keys_load(keys)
    assert st == [0 if loads[k] else bls.E_BAD_KEY for k in keys], [k.hex() for k, s in zip(keys, st) if (s == 0) != loads[k]]
    want = [r[5] for r in rows]
    codes, words = ctx.ed25519_verify_batch(idx, msgs, sigs, with_bitmap=True)
    assert list(codes) == want, [r[0] for r, c in zip(rows, codes) if c != r[5]]
    assert words == bitmap_of(want)
    at_zero = device_codes(ctx, idx, msgs, sigs, b"")
    assert list(at_zero) == want, [r[0] for r, c in zip(rows, at_zero) if c != r[5]]
    # the same records behind 37 junk bytes: msg_offsets[0] = 37
    shifted = device_codes(ctx, idx, msgs, sigs, bytes(range(0xC0, 0xC0 + 37)))
    assert list(shifted) == list(at_zero)
    # the single-record entry: every seventh row and every accepted one of the small groups
    sample = [r for i, r in enumerate(rows) if i % 7 == 0 or (r[1] in ("scalar", "noncanonical") and r[5] == OK)]
    for name, _, key, msg, sig, code in sample:
        if loads[key]:
            assert ctx.verify_ed25519(key, msg, sig) == (code == OK), name
        else:
            with pytest.raises(bls.BlsInfraError) as ei:
                ctx.verify_ed25519(key, msg, sig)
            assert ei.value.status == bls.E_BAD_KEY
