"""GPU: the RSASSA-PSS check and the store-mode exponentiation kernels over every byte phase and class edge.
Every expected code is the model's (tests/rsa_pss_model.py).

k_rsa_pss alone (rsa_pss_em_batch) over the records of tests/rsa_pss_sweep.py: all 32 pairs (em_len & 3,
em_bits & 7) at the smallest sizes, at 2041..2072 and at 4081..4112 bits, ps_len 0..11, the salt's mask at
r = 1, 2, 3, 4, h - 1, h, one changed bit at every byte position: shuffled (lanes of a wave differ in em_len,
phase, r and MGF1 trip count; the records of wrong length are left out of the list, so list entry t is not
record t), sorted by size (a wave runs one size), and a batch with the failing records at the wave's edges.

The keys of tests/golden/rsa_pss_phase_keys.json.gz through the verification entries: the key-uniform store
twin with m of 65 words, a leading zero byte in word 64 and the largest key of the compile-time class; the
unsorted lists over a table with no loop-form key; the loop-form class at phase 3 and at its largest key."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import rsa_pss_model as model  # noqa: E402
import rsa_pss_sweep as sweep  # noqa: E402
from gen_rsa_pss_edges import EM_CASES, LEAD, craft  # noqa: E402
from test_gpu_rsa_pss import _bitmap_of, _cols, _device_codes, _load  # noqa: E402

pytestmark = pytest.mark.gpu
OK, SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH, KEY = range(6)
DIGESTS = ("SHA256", "SHA384", "SHA512")
EDGE_SIZES = (2058, 2065, 2070, 4112)


@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=4096, profile=True)      # (stage statistics tell which list path a call took)
    yield c
    c.close()


def _load_fx(name):
    fx = model.load_fixture(name)
    fx["ders"] = [bytes.fromhex(t["der"]) for t in fx["table"]]
    for k in fx["keys"]:
        for f_ in ("n", "e", "d"):
            if f_ in k:
                k[f_] = int(k[f_], 16)
    fx["by_name"] = {k["name"]: i for i, k in enumerate(fx["keys"])}
    return fx


@pytest.fixture(scope="module")
def edges():
    return _load_fx("rsa_pss_edges.json.gz")


@pytest.fixture(scope="module")
def phase():
    return _load_fx("rsa_pss_phase_keys.json.gz")


# --- k_rsa_pss alone over the sweep ----------------------------------------------------------------------
def _em_batch_against_model(ctx, name, recs):
    got = ctx.rsa_pss_em_batch(model.DIGEST_ID[name], [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
    assert len(got) == len(recs)
    bad = [sweep.where(r) + (g,) for r, g in zip(recs, got) if g != (OK if r[3] else MISMATCH)]
    assert not bad, (name, len(bad), "of", len(recs), "(bits, tag, byte position, code):", bad[:20])


@pytest.mark.parametrize("name", DIGESTS)
def test_sweep_mixed_waves(ctx, name):
    recs = list(sweep.sweep(name))
    random.Random(0x6d6978).shuffle(recs)
    # the records of wrong length never reach the kernel's list: from the first of them on, list entry t is not record t
    first = next(i for i, r in enumerate(recs) if len(r[1]) != sweep.metrics(name, r[0])["k"])
    assert first < 1000 and sum(r[3] for r in recs[first:]) > 400
    sizes_per_wave = [len({r[0] for r in recs[i:i + 64]}) for i in range(0, len(recs) - 64, 64)]
    assert min(sizes_per_wave) > 8
    _em_batch_against_model(ctx, name, recs)


@pytest.mark.parametrize("name", DIGESTS)
def test_sweep_uniform_waves(ctx, name):
    recs = sorted(sweep.sweep(name), key=lambda r: r[0])
    assert [r[0] for r in recs[-64:]] == [model.GPU_MAX_BITS] * 64
    _em_batch_against_model(ctx, name, recs)


@pytest.mark.parametrize("name", DIGESTS)
def test_sweep_wave_edges(ctx, name):
    """257 records, the sizes 2058, 2065, 2070 and 4112 bits in rotation, all valid but those at the edges of
    the waves and of the 256-lane block"""
    bad_at = (0, 63, 64, 127, 128, 255, 256)
    pool = {b: ([r for r in sweep.sweep(name) if r[0] == b and r[3]],
                [r for r in sweep.sweep(name) if r[0] == b and not r[3] and len(r[1]) == sweep.metrics(name, b)["k"]])
            for b in EDGE_SIZES}
    recs = []
    for i in range(257):
        valid, invalid = pool[EDGE_SIZES[(i + i // 64) % 4]]     # (the rotation moves on by one per wave: each size fails somewhere)
        assert len(valid) == 3 and len(invalid) > 256
        recs.append(invalid[(37 * i) % len(invalid)] if i in bad_at else valid[(i // 4) % 3])
    assert [not r[3] for r in recs] == [i in bad_at for i in range(257)]
    assert {recs[i][0] for i in bad_at} == set(EDGE_SIZES)
    _em_batch_against_model(ctx, name, recs)


# --- the phase keys through the verification entries ----------------------------------------------------------
def _rows(fx, name, key_name, ti):
    """(table index ti, msg, sig, code) of the fixture's rows of one key and digest"""
    ki = fx["by_name"][key_name]
    return [(ti, bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"]) for r in fx["rows"]
            if r["digest"] == name and r["key"] == ki]


def _signed_here(key, name, ti, rng):
    """about 20 records signed under a key that has d: every crafted case of the edge fixture and valid
    signatures over messages of other lengths, each with the model's code"""
    out = []
    k = (key["bits"] + 7) // 8
    cases = list(EM_CASES) + ([LEAD] if key["bits"] % 8 == 1 else [])
    cases += ["valid"] * (20 - len(cases))
    for i, case in enumerate(cases):
        msg = bytes(rng.randrange(256) for _ in range((1, 33, 55, 64, 200)[i % 5]))
        while True:                                          # a crafted EM at or above n: draw again
            v = int.from_bytes(craft(name, msg, key["bits"], rng, case), "big")
            if v < key["n"]:
                break
        vmsg = bytes([msg[0] ^ 1]) + msg[1:] if case == "msg_changed" else msg
        sig = pow(v, key["d"], key["n"]).to_bytes(k, "big")
        code = model.verify_code(name, key["n"], key["e"], vmsg, sig)
        assert (code == OK) == (case == "valid") and code in (OK, MISMATCH), (key["name"], case)
        out.append((ti, vmsg, sig, code))
    return out


P_SMALL, K_SMALL = ("p2058", "p2065", "p2070"), ("k2041", "k2049", "k2056")


@pytest.fixture(scope="module")
def small_table(edges, phase):
    """the table with no loop-form key (p2058, p2065, p2070, k2041, k2049, k2056) and, per digest and table
    index, the records of that key with their codes: fixture rows, and for the p keys records signed here"""
    ders = [phase["ders"][phase["by_name"][n]] for n in P_SMALL] + [edges["ders"][edges["by_name"][n]] for n in K_SMALL]
    pools = {}
    for name in DIGESTS:
        rng = random.Random(0x7368 + model.DIGEST_ID[name])
        per_key = []
        for ti, kn in enumerate(P_SMALL):
            per_key.append(_rows(phase, name, kn, ti) + _signed_here(phase["keys"][phase["by_name"][kn]], name, ti, rng))
        for ti, kn in enumerate(K_SMALL, len(P_SMALL)):
            per_key.append(_rows(edges, name, kn, ti))
        for p in per_key:
            assert OK in {r[3] for r in p} and MISMATCH in {r[3] for r in p}
        pools[name] = per_key
    return ders, pools


@pytest.mark.parametrize("name", DIGESTS)
def test_key_uniform_store_twin_on_the_phase_keys(ctx, small_table, name):
    """k_rsa_verify_2048um and k_rsa_pss over key-uniform lists: 260 records per key, above the threshold of 256;
    m of 65 words (k = 258, 259), a leading zero byte in word 64, the largest key of the class, beside keys of 64
    and 65 words with the other phases; a failing record at lanes 0, 63 and 64 of every key's segment"""
    ders, pools = small_table
    dg = model.DIGEST_ID[name]
    assert _load(ctx, ders) == [0] * 6
    recs = []
    for pool in pools[name]:
        valid, invalid = [r for r in pool if r[3] == OK], [r for r in pool if r[3] != OK]
        seg = [pool[i % len(pool)] for i in range(260)]
        for j, i in enumerate((0, 63, 64)):
            seg[i] = invalid[j % len(invalid)]
        for j, i in enumerate((1, 62, 65)):
            seg[i] = valid[j % len(valid)]
        recs += seg
    want = [r[3] for r in recs]
    assert len(recs) == 6 * 260 and set(want) == {OK, MISMATCH} and want.count(OK) > 6 * 30
    ctx.rsa_pss_stage_stats(reset=True)
    codes, bitmap = ctx.rsa_verify_pss_batch(dg, *_cols(recs), with_bitmap=True)
    st = ctx.rsa_pss_stage_stats(reset=True)
    assert st["k_rsa_pss_u"][1] == 1 and st["k_rsa_pss"][1] == 0          # the key-uniform lists
    bad = [(i, r[0], g, w) for i, (r, g, w) in enumerate(zip(recs, codes, want)) if g != w]
    assert not bad, (len(bad), "(record, key, code, model's code):", bad[:20])
    assert bitmap == _bitmap_of(want)
    assert _device_codes(ctx, dg, recs) == want


@pytest.mark.parametrize("name", DIGESTS)
def test_unsorted_lists_without_a_loop_form_key(ctx, small_table, name):
    """the same table with 65 records, below the key-uniform threshold: k_rsa_verify_2048m and k_rsa_pss over
    the unsorted list, where the buffer of m has no loop-form part"""
    ders, pools = small_table
    dg = model.DIGEST_ID[name]
    assert _load(ctx, ders) == [0] * 6
    recs = [pool[i] for i in range(27) for pool in pools[name] if i < len(pool)][:65]      # the keys in turn
    want = [r[3] for r in recs]
    assert len(recs) == 65 and {r[0] for r in recs} == set(range(6)) and set(want) == {OK, MISMATCH}
    ctx.rsa_pss_stage_stats(reset=True)
    codes, bitmap = ctx.rsa_verify_pss_batch(dg, *_cols(recs), with_bitmap=True)
    st = ctx.rsa_pss_stage_stats(reset=True)
    assert st["k_rsa_pss"][1] == 1 and st["k_rsa_pss_u"][1] == 0          # the unsorted lists
    assert list(codes) == want and bitmap == _bitmap_of(want)
    assert _device_codes(ctx, dg, recs) == want


@pytest.mark.parametrize("name", DIGESTS)
def test_loop_form_class_at_phase_3_and_at_its_largest_key(ctx, edges, phase, name):
    """a2048, p3090 (k = 387: phase 3) and p4112 (k = 514, 129 words: the largest key the GPU verifies) in one
    table, through the host-buffer, the device-resident and the one-record entries"""
    from cess_amd import bls
    dg = model.DIGEST_ID[name]
    ders = [edges["ders"][edges["by_name"]["a2048"]], phase["ders"][phase["by_name"]["p3090"]],
            phase["ders"][phase["by_name"]["p4112"]]]
    assert _load(ctx, ders) == [0, 0, 0]
    recs = _rows(edges, name, "a2048", 0)[:12] + _rows(phase, name, "p3090", 1) + _rows(phase, name, "p4112", 2)
    random.Random(0x6c66).shuffle(recs)
    want = [r[3] for r in recs]
    assert len(recs) == 24 and want.count(OK) >= 3 and MISMATCH in want
    ctx.rsa_pss_stage_stats(reset=True)
    codes, bitmap = ctx.rsa_verify_pss_batch(dg, *_cols(recs), with_bitmap=True)
    st = ctx.rsa_pss_stage_stats(reset=True)
    assert st["k_rsa_pss"][1] == 1 and st["k_rsa_pss_u"][1] == 0
    assert list(codes) == want and bitmap == _bitmap_of(want)
    assert _device_codes(ctx, dg, recs) == want
    for ti, msg, sig, code in recs:
        if ti:
            assert ctx.verify_rsa_pss(dg, ders[ti], msg, sig, bls.RSA_KEY_PKCS1) == (code == OK), (ti, code)
