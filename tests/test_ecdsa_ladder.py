"""The ladder of cess_amd/csrc/p256.hpp steered into the special returns of
pt_madd, on the host build: all 256 targets (64 rounds x the Q or the G
addition x doubling or cancel), infinite accumulators doubled through one and
three whole rounds before they are re-entered, and the end cases, through
double_mul, verify_scalars and emu_ecdsa_record, against
tests/ecdsa_ladder_model.py and tests/ecdsa_model.py.  The host build counts
each special return of pt_madd; the counts must equal what the model's trace of
the same scalars predicts, so a row can not claim a branch it does not take.
The same rows run as records (the record path only) through the stand-alone
program under the sanitizers (a child process).  The grinded full records of tests/golden/ecdsa_ladder.json are
checked here against their names; they run through every entry point in
tests/test_ecdsa.py and tests/test_gpu_ecdsa.py.
"""
import ctypes
import os
import subprocess

import pytest

import ecdsa_ladder_model as lm
import ecdsa_model as model
import ecdsa_probe_model as pm
from test_ecdsa import LADDER, ROWS, SAN_ENV, col_max, digest_of, emu_lib, san_exe

N = model.N


@pytest.fixture(scope="module")
def emu():
    e = emu_lib()
    e.emu_ecdsa_madd_counts.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    return e


def madd_counts(emu, reset=True):
    out = (ctypes.c_uint64 * 3)()
    emu.emu_ecdsa_madd_counts(out, 1 if reset else 0)
    return tuple(out)


def run(emu, op, rows, tabs=None, n_tabs=0):
    ni, no, _ = pm.OPS[op]
    n = len(rows)
    a_in = (ctypes.c_uint32 * (n * ni))(*[w for r in rows for w in r])
    a_out = (ctypes.c_uint32 * (n * no))(*([0xa5a5a5a5] * (n * no)))
    act = (ctypes.c_uint8 * n)(*([1] * n))
    assert emu.emu_ecp(op.encode(), n, act, a_in, a_out, tabs, n_tabs) == 0, op
    return [list(a_out[i * no:(i + 1) * no]) for i in range(n)]


@pytest.fixture(scope="module")
def steered(emu):
    """(rows, their key tables followed by G's): table i is row i's key's"""
    rows = lm.all_rows()
    keys = [model.key_bytes(r.key) for r in rows] + [model.key_bytes(model.G)]
    kt = run(emu, "key_table", [[len(k)] + pm.bytes_words(k, 17) for k in keys])
    assert all(t[0] == 0 for t in kt)
    return rows, (ctypes.c_uint32 * (240 * len(keys)))(*[w for t in kt for w in t[1:]])


def test_every_target_is_steered_and_traced():
    targets, long_inf, ends = lm.rows()
    assert len(lm.TARGETS) == 256 and [r.target for r in targets] == lm.TARGETS
    seen = set()
    for r in targets + long_inf + ends:
        assert r.target in r.events, r.name
        r.judge()
        seen.update(e for e in r.events if e[2] != "inf" and e[0] != lm.START)
        for i, e in enumerate(r.events):
            if e[2] == "cancel":
                if i + 1 < len(r.events):
                    assert r.events[i + 1][2] == "inf", r.name     # the next non-zero digit re-enters
                else:
                    assert r.want is None, r.name                  # the ladder's last addition: an infinite sum
            if e[2] == "inf" and i:
                assert r.events[i - 1][2] == "cancel", r.name
        assert r.events[0][2] == "inf"                             # the first non-zero digit meets the start
        assert r.counts == lm.counts(r.events) and sum(r.counts) == len(r.events)
    missing = [t for t in lm.TARGETS if t not in seen]
    assert not missing, missing
    # a cancel at Q that the same round's G addition re-enters: every Q-cancel row with a non-zero G digit
    both = 0
    for r in targets + ends:
        k, addend, kind = r.target
        if addend == "Q" and kind == "cancel" and lm.recode(r.u1)[k + 1] != 0:
            assert r.events[r.events.index(r.target) + 1] == (k, "G", "inf"), r.name
            both += 1
    assert both >= 32
    assert sorted({r.inf_doublings for r in long_inf}) == [8, 16]
    assert sum(1 for r in targets + long_inf + ends if r.want is None) >= 3


def test_model_trace_on_ordinary_scalars():
    """a key nobody steered: one event, the start's, and the sum the model's"""
    import random
    rng = random.Random(5)
    for _ in range(8):
        d, u1, u2 = (rng.randrange(1, N) for _ in range(3))
        events, sigma = lm.trace(u1, u2, d)
        assert [e[2] for e in events] == ["inf"] and sigma == (u1 + u2 * d) % N
    # key G, u1 = u2: the first addition doubles, as the crafted rows of ecdsa_edges.json do
    assert lm.trace(5, 5, 1)[0] == [(63, "Q", "inf"), (63, "G", "dbl")]
    assert lm.trace(5, 5, N - 1)[0] == [(63, "Q", "inf"), (63, "G", "cancel")]


def test_double_mul_sums_and_branch_counts(emu, steered):
    rows, tabs = steered
    g = len(rows)
    col_max(emu, reset=True)
    madd_counts(emu)
    for i, r in enumerate(rows):
        got = run(emu, "double_mul", [[i, g] + pm.words(r.u1) + pm.words(r.u2)], tabs, g + 1)
        assert madd_counts(emu) == r.counts, (r.name, r.events)
        pm.check_mul([(r.name,)], got, [r.want])
    assert 0 < col_max(emu) < emu.emu_ecdsa_col_bound()


def test_verify_scalars_accepts_the_signature_and_rejects_its_neighbour(emu, steered):
    rows, tabs = steered
    g = len(rows)
    col_max(emu, reset=True)
    madd_counts(emu)
    for i, r in enumerate(rows):
        got = run(emu, "verify_scalars", [[i, g] + pm.words(r.e) + pm.words(r.r) + pm.words(r.s)], tabs, g + 1)
        assert madd_counts(emu) == r.counts, r.name
        assert got[0][0] == r.valid, r.name
    bad = run(emu, "verify_scalars", [[i, g] + pm.words(r.e) + pm.words(r.r) + pm.words(r.s_bad) for i, r in enumerate(rows)],
              tabs, g + 1)
    assert [b[0] for b in bad] == [0] * g
    assert sum(r.valid for r in rows) >= g - 8 and 0 < col_max(emu) < emu.emu_ecdsa_col_bound()


def be32(v):
    return v.to_bytes(32, "big")


def test_record_path_with_the_digest_given(emu, steered):
    """emu_ecdsa_record under the fixed-length SHA-256 algorithm, the digest the 32 big-endian bytes of e: the
    key's table is built inside (its first addition doubles: one more doubling than the ladder's)"""
    rows, _ = steered
    g = model.key_bytes(model.G)
    emu.emu_ecdsa_record(0, g, 65, be32(1) + be32(1), 64, bytes(32))       # (G's table exists from here on)
    col_max(emu, reset=True)
    madd_counts(emu)
    for r in rows:
        key = model.key_bytes(r.key)
        got = emu.emu_ecdsa_record(0, key, 65, be32(r.r) + be32(r.s), 64, be32(r.e))
        c = r.counts
        assert madd_counts(emu) == (c[0], c[1] + 1, c[2]), r.name
        assert got == (model.OK if r.valid else model.MISMATCH), r.name
        assert emu.emu_ecdsa_record(0, key, 65, be32(r.r) + be32(r.s_bad), 64, be32(r.e)) == model.MISMATCH, r.name
        madd_counts(emu)
    assert 0 < col_max(emu) < emu.emu_ecdsa_col_bound()


def test_under_sanitizers(tmp_path):
    """The steered rows as records of the stand-alone program under the address and undefined-behaviour
    sanitizers; its branch counts over the whole file against the traces.  Only the record path
    (emu_ecdsa_record: key_table, then verify_scalars and double_mul inside it, each row under its own key) runs
    under the sanitizers; the program's primitive rows know G's table alone and are left empty here."""
    rows = lm.all_rows()
    recs, ops, outp = str(tmp_path / "records.txt"), str(tmp_path / "ops.txt"), str(tmp_path / "ops_out.txt")
    want = [0, 1, 0]                                                        # G's table, built at the first record
    n = 0
    with open(recs, "w") as f:
        for r in rows:
            key = model.key_bytes(r.key).hex()
            for s, code in ((r.s, model.OK if r.valid else model.MISMATCH), (r.s_bad, model.MISMATCH)):
                f.write("0 %s %s %s %d\n" % (key, (be32(r.r) + be32(s)).hex(), be32(r.e).hex(), code))
                w = lm.inv(s)
                c = lm.counts(lm.trace(r.e * w % N, r.r * w % N, r.d)[0])
                want = [want[0] + c[0], want[1] + c[1] + 1, want[2] + c[2]]
                n += 1
    open(ops, "w").close()
    p = subprocess.run([san_exe(), recs, ops, outp], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **SAN_ENV))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "%d records, 0 wrong" % n in p.stdout
    assert "madd returns: %d infinite, %d doubling, %d cancel" % tuple(want) in p.stdout, p.stdout[-500:]


def test_grinded_records_take_the_branch_their_name_promises(emu):
    rows = LADDER["rows"]
    assert "model" in LADDER["judge"] and len(rows) <= 120
    have = {(r["alg"], r["round"], r["addend"], r["kind"]) for r in rows if r["code"] == model.OK}
    assert have >= {(alg, k, a, kind) for alg in range(3) for k in (0, 1) for a in lm.ADDENDS for kind in lm.KINDS}
    assert any(t[1] == 2 and t[2] == "Q" for t in have)
    emu.emu_ecdsa_record(0, model.key_bytes(model.G), 65, be32(1) + be32(1), 64, bytes(32))
    madd_counts(emu)
    for r in rows:
        alg, d, msg, sig = r["alg"], int(r["d"], 16), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"])
        key = model.key_bytes(model.mul(d, model.G))
        assert key.hex() == r["key"] and model.verify_code(alg, key, msg, sig) == r["code"], r["name"]
        rr, ss = (int.from_bytes(b, "big") for b in model.split_sig(alg, sig))
        e, w = model.digest_scalar(alg, msg), lm.inv(ss)
        events, _ = lm.trace(e * w % N, rr * w % N, d)
        if r["code"] == model.OK:              # (a twin may take it too: at round 0 its digits match 1 time in 64)
            assert (r["round"], r["addend"], r["kind"]) in events, r["name"]
        assert emu.emu_ecdsa_record(alg, key, 65, sig, len(sig), digest_of(alg, msg)) == r["code"], r["name"]
        c = lm.counts(events)
        assert madd_counts(emu) == (c[0], c[1] + 1, c[2]), r["name"]
    twins = [r for r in rows if r["code"] == model.MISMATCH]
    assert len(twins) * 2 == len(rows) and all(t["name"].endswith("one more message byte") for t in twins)


def test_equal_halves_rows_of_the_edge_fixture_do_not_double():
    """ecdsa_edges.json's "u1 G = u2 Q" rows (key (e / r) G): the interleaved ladder's accumulator never meets an
    addend, so they take no doubling; what they exercise is the final r Z^2 = X test on 2 u1 G.  The "-u2 Q" rows
    (key (-e / r) G) do cancel, once, at the ladder's last addition."""
    seen = 0
    for name, alg, key, msg, sig, code in ROWS:
        if not name.startswith(("u1 G = u2 Q", "u1 G = -u2 Q")):
            continue
        rr, ss = (int.from_bytes(b, "big") for b in model.split_sig(alg, sig))
        e, w = model.digest_scalar(alg, msg), lm.inv(ss)
        d = (-e if "-u2" in name else e) * lm.inv(rr) % N
        assert model.key_bytes(lm.mul_g(d)) == key, name
        events, sigma = lm.trace(e * w % N, rr * w % N, d)
        if "-u2" in name:
            assert lm.counts(events) == (1, 0, 1) and events[-1][2] == "cancel" and sigma == 0, name
        else:
            assert lm.counts(events) == (1, 0, 0) and sigma == 2 * e * w % N, name
        seen += 1
    assert seen == 6
