"""The ladder of cess_amd/csrc/p256.hpp on the GPU, steered into the special
returns of pt_madd (tests/ecdsa_ladder_model.py: a doubling or a cancel at every
round and either addition, infinite accumulators doubled through whole rounds,
the end cases), through the probe's double_mul and verify_scalars kernels
(libcess_ecdsa_probe.so).  The host tests (tests/test_ecdsa_ladder.py) hold the
same rows to the model and to the branch counts; here the question is the
device code's: a branch that diverges inside the round loop with pt_dbl called
from it.  One lane per row, every lane of a wave on one row, and waves that mix
steered rows of different rounds with ordinary rows and inactive lanes.  Affine
sums as integers, verdicts as 0 / 1: exact."""
import ctypes

import pytest

import ecdsa_ladder_model as lm
import ecdsa_probe_model as pm
from test_gpu_ecdsa_primitives import POISON, probe, run_all  # noqa: F401  (probe: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(probe):  # noqa: F811
    """the steered rows, the ordinary ones of mul_rows(), and one array of key tables: the steered rows' keys
    (table i is row i's), the ordinary rows' keys, then G"""
    rows = lm.all_rows()
    for r in rows:
        r.judge_points()              # the expected sums are ecdsa_model.mul's, whichever way the rows computed them
    okeys, orows, owant = pm.mul_rows()
    keys = [pm.m.key_bytes(r.key) for r in rows] + okeys + [pm.m.key_bytes(pm.m.G)]
    _, kt = run_all(probe, "key_table", [[len(k)] + pm.bytes_words(k, 17) for k in keys])
    assert all(t[0] == 0 for t in kt)
    tabs = (ctypes.c_uint32 * (240 * len(keys)))(*[w for t in kt for w in t[1:]])
    g = len(keys) - 1
    steered = [([i, g] + pm.words(r.u1) + pm.words(r.u2), r.want, r.name) for i, r in enumerate(rows)]
    ordinary = [([len(rows) + q, g] + pm.words(u1) + pm.words(u2), w, "ordinary %d" % j)
                for j, ((q, u1, u2), w) in enumerate(zip(orows, owant))]
    return rows, steered, ordinary, tabs, len(keys)


def launch(lib, op, table, active, tabs, n_tabs):
    """one launch, lane i on table[i]; the results of the active lanes by lane, None for the inactive ones, whose
    words must come back as they went in"""
    ni, no, _ = pm.OPS[op]
    n = len(table)
    a_in = (ctypes.c_uint32 * (n * ni))(*[w for r in table for w in r])
    a_out = (ctypes.c_uint32 * (n * no))(*([POISON] * (n * no)))
    act = (ctypes.c_uint8 * n)(*active)
    st = getattr(lib, "ecp_" + op)(n, act, a_in, a_out, tabs, n_tabs)
    assert st == 0, lib.ecdsa_probe_error(st)
    outs = [list(a_out[i * no:(i + 1) * no]) for i in range(n)]
    for i in range(n):
        if not active[i]:
            assert outs[i] == [POISON] * no, i
    return [o if a else None for o, a in zip(outs, active)]


def verify_in(i, g, r, s):
    return [i, g] + pm.words(r.e) + pm.words(r.r) + pm.words(s)


def test_every_steered_row_one_lane_each(probe, world):  # noqa: F811
    rows, steered, _, tabs, n_tabs = world
    assert len(steered) >= 256 and {r.target for r in rows} == set(lm.TARGETS)
    outs = launch(probe, "double_mul", [s[0] for s in steered], [1] * len(steered), tabs, n_tabs)
    pm.check_mul([(s[2],) for s in steered], outs, [s[1] for s in steered])
    g = n_tabs - 1
    good = launch(probe, "verify_scalars", [verify_in(i, g, r, r.s) for i, r in enumerate(rows)], [1] * len(rows), tabs, n_tabs)
    assert [o[0] for o in good] == [r.valid for r in rows], [r.name for r, o in zip(rows, good) if o[0] != r.valid]
    bad = launch(probe, "verify_scalars", [verify_in(i, g, r, r.s_bad) for i, r in enumerate(rows)], [1] * len(rows), tabs, n_tabs)
    assert [o[0] for o in bad] == [0] * len(rows), [r.name for r, o in zip(rows, bad) if o[0]]


def uniform_rows():
    targets, long_inf, _ = lm.rows()
    by = {r.target: r for r in targets}
    return [by[(17, "Q", "dbl")], by[(40, "G", "cancel")], next(r for r in long_inf if r.inf_doublings == 16)]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["dbl", "cancel", "long-infinity"])
def test_whole_wave_on_one_steered_row(probe, world, which):  # noqa: F811
    """64 lanes, all active, all on the same row: the special return is taken by the whole wave at once"""
    rows, steered, _, tabs, n_tabs = world
    r = uniform_rows()[which]
    i = rows.index(r)
    outs = launch(probe, "double_mul", [steered[i][0]] * 64, [1] * 64, tabs, n_tabs)
    pm.check_mul([(r.name,)] * 64, outs, [r.want] * 64)
    got = launch(probe, "verify_scalars", [verify_in(i, n_tabs - 1, r, r.s)] * 64, [1] * 64, tabs, n_tabs)
    assert [o[0] for o in got] == [r.valid] * 64 and r.valid == 1


@pytest.mark.parametrize("lanes", [65, 257])
def test_waves_that_mix_steered_ordinary_and_inactive_lanes(probe, world, lanes):  # noqa: F811
    """lane i: a steered row (i = 0 mod 3; consecutive ones 37 rows apart, so a wave holds doublings, cancels and
    re-entries at rounds all over the ladder), an ordinary row (1 mod 3) or inactive (2 mod 3)"""
    rows, steered, ordinary, tabs, n_tabs = world
    picks, active = [], []
    for i in range(lanes):
        picks.append(steered[(i // 3 * 37) % len(steered)] if i % 3 == 0 else ordinary[(i // 3) % len(ordinary)])
        active.append(0 if i % 3 == 2 else 1)
    wave0 = [p[2] for p, a in zip(picks[:64], active[:64]) if a and not p[2].startswith("ordinary")]
    assert len({n.split()[1] for n in wave0}) >= 16 and any("cancel" in n for n in wave0) and any("dbl" in n for n in wave0)
    outs = launch(probe, "double_mul", [p[0] for p in picks], active, tabs, n_tabs)
    live = [i for i in range(lanes) if active[i]]
    pm.check_mul([(picks[i][2],) for i in live], [outs[i] for i in live], [picks[i][1] for i in live])
    # the same lanes through the verify loop: the steered lanes' signatures, the inactive lanes as they were
    g = n_tabs - 1
    vpicks = [(i // 3 * 37) % len(rows) for i in range(lanes)]
    vact = [1 if i % 3 == 0 else 0 for i in range(lanes)]
    got = launch(probe, "verify_scalars", [verify_in(j, g, rows[j], rows[j].s) for j in vpicks], vact, tabs, n_tabs)
    assert [got[i][0] for i in range(lanes) if vact[i]] == [rows[vpicks[i]].valid for i in range(lanes) if vact[i]]
