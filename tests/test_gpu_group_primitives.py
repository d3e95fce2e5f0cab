"""GPU: the lane-group layer (cess_amd/csrc/bls/group.hpp, run by k_group and
k_group_fe of k_group.hip) against integer arithmetic: the half-products
grp_mul_comp and grp_sqr_comp alone, one round of a lane-group program on a
caller-built register file, and the two shipped kernels on caller-built inputs.

k_group serves every per-signature batch of up to 5,120 records and k_group_fe
the final exponentiation of every RLC check; both are otherwise checked end to
end only, on golden records whose intermediates are random residues.  Here they
run through the test-only library cess_amd/lib/libcess_group_probe.so
(tests/probe/group_probe.hip: k_group.hip, bls/group.hpp and both program
headers included unchanged, built with k_group's flags) on the tables of
tests/group_probe_model.py -- operands at the edges of the lazy-reduction
contract (slots near 2p, add_nr sums near 4p, digits of 0xfffffff, both
representations x and x + p), every flag byte and LIN shape of the two
programs and the unused ones, rounds of 1, 31 and 32 operations, a destination
that the other operations of its round read -- and every result is held to
exactly what the CPU test (tests/test_group_primitives.py) asserts of the host
build: the model's residue, below 2p, every unwritten word bit-identical.

The probe's `round` entry runs group_rounds of k_group.hip, the one loop
function that k_group and k_group_fe call, on a program of one round; the
kernels' own programs run through the whole-kernel entries `group_fe` and
`group` below.

What only the device runs is here alone: the store into the LDS register file
with no barrier between a round's reads and its writes (wave lockstep), under
the device compiler and the divergent flag and term-count branches of
group_eval_comp; Regs' uint4 rows; the kernels' loads, verdicts and Gt bytes.
"""
import ctypes
import os

import numpy as np
import pytest

import group_probe_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cess_amd", "lib", "libcess_group_probe.so")
MAKE_HINT = "make -C cess_amd/csrc ../lib/libcess_group_probe.so"

_lib = []


def probe():
    if not _lib:
        if not os.path.exists(LIB):
            pytest.fail("%s is missing: build it with `%s` (or `make -C cess_amd/csrc`)" % (LIB, MAKE_HINT))
        lib = ctypes.CDLL(LIB)
        lib.group_probe_ops.restype = ctypes.c_char_p
        lib.group_probe_error.restype = ctypes.c_char_p
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        lib.gp_grp_mul_comp.argtypes = lib.gp_grp_sqr_comp.argtypes = [u32, vp, vp, vp]
        lib.gp_round.argtypes = [u32, u32, vp, vp, vp, vp]
        lib.gp_group_fe.argtypes = [u32, vp, vp, vp]
        lib.gp_group.argtypes = [u32, u32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int, vp, vp]
        _lib.append(lib)
    return _lib[0]


def _status(name, rc):
    if rc != 0:     # a HIP error (a fault included): nothing more is launched on this device
        pytest.exit("gp_%s: HIP status %d (%s)" % (name, rc, probe().group_probe_error(rc).decode()), returncode=3)
    return rc


def call_comp(name, lanes, act, inp, out):
    return _status(name, getattr(probe(), "gp_" + name)(lanes, act, inp, out))


def call_round(n, n_slots, act, heads, ents, img):
    return _status("round", probe().gp_round(n, n_slots, act, heads, ents, img))


def call_fe(m, fin, code, gt):
    return _status("group_fe", probe().gp_group_fe(m, fin, code, gt))


def call_group(*args):
    return _status("group", probe().gp_group(*args))


def test_probe_covers_the_model():
    """the library's entry points and the model's operations are the same set, with the same layouts"""
    lib = probe()
    listed = {it.split(":")[0]: tuple(int(v) for v in it.split(":")[1:]) for it in lib.group_probe_ops().decode().strip(",").split(",")}
    assert listed == pm.OPS
    assert all(hasattr(lib, "gp_" + name) for name in pm.OPS)
    assert lib.group_probe_threads() == 64 and lib.group_probe_slots() == pm.programs()["full"][3]


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
@pytest.mark.parametrize("name", ["grp_mul_comp", "grp_sqr_comp"])
def test_half_product(name, half):
    """2, 130 and 642 lanes (pairs of lanes: one pair; two waves and a pair; ten waves and a pair) and the whole
    table, all rows live or rows i mod 4 in {1, 2} switched off (their lanes stay poison): the named component of
    A B / R (A^2 / R) mod p, below 2p"""
    rows = pm.comp_table(name)[0]
    assert len(rows) >= 321 and all(rows[i] != rows[i + 1] for i in range(len(rows) - 1))
    for n in pm.PAIR_COUNTS + (len(rows),):
        active = pm.active_rows(n, half)
        _, out = pm.run_comp(call_comp, name, n, active)
        pm.check_comp(name, out, active)


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
def test_round(half):
    """every row of the round table, one wave per row: entry decoding, every flag byte (used and unused), the LIN
    term classes, INV, idle lanes, rounds of 1, 31 and 32 operations, a destination that the other 31 operations
    read (they see the old value).  Then the same rounds on their neighbours' images -- nothing survives in LDS
    between two launches -- one row alone, and a full-size image.  Unwritten slots and the poison past the image
    come back bit-identical."""
    cases = pm.round_cases()
    for table, n_slots in ((cases, pm.ROUND_SLOTS), (pm.rotate_images(cases), pm.ROUND_SLOTS), (cases[:1], pm.ROUND_SLOTS),
                           (pm.wide_cases(), pm.programs()["full"][3])):
        active = pm.active_rows(len(table), half)
        _, before, after = pm.run_round(call_round, table, active, n_slots)
        pm.check_round(table, active, before, after)


def test_round_refuses_what_its_bounds_forbid():
    """a slot index past the image is refused on the host, before anything is launched"""
    c = pm.round_cases()[0]
    bad = pm.Case(c.kind, c.ents[:c.cnt], c.image)
    bad.ents[0][0] = pm.ROUND_SLOTS
    status, before, after = pm.run_round(probe().gp_round, [bad], [1])
    assert status == 1 and np.array_equal(before, after)      # hipErrorInvalidValue


def test_group_fe():
    """the shipped k_group_fe on caller-built Fp12 values, 1, 2 and 65 values a launch (a different row in each
    neighbouring wave): Gt bytes and code from the oracle's final_exponentiation.  f = 0 is not a row: zero has no
    defined result and never reaches the kernel."""
    rows = pm.fe_rows()
    for m in pm.BLOCK_COUNTS:
        table = pm.pick(rows, m, shift=m)
        _, code, gt = pm.run_fe(call_fe, table)
        pm.check_fe(table, code, gt)


def test_group():
    """the shipped k_group on caller-built codes, flags and SoA affine arrays of stride n + 7, in 1, 2 and 65
    blocks: real records (Gt and code from the oracle), arbitrary field values with INF_PK set (Gt from
    gen_group.simulate), the same with INF_PK clear (code 4, no Gt bytes), and decode codes arriving in `code` or
    `code2` (the signature's first), with code_out its own array or aliasing `code`"""
    recs = pm.group_recs()
    for n, split, alias in ((1, False, False), (2, True, True), (65, True, False), (65, False, True)):
        table = pm.pick(recs, n, shift=n + split)
        _, out, gt = pm.run_group(call_group, table, split, alias)
        pm.check_group(table, split, out, gt)
