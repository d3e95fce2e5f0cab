"""GPU: the one-lane-per-record BLS primitives (cess_amd/csrc/bls/field.hpp Fp
and Fp2, curve.hpp, h2c.hpp, the line steps of pairing.hpp), each alone,
against integer arithmetic.

k_decode_*, k_hash, k_prepare, k_norm_keys, k_sign and k_rlc are otherwise
checked end to end only, on records whose intermediates are random residues.
Here each primitive runs alone, through the test-only library
cess_amd/lib/libcess_lane_probe.so (tests/probe/lane_probe.hip: the shipped
headers, one kernel per operation, the production block and launch bounds,
each part built with the flags of the unit that ships its code), on the
operand tables of tests/lane_probe_model.py, and every lane's result is held
to what the CPU test (tests/test_lane_primitives.py) asserts of the host
build.  What only the device build runs is here alone: inv() leaving its loop
on a wave-wide ballot (a first wave that mixes both zeros, the 26- and the
>= 27-iteration class, a second wave of the 26 class only), pow_fixed's
readfirstlane table selection under a divergent choice of exponent,
hash_to_g1_parked with its LDS park indexed by threadIdx, g2_prepare_emit with
the key re-read from LDS, the interleaved carry chains and asm fences of
field.hpp under the device compiler.

Placement: every operation runs with 1, 65 and 321 lanes (one lane; a wave and
a lane; a block, a wave and a lane), the cheap Fp / Fp2 operations also on
their whole table, and each size once more with every lane i mod 4 in {1, 2}
switched off, whose results must come back as the poison they were filled
with.  Neighbouring lanes hold different rows; every live row is compared.
"""
import ctypes
import os

import numpy as np
import pytest

import lane_probe_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cess_amd", "lib", "libcess_lane_probe.so")
MAKE_HINT = "make -C cess_amd/csrc ../lib/libcess_lane_probe.so"

_lib = []


def probe():
    if not _lib:
        if not os.path.exists(LIB):
            pytest.fail("%s is missing: build it with `%s` (or `make -C cess_amd/csrc`)" % (LIB, MAKE_HINT))
        lib = ctypes.CDLL(LIB)
        lib.lane_probe_ops.restype = ctypes.c_char_p
        lib.lane_probe_error.restype = ctypes.c_char_p
        _lib.append(lib)
    return _lib[0]


def call(name, n, act, inp, out):
    lib = probe()
    rc = getattr(lib, "lp_" + name)(ctypes.c_uint32(n), act, inp, out)
    if rc != 0:     # a HIP error (a fault included): nothing more is launched on this device
        pytest.exit("lp_%s: HIP status %d (%s)" % (name, rc, lib.lane_probe_error(rc).decode()), returncode=3)
    return rc


def test_probe_covers_the_model():
    """the library's entry points and the model's operations are the same set, with the same lane layouts"""
    lib = probe()
    listed = {}
    for item in lib.lane_probe_ops().decode().strip(",").split(","):
        f = item.split(":")
        listed[f[0]] = tuple(int(v) for v in f[1:])
    ops = pm.ops()
    assert listed.pop("soa_layout") == (pm.SOA_IN, pm.SOA_OUT) and hasattr(lib, "lp_soa_layout")
    assert sorted(listed) == sorted(pm.OP_NAMES) == sorted(o.name for o in ops)
    assert lib.lane_probe_threads() == 256
    for o in ops:
        assert hasattr(lib, "lp_" + o.name), o.name
        assert listed[o.name] == (o.n_in, o.n_out), o.name


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
@pytest.mark.parametrize("name", pm.OP_NAMES)
def test_lane_primitive(name, half):
    """one primitive at 1, 65 and 321 lanes (the cheap ones also on their whole
    table), all lanes live or lanes i mod 4 in {1, 2} switched off"""
    op = pm.get_op(name)
    assert len(op.rows) >= 321 and all(op.rows[i] != op.rows[i + 1] for i in range(320))
    for n in pm.LANE_COUNTS + ((len(op.rows),) if op.cheap and len(op.rows) > 321 else ()):
        active = pm.active_mask(n, half)
        _, out = pm.run(call, op, n, active)
        pm.check_lanes(op, out, active)


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
def test_soa_layout(half):
    """soa.hpp's stores and loads (st_fp / ld_fp, st_fp2 / ld_fp2, st_coeff4,
    st_coeff4_one, ld_coeff4, ld_coeff_uniform) with a stride larger than the
    lane count: rows land where the comments say, and nothing is written
    outside the live columns"""
    lib = probe()

    def call_soa(n, stride, act, inp, slots, tab, out):
        rc = lib.lp_soa_layout(ctypes.c_uint32(n), ctypes.c_uint32(stride), act, inp, slots, tab, out)
        if rc != 0:
            pytest.exit("lp_soa_layout: HIP status %d (%s)" % (rc, lib.lane_probe_error(rc).decode()), returncode=3)
        return rc
    for n in pm.LANE_COUNTS:
        active = pm.active_mask(n, half)
        _, rows, tab, stride, out, slots = pm.soa_run(call_soa, n, active)
        pm.soa_check(rows, tab, stride, active, out, slots)


def test_inversion_waves_leave_apart():
    """fp_inv's table as the model places it: the first wave holds both zeros
    and both iteration classes, the second the lower class alone"""
    rows, classes = pm.inv_rows()
    pm.assert_inv_placement(rows, classes)
    op = pm.get_op("fp_inv")
    assert op.rows[:128] == [pm.words(v) for v in rows[:128]]
    for n in (64, 128):
        _, out = pm.run(call, op, n, [1] * n)
        pm.check_lanes(op, out, [1] * n)


def test_parked_hash_equals_the_register_form():
    """hash_to_g1_parked (k_hash's form: LDS park indexed by threadIdx, the
    SELECT expand) and hash_to_g1 give the same limbs on every message row,
    at 321 lanes, so that threadIdx differs from the lane index and blockIdx > 0"""
    a, b = pm.get_op("hash_to_g1"), pm.get_op("hash_to_g1_parked")
    assert a.rows == b.rows
    n = 321
    for half in (False, True):
        active = pm.active_mask(n, half)
        _, out_a = pm.run(call, a, n, active)
        _, out_b = pm.run(call, b, n, active)
        assert np.array_equal(out_a, out_b)
        pm.check_lanes(b, out_b, active)
