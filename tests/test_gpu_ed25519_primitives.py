"""GPU: the Ed25519 primitives of cess_amd/csrc/ed25519.hpp, each alone,
against integer arithmetic.

k_ed25519_keys and k_ed25519_verify are otherwise checked end to end only, on
records whose intermediates are uniform field elements and whose h is a hash
nobody can choose.  Here each primitive runs alone, through the test-only
library cess_amd/lib/libcess_ed25519_probe.so (tests/probe/ed25519_probe.hip:
the shipped header, one kernel per operation, the production blocks and launch
bounds, built with k_ed25519_verify's flags), on the operand tables of
tests/ed25519_probe_model.py, and every lane's result is held to what the CPU
test (tests/test_ed25519_primitives.py) asserts of the host build: the exact
value mod p and the stated limb bound of every field result, canonical bytes
and flags, x mod L, the digit strings, E, H, G, F and X, Y, Z, T of the group
formulas, every entry of ge_pre_digit read through the device's uint2 path,
key tables and statuses, and verify_equation with chosen S, h and R.

Placement: every operation runs on its whole table and with 1, 65 and 257
lanes (one lane; a wave and a lane; a block and a lane), and once more with
every lane i mod 4 in {1, 2} switched off, whose results must come back as the
poison they were filled with.  Neighbouring lanes hold different rows.  The
probe's kernels are compiled apart from the production kernels: this checks the
header's arithmetic under the device compiler at the edges, the end-to-end
tests keep checking those kernels' code generation."""
import ctypes
import os

import pytest

import ed25519_probe_model as pm
from test_ed25519_crafted import load_crafted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cess_amd", "lib", "libcess_ed25519_probe.so")
MAKE_HINT = "make -C cess_amd/csrc ../lib/libcess_ed25519_probe.so"

_lib = []


def probe():
    if not _lib:
        if not os.path.exists(LIB):
            pytest.fail("%s is missing: build it with `%s` (or `make -C cess_amd/csrc`)" % (LIB, MAKE_HINT))
        lib = ctypes.CDLL(LIB)
        lib.ed25519_probe_ops.restype = ctypes.c_char_p
        lib.ed25519_probe_error.restype = ctypes.c_char_p
        _lib.append(lib)
    return _lib[0]


def call(name, n, act, inp, out, tabs, n_tabs):
    lib = probe()
    fn = getattr(lib, "edp_" + name)
    rc = fn(ctypes.c_uint32(n), act, inp, out, tabs, ctypes.c_uint32(n_tabs))
    if rc != 0:     # a HIP error (a fault included): nothing more is launched on this device
        pytest.exit("edp_%s: HIP status %d (%s)" % (name, rc, lib.ed25519_probe_error(rc).decode()), returncode=3)
    return rc


@pytest.fixture(scope="module")
def fixture_keys():
    return load_crafted()["keys"]


def test_probe_covers_the_model(fixture_keys):
    """the library's entry points and the model's operations are the same set, with the same lane layouts"""
    lib = probe()
    listed = {}
    for item in lib.ed25519_probe_ops().decode().strip(",").split(","):
        f = item.split(":")
        listed[f[0]] = tuple(int(v) for v in f[1:])
    ops = pm.ops(fixture_keys)
    assert sorted(listed) == sorted(pm.OP_NAMES) == sorted(o.name for o in ops)
    for o in ops:
        assert hasattr(lib, "edp_" + o.name), o.name
        assert listed[o.name] == (o.n_in, o.n_out, o.n_idx, o.threads), o.name


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
@pytest.mark.parametrize("name", pm.OP_NAMES)
def test_ed25519_primitive(fixture_keys, name, half):
    """one primitive at 1, 65 and 257 lanes and on its whole table, all lanes
    live or lanes i mod 4 in {1, 2} switched off"""
    op = pm.get_op(name, fixture_keys)
    assert len(op.rows) >= 257 and all(op.rows[i] != op.rows[i + 1] for i in range(256))
    for n in pm.LANE_COUNTS + ((len(op.rows),) if len(op.rows) > 257 else ()):
        active = pm.active_mask(n, half)
        _, out = pm.run(call, op, n, active)
        pm.check_lanes(op, out, active)


@pytest.mark.parametrize("name", ["ge_pre_digit", "verify_equation"])
def test_tables_from_key_table(fixture_keys, name):
    """the same rows on the tables the probe's own key_table wrote on the device"""
    op = pm.get_op(name, fixture_keys)
    kt = pm.Op("key_table", 9, 1 + pm.TABLE_WORDS, threads=64)
    for k in op.keys:
        kt.add([32] + pm.words_of(int.from_bytes(k, "little")), None)
    _, out = pm.run(call, kt, len(op.keys), [1] * len(op.keys))
    assert [int(r[0]) for r in out] == [0] * len(op.keys)
    n = len(op.rows)
    _, res = pm.run(call, op, n, [1] * n, tabs=pm.tables_from(out))
    pm.check_lanes(op, res, [1] * n)
