"""CPU: the Ed25519 primitives of cess_amd/csrc/ed25519.hpp, each alone, in the
host build (tests/hostemu/ed25519_emu.cpp, emu_edp: the lane functions of
tests/probe/ed25519_probe.hip in a loop) against the integer references of
tests/ed25519_probe_model.py, on the tables the GPU probe takes
(tests/test_gpu_ed25519_primitives.py): limbs at the input and tight maxima,
carry ripples, non-canonical encodings of k p + d, scalars at multiples of L
and with every count of final subtractions, digit strings of all -8, 7 and 0,
the group formulas at the corners of the tight bound and on torsion points,
every digit of ge_pre_digit, key tables of crafted keys, and the verify loop
with chosen S and h.

The same tables go through the stand-alone sanitizer program (address and
undefined behaviour; its own main, a child process).  After the group and
verify rows the 128-bit shadow of every column sum stays below the header's
2^62.4.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ed25519_probe_model as pm
from test_ed25519 import SAN_ENV, _emu, san_exe
from test_ed25519_crafted import load_crafted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = os.path.join(ROOT, "tests", "probe", "ed25519_probe.hip")


@pytest.fixture(scope="module")
def fixture_keys():
    return load_crafted()["keys"]


@pytest.fixture(scope="module")
def call():
    emu = _emu()
    vp = ctypes.c_void_p
    emu.emu_edp.argtypes = [ctypes.c_char_p, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32]
    emu.emu_edp_ops.restype = ctypes.c_char_p

    def call(name, n, act, inp, out, tabs, n_tabs):
        return emu.emu_edp(name.encode(), n, act, inp, out, tabs, n_tabs)
    call.emu = emu
    return call


def listed_in_source():
    """{name: (n_in, n_out, n_idx, threads)} of the probe's EDP_OPS list"""
    text = open(PROBE_SRC).read()
    body = text[text.index("#define EDP_OPS(X)"):text.index("namespace edp")]
    return {m.group(1): tuple(int(m.group(k)) for k in range(2, 6))
            for m in re.finditer(r"X\((\w+), (\d+), (\d+), (\d+), (\d+)\)", body)}


def test_probe_lists_the_models_operations(call, fixture_keys):
    listed = listed_in_source()
    ops = pm.ops(fixture_keys)
    assert [o.name for o in ops] == pm.OP_NAMES and sorted(listed) == sorted(pm.OP_NAMES)
    for o in ops:
        assert listed[o.name] == (o.n_in, o.n_out, o.n_idx, o.threads), o.name
        assert len(o.rows) >= pm.LANE_COUNTS[-1], (o.name, len(o.rows))
        assert all(o.rows[i] != o.rows[i + 1] for i in range(len(o.rows) - 1)), o.name
    assert max(len(o.rows) for o in ops if o.name in ("verify_equation", "key_table")) <= 257
    built = {it.split(":")[0]: tuple(int(v) for v in it.split(":")[1:])
             for it in call.emu.emu_edp_ops().decode().strip(",").split(",")}
    assert built == listed
    text = open(PROBE_SRC).read()
    assert "__launch_bounds__(64, 1)" in text and "EDP_LB_256 CESS_LB" in text
    assert [t for n, (_, _, _, t) in listed.items() if n != "key_table"] == [256] * (len(listed) - 1)
    assert listed["key_table"][3] == 64


@pytest.mark.parametrize("name", pm.OP_NAMES)
def test_primitive_on_host(call, fixture_keys, name):
    op = pm.get_op(name, fixture_keys)
    n = len(op.rows)
    for half in (False, True):
        active = pm.active_mask(n, half)
        status, out = pm.run(call, op, n, active)
        assert status == 0
        pm.check_lanes(op, out, active)
    # arguments the lanes' bounds forbid are refused
    if op.n_idx:
        assert pm.run(call, op, n, [1] * n, tabs=op.tabs[:1])[0] == 1


def test_tables_from_key_table_on_host(call, fixture_keys):
    """ge_pre_digit and verify_equation on the tables key_table itself wrote"""
    for name in ("ge_pre_digit", "verify_equation"):
        op = pm.get_op(name, fixture_keys)
        kt = pm.Op("key_table", 9, 1 + pm.TABLE_WORDS, threads=64)
        for k in op.keys:
            kt.add([32] + pm.words_of(int.from_bytes(k, "little")), None)
        status, out = pm.run(call, kt, len(op.keys), [1] * len(op.keys))
        assert status == 0 and [int(r[0]) for r in out] == [0] * len(op.keys)
        n = len(op.rows)
        status, res = pm.run(call, op, n, [1] * n, tabs=pm.tables_from(out))
        assert status == 0
        pm.check_lanes(op, res, [1] * n)


def test_column_maximum(call, fixture_keys):
    """the 128-bit shadow of every column sum over all group, table and verify rows"""
    hi, lo = ctypes.c_uint64(), ctypes.c_uint64()
    call.emu.emu_ed_col_max(hi, lo, 1)
    for name in ("ge_dbl", "ge_madd", "ge_decode", "key_table", "ge_pre_digit", "verify_equation"):
        op = pm.get_op(name, fixture_keys)
        assert pm.run(call, op, len(op.rows), [1] * len(op.rows))[0] == 0
    call.emu.emu_ed_col_max(hi, lo, 0)
    print("largest column sum: 2^%.2f" % math.log2(lo.value))
    assert hi.value == 0 and 2**60 < lo.value < pm.COL_BOUND


def test_primitives_under_sanitizers(tmp_path, fixture_keys):
    exe = san_exe()
    ops = pm.ops(fixture_keys)
    src, dst = str(tmp_path / "ops.txt"), str(tmp_path / "results.txt")
    with open(src, "w") as f:
        for op in ops:
            tabs = op.tabs or []
            f.write("%s %d %d %d %d\n" % (op.name, len(op.rows), op.n_in, op.n_out, len(tabs)))
            f.write("\n".join(" ".join(str(w) for w in r) for r in op.rows) + "\n")
            for t in tabs:
                f.write(" ".join(str(w) for w in t) + "\n")
    r = subprocess.run([exe, "ops", src, dst], capture_output=True, text=True, timeout=900, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d operations" % len(ops) in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    words = np.loadtxt(dst, dtype=np.uint64).astype(np.uint32)
    at = 0
    for op in ops:
        n = len(op.rows)
        out = words[at:at + n * op.n_out].reshape(n, op.n_out)
        at += n * op.n_out
        pm.check_lanes(op, out, [1] * n)
    assert at == len(words)
