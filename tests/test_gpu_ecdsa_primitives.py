"""The ECDSA P-256 primitives on the GPU, one kernel per primitive
(libcess_ecdsa_probe.so from tests/probe/ecdsa_probe.hip), on the operand tables
of tests/ecdsa_probe_model.py against Python integers, with lane counts 1, 63,
64, 65 and 257, and the verify loop on integers (e = 0 and e = n - 1)."""
import ctypes
import os

import pytest

import ecdsa_probe_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = pm.tables()
POISON = 0xa5a5a5a5


@pytest.fixture(scope="module")
def probe():
    lib = ctypes.CDLL(os.path.join(ROOT, "cess_amd", "lib", "libcess_ecdsa_probe.so"))
    lib.ecdsa_probe_ops.restype = ctypes.c_char_p
    lib.ecdsa_probe_error.restype = ctypes.c_char_p
    ops = {t.split(":")[0]: tuple(int(x) for x in t.split(":")[1:4]) for t in lib.ecdsa_probe_ops().decode().split(",") if t}
    assert ops == pm.OPS
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    for op in ops:
        getattr(lib, "ecp_" + op).argtypes = [ctypes.c_uint32, u8p, u32p, u32p, u32p, ctypes.c_uint32]
    return lib


def run(lib, op, rows, lanes, tabs=None, n_tabs=0):
    """`lanes` lanes cycling the rows; every third lane past the first inactive.  Returns the active lanes' (row, out)."""
    ni, no, _ = pm.OPS[op]
    picks = [rows[i % len(rows)] for i in range(lanes)]
    active = [0 if (i % 3 == 2 and lanes > 1) else 1 for i in range(lanes)]
    a_in = (ctypes.c_uint32 * (lanes * ni))(*[w for r in picks for w in r])
    a_out = (ctypes.c_uint32 * (lanes * no))(*([POISON] * (lanes * no)))
    act = (ctypes.c_uint8 * lanes)(*active)
    st = getattr(lib, "ecp_" + op)(lanes, act, a_in, a_out, tabs, n_tabs)
    assert st == 0, lib.ecdsa_probe_error(st)
    outs = [list(a_out[i * no:(i + 1) * no]) for i in range(lanes)]
    for i in range(lanes):
        if not active[i]:
            assert outs[i] == [POISON] * no
    return [picks[i] for i in range(lanes) if active[i]], [outs[i] for i in range(lanes) if active[i]]


def run_all(lib, op, rows, tabs=None, n_tabs=0):
    """one active lane per row, in order"""
    ni, no, _ = pm.OPS[op]
    n = len(rows)
    a_in = (ctypes.c_uint32 * (n * ni))(*[w for r in rows for w in r])
    a_out = (ctypes.c_uint32 * (n * no))(*([POISON] * (n * no)))
    act = (ctypes.c_uint8 * n)(*([1] * n))
    st = getattr(lib, "ecp_" + op)(n, act, a_in, a_out, tabs, n_tabs)
    assert st == 0, lib.ecdsa_probe_error(st)
    return rows, [list(a_out[i * no:(i + 1) * no]) for i in range(n)]


@pytest.mark.parametrize("op", sorted(TABLES))
def test_primitive_on_its_table(probe, op):
    rows = TABLES[op]
    r, o = run(probe, op, rows, max(len(rows) * 3 // 2 + 1, 65))
    pm.check(op, r, o)


@pytest.mark.parametrize("lanes", [1, 63, 64, 65, 257])
def test_lane_counts(probe, lanes):
    for op in ("fe_mul", "fe_sub", "sc_mul", "sc_digits", "pt_madd", "parse_sig"):
        r, o = run(probe, op, TABLES[op], lanes)
        pm.check(op, r, o)


@pytest.mark.parametrize("lanes", [1, 65])
def test_verify_loop_on_integers(probe, lanes):
    key, rows, want = pm.verify_rows()
    _, kt = run(probe, "key_table", [[len(key)] + pm.bytes_words(key, 17), [65] + pm.bytes_words(pm.m.key_bytes(pm.m.G), 17)], 2)
    assert kt[0][0] == 0 and kt[1][0] == 0
    tabs = (ctypes.c_uint32 * 480)(*(kt[0][1:] + kt[1][1:]))
    table = [[0, 1] + pm.words(e) + pm.words(r) + pm.words(s) for e, r, s in rows]
    r, o = run(probe, "verify_scalars", table, lanes, tabs, 2)
    for row, out in zip(r, o):
        assert out[0] == want[table.index(row)]


def test_ladder_on_ring_point_mul_rows_and_corner_scalars(probe):
    keys, rows, want = pm.mul_rows()
    keys = keys + [pm.m.key_bytes(pm.m.G)]
    picks, kt = run_all(probe, "key_table", [[len(k)] + pm.bytes_words(k, 17) for k in keys])
    assert all(t[0] == 0 for t in kt)
    tabs = (ctypes.c_uint32 * (240 * len(keys)))(*[w for t in kt for w in t[1:]])
    table = [[q, len(keys) - 1] + pm.words(u1) + pm.words(u2) for q, u1, u2 in rows]
    _, got = run_all(probe, "double_mul", table, tabs, len(keys))
    pm.check_mul(rows, got, want)
