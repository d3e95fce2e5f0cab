"""Every primitive of cess_amd/csrc/p256.hpp alone against Python integers, on
the host build (tests/hostemu/ecdsa_emu.cpp runs the lane functions of
tests/probe/ecdsa_probe.hip): the field at the stated digit maxima and at 0, 1,
q - 1 and k q + d encodings, the scalars likewise with the inverse, the digit
recoding on every pattern of the crafted rows, the group formulas on ring's
point rows and the special cases, the key tables of the crafted keys, the
signature parser on every format row, and the verify loop on integers."""
import ctypes

import pytest

import ecdsa_probe_model as pm
from test_ecdsa import col_max, emu_lib

TABLES = pm.tables()


@pytest.fixture(scope="module")
def emu():
    return emu_lib()


def run(emu, op, rows, tabs=None, n_tabs=0):
    ni, no, _ = pm.OPS[op]
    n = len(rows)
    flat = [w for r in rows for w in r]
    assert len(flat) == n * ni, op
    a_in = (ctypes.c_uint32 * (n * ni))(*flat)
    a_out = (ctypes.c_uint32 * (n * no))(*([0xa5a5a5a5] * (n * no)))
    act = (ctypes.c_uint8 * n)(*([1] * n))
    assert emu.emu_ecp(op.encode(), n, act, a_in, a_out, tabs, n_tabs) == 0, op
    return [list(a_out[i * no:(i + 1) * no]) for i in range(n)]


@pytest.mark.parametrize("op", sorted(TABLES))
def test_primitive(emu, op):
    col_max(emu, reset=True)
    pm.check(op, TABLES[op], run(emu, op, TABLES[op]))
    assert col_max(emu) < emu.emu_ecdsa_col_bound()


def test_column_bound_is_reached_only_from_below(emu):
    """The lazy maxima (digits 0..8 at 3 * (2^28 - 1), digit 9 at 93) come close to the header's bound: the
    middle column holds eight products of two full digits (the two with digit 9 are small)."""
    col_max(emu, reset=True)
    lz = pm.lazy_max()
    run(emu, "fe_mul", [lz + lz])
    run(emu, "fe_sqr", [lz])
    run(emu, "sc_mul", [lz + lz])
    top = col_max(emu)
    assert 8 * (3 * pm.M28) ** 2 <= top < emu.emu_ecdsa_col_bound()


def test_verify_loop_on_integers(emu):
    key, rows, want = pm.verify_rows()
    kt = run(emu, "key_table", [[len(key)] + pm.bytes_words(key, 17), [65] + pm.bytes_words(pm.m.key_bytes(pm.m.G), 17)])
    assert kt[0][0] == 0 and kt[1][0] == 0
    tabs = (ctypes.c_uint32 * 480)(*(kt[0][1:] + kt[1][1:]))
    got = run(emu, "verify_scalars", [[0, 1] + pm.words(e) + pm.words(r) + pm.words(s) for e, r, s in rows], tabs, 2)
    assert [g[0] for g in got] == want


def key_tables(emu, keys):
    kt = run(emu, "key_table", [[len(k)] + pm.bytes_words(k, 17) for k in keys])
    assert all(t[0] == 0 for t in kt)
    return (ctypes.c_uint32 * (240 * len(keys)))(*[w for t in kt for w in t[1:]])


def test_ladder_on_ring_point_mul_rows_and_corner_scalars(emu):
    keys, rows, want = pm.mul_rows()
    tabs = key_tables(emu, keys + [pm.m.key_bytes(pm.m.G)])
    got = run(emu, "double_mul", [[q, len(keys)] + pm.words(u1) + pm.words(u2) for q, u1, u2 in rows], tabs, len(keys) + 1)
    pm.check_mul(rows, got, want)
    assert col_max(emu) < emu.emu_ecdsa_col_bound()
