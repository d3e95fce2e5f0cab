"""CPU: the final-exponentiation programs of cess_amd/csrc/bls/staged.hpp.

a^|x| is built from the three powers a^(2^16), a^(2^48), a^(2^57) with
|x| = 2^16 + 2^48 + (8 - 1)(16 - 1) 2^57 (four Fp12 products per power), and
the verdict-only program decides m^(3 h) = 1 through
3 h = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3 instead of m^h = 1 (h the hard
exponent).  The exponent identities are checked on the oracle's integers; the
programs run through the host build of the device headers (tests/hostemu,
-DCESS_HOSTEMU) on the golden records."""
import ctypes
import math
import os
import subprocess

import pytest

import oracle.bls_oracle as o

HERE = os.path.dirname(os.path.abspath(__file__))
FE_OPS = {"LOAD": 0, "STORE": 1, "MUL": 2, "SQN": 3, "CONJ": 4, "FROB": 5, "INV": 6, "CHAIN": 7}


def _host_lib(src_name, lib_name):
    src = os.path.join(HERE, "hostemu", src_name)
    lib = os.path.join(HERE, "hostemu", lib_name)
    hdr_dir = os.path.join(HERE, "..", "cess_amd", "csrc", "bls")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr_dir, f)) for f in os.listdir(hdr_dir)])
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", src, "-o", lib])
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def fe():
    return _host_lib("fe_prog_emu.cpp", "libfe_prog_emu.so")


@pytest.fixture(scope="module")
def emu():
    return _host_lib("emu.cpp", "libemu.so")


def _subfield_records():
    """Secret keys 1 and r - 1: the Miller value lies in Fp6, m = 1, every
    compressed power has z2 = z3 = 0 (the chain's Granger-Scott fallback)."""
    recs = []
    for msg in (b"", b"subfield miller value"):
        h = o.hash_to_g1(msg)
        for sig_pt, pk_pt in ((h, o.G2_GEN), (o.ec_neg(o.FP, h), o.ec_neg(o.FP2, o.G2_GEN))):
            recs.append((o.g1_to_compressed(sig_pt), msg, o.g2_to_compressed(pk_pt)))
    return recs


def test_exponent_identities():
    p, r, x = o.P, o.R, o.X
    assert x < 0 and -x == 0xD201000000010000
    assert 2**16 + 2**48 + 7 * 15 * 2**57 == -x
    assert 7 == 8 - 1 and 15 == 16 - 1
    # t = b^8 conj(b) = b^7, y = t^16 conj(t) = t^15 = b^105
    assert (8 - 1) * (16 - 1) == 105
    assert (p**4 - p**2 + 1) % r == 0
    hard = (p**4 - p**2 + 1) // r
    assert 3 * hard == (x - 1) ** 2 * (x + p) * (x * x + p * p - 1) + 3
    assert math.gcd(3, r) == 1
    # the whole exponent the verdict-only program applies to the Miller value
    easy = (p**6 - 1) * (p**2 + 1)
    assert easy * hard == (p**12 - 1) // r


def test_program_shape(fe):
    """Fp12 products: 2 (easy part) + 5 powers x 4 + 6 glue = 28 in the
    verdict-only program; the Gt-output program keeps the reference's nine
    glue products and its final one: 2 + 20 + 10 = 32.  Each power is one
    FE_CHAIN (57 compressed squarings) and 3 + 4 Granger-Scott squarings."""
    cnt = lambda verify, op, sqn=0: fe.emu_fe_prog_count(verify, FE_OPS[op], sqn)
    assert cnt(1, "MUL") == 28
    assert cnt(0, "MUL") == 32
    for verify in (0, 1):
        assert cnt(verify, "CHAIN") == 5
        assert cnt(verify, "INV") == 1
    assert cnt(1, "SQN", 1) == 5 * 7 + 1
    assert cnt(0, "SQN", 1) == 5 * 7 + 2
    # slots: F, M, T0, T1, T3..T6, X0..X2, XT, TM
    assert fe.emu_fe_slot_count() == 13


def _both(fe, rec):
    s, m, k = rec
    gt = (ctypes.c_uint8 * 576)()
    full, ver = ctypes.c_int(-1), ctypes.c_int(-1)
    st = fe.emu_fe_both(s, m, len(m), k, ctypes.byref(full), ctypes.byref(ver), gt)
    return st, full.value, ver.value, bytes(gt)


def test_verify_program_decides_as_full_program(fe, vectors):
    """Every golden record that reaches the final exponentiation (code 0 or
    5): the verdict-only program accepts exactly when the Gt-output program's
    result is one, and the Gt bytes are the fixtures'."""
    cases = [c for c in vectors["cases"] if c["code"] in (0, 5)]
    names = [c["name"] for c in cases]
    # the classes the set must hold: (O, O) records, identity on one side only,
    # forgeries of every message length the fixtures have
    assert sum(n.startswith("identity_pair") for n in names) >= 3
    assert "identity_sig_real_pk" in names and "real_sig_identity_pk" in names
    forged_lens = {len(c["msg"]) // 2 for c in vectors["cases"] if c["name"].startswith("forged")}
    assert forged_lens == {len(c["msg"]) // 2 for c in cases if c["name"].startswith("forged")}
    assert len(forged_lens) >= 4
    ngt = 0
    for c in cases:
        rec = (bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"]))
        st, full, ver, gt = _both(fe, rec)
        assert st == 0, c["name"]
        assert full == c["code"], c["name"]
        assert ver == full, c["name"]
        if "gt" in c:
            assert gt.hex() == c["gt"], c["name"]
            ngt += 1
    assert ngt >= 8


def test_degenerate_chain_fills_three_powers(fe):
    """z2 = z3 = 0 in every compressed power (m = 1): the fallback must leave
    X0..X2 as the program reads them; both programs give one / accept.  The
    same signatures on another message are forgeries for both."""
    one = o.gt_to_bytes(o.F12_ONE)
    recs = _subfield_records()
    for rec in recs:
        assert _both(fe, rec) == (0, 0, 0, one)
    for s, m, k in recs:
        st, full, ver, gt = _both(fe, (s, m + b"!", k))
        assert (st, full, ver) == (0, 5, 5) and gt != one


def test_existing_entry_point_agrees(emu, vectors):
    """emu_verify (tests/hostemu/emu.cpp) runs both programs and returns 99
    when their verdicts differ: golden codes for the records above, the
    subfield records included."""
    for c in vectors["cases"]:
        if c["code"] not in (0, 5):
            continue
        s, m, k = bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"])
        gt = (ctypes.c_uint8 * 576)()
        assert emu.emu_verify(s, m, len(m), k, gt) == c["code"], c["name"]
        if "gt" in c:
            assert bytes(gt).hex() == c["gt"], c["name"]
    for s, m, k in _subfield_records():
        assert emu.emu_verify(s, m, len(m), k, None) == 0
