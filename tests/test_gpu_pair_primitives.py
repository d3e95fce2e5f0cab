"""GPU: every lane-pair primitive of cess_amd/csrc/bls/pair.hpp and
bls/pair_fe.hpp against integer arithmetic mod p.

k_miller2 and k_final2 are otherwise checked end to end only, where every
intermediate is a uniformly random residue and a wrong primitive shows as
"everything is code 5".  Here each primitive runs alone, through the test-only
library cess_amd/lib/libcess_pair_probe.so (tests/probe/pair_probe.hip: the
shipped headers, one kernel per operation in the production launch shape), on
the operand tables of tests/pair_probe_model.py: the range edges of each
operation's contract (0, p, 2p - 1, the 2p summand of partner_signed, product
operands up to 2^384 - 1), both representations of a residue, the zero classes
and the branches valid signatures never reach.  For every result component the
test asserts the residue (exactly, against the oracle's tower arithmetic with
R = 2^392 applied here) and the range the header promises (< 2p; < 4p
mul_nr_nr; < 6p add_xi_nr; <= 2p partner_signed); predicates must agree in
both lanes.

Placement: every operation runs with 1, 33 and 161 pairs (one pair; a wave and
one pair; two blocks, so blockIdx > 0 and a non-zero w0 in LdsPair), and once
more with every pair i mod 4 in {1, 2} switched off (one live and one dead pair
in each quad), whose results must come back as the poison they were filled
with.  Neighbouring pairs hold different operands.  Slot strides are larger
than the pair count.  The probe's kernels are compiled apart from k_miller2 /
k_final2: this checks the headers' arithmetic and lane logic, the end-to-end
parity tests keep checking those kernels' code generation."""
import ctypes
import os

import numpy as np
import pytest

import pair_probe_model as m

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cess_amd", "lib", "libcess_pair_probe.so")
MAKE_HINT = "make -C cess_amd/csrc ../lib/libcess_pair_probe.so"

_lib = []


def probe():
    if not _lib:
        if not os.path.exists(LIB):
            pytest.fail("%s is missing: build it with `%s` (or `make -C cess_amd/csrc`)" % (LIB, MAKE_HINT))
        lib = ctypes.CDLL(LIB)
        lib.pair_probe_ops.restype = ctypes.c_char_p
        lib.pair_probe_error.restype = ctypes.c_char_p
        _lib.append(lib)
    return _lib[0]


def to_words(cases, n_in):
    """(n, n_in, 2, 12) uint32 raw limbs of the cases' operands"""
    buf = b"".join(v.to_bytes(48, "little") for c in cases for x in c for v in x)
    if not n_in:
        return np.zeros((len(cases), 1, 2, 12), np.uint32)
    return np.frombuffer(buf, dtype="<u4").reshape(len(cases), n_in, 2, 12).copy()


def run(op, cases, active, want_slots=False):
    """launch op's kernel on `cases`; returns the (n, n_out, 2) results as
    Python integers per pair (None for a pair still holding the poison)"""
    lib, n = probe(), len(cases)
    stride = n + 11                      # larger than the pair count
    inp = to_words(cases, op.n_in)
    out = np.full((n, op.n_out, 2, 12), m.POISON, dtype=np.uint32)
    act = np.array(active, dtype=np.uint8)
    raw = np.zeros((lib.pair_probe_slots(), 36, stride, 4), dtype=np.uint32) if want_slots else None
    fn = getattr(lib, "pp_" + op.entry)
    rc = fn(ctypes.c_uint32(n), act.ctypes.data_as(ctypes.c_void_p), inp.ctypes.data_as(ctypes.c_void_p),
            out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(op.arg), ctypes.c_uint64(stride),
            raw.ctypes.data_as(ctypes.c_void_p) if want_slots else None)
    if rc != 0:     # a HIP error (a fault included): nothing more is launched on this device
        pytest.exit("pp_%s: HIP status %d (%s)" % (op.entry, rc, lib.pair_probe_error(rc).decode()), returncode=3)
    res = []
    for i in range(n):
        if (out[i] == m.POISON).all():
            res.append(None)
            continue
        b = out[i].astype("<u4").tobytes()
        res.append([(int.from_bytes(b[96 * v:96 * v + 48], "little"), int.from_bytes(b[96 * v + 48:96 * v + 96], "little"))
                    for v in range(op.n_out)])
    return (res, raw, stride) if want_slots else res


def check(op, n, half):
    cases = op.cases[:n]
    active = m.active_mask(n, half)
    got = run(op, cases, active)
    for i in range(n):        # every generated pair is compared
        if not active[i]:
            assert got[i] is None, (op.name, n, i, "an inactive pair's result was written")
            continue
        assert got[i] is not None, (op.name, n, i, "no result")
        m.check_result(op, i, got[i])
    return got


def test_probe_covers_the_model():
    """the library's entry points and the model's operations are the same set,
    with the same operand / result counts, in the production block size"""
    lib = probe()
    listed = {}
    for item in lib.pair_probe_ops().decode().strip(",").split(","):
        name, ni, no = item.split(":")
        listed[name] = (int(ni), int(no))
    assert lib.pair_probe_threads() == 256
    used = {}
    for op in m.ops():
        assert op.entry in listed, op.entry
        assert listed[op.entry] == (op.n_in, op.n_out), (op.name, listed[op.entry])
        used[op.entry] = True
    assert sorted(used) == sorted(listed)


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
@pytest.mark.parametrize("name", m.op_names())
def test_pair_primitive(name, half):
    """one primitive at 1, 33 and 161 pairs (cheap Fp2 operations also on their
    whole edge table), all pairs live or one live pair per quad"""
    op = m.get_op(name)
    op.check_contract()        # operands within the documented bounds, before anything is launched
    counts = list(m.PAIR_COUNTS) + ([len(op.cases)] if op.full_table else [])
    for n in counts:
        check(op, n, half)


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
@pytest.mark.parametrize("prepared,plain", [("pmul_p", "pmul_scaled1"), ("pdot2_p", "pdot2")])
def test_prepared_products_bit_for_bit(prepared, plain, half):
    """pmul_p(prep_x, prep_y) / pdot2_p give the limbs of pmul / pdot2"""
    a, b = m.get_op(prepared), m.get_op(plain)
    assert a.cases is b.cases
    n = len(a.cases)
    act = m.active_mask(n, half)
    ga, gb = run(a, a.cases, act), run(b, b.cases, act)
    assert ga == gb
    assert sum(1 for g in ga if g is not None) == sum(act)


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
def test_glob_pair_layout(half):
    """GlobPair.st puts word 4q..4q+3 of component h of coefficient k into row
    6k + 3h + q, column = pair, of a slot with a stride larger than the pair
    count, and st_full / ld_full address the same rows"""
    op = m.get_op("glob_roundtrip")
    for n in m.PAIR_COUNTS:
        cases, act = op.cases[:n], m.active_mask(n, half)
        got, raw, stride = run(op, cases, act, want_slots=True)
        words = to_words(cases, 6)
        fill = np.uint32(0xA5A5A5A5)
        for s in (0, 1):
            for i in range(n):
                col = raw[s, :, i, :].reshape(6, 2, 12)
                if act[i]:
                    assert (col == words[i]).all(), (s, n, i)
                else:
                    assert (col == fill).all(), (s, n, i)
            assert (raw[s, :, n:, :] == fill).all()      # nothing past the last pair
        assert (raw[2:] == fill).all()
