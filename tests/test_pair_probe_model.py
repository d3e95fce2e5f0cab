"""The reference side of tests/test_gpu_pair_primitives.py, with no device:
the case tables stay within each operation's contract and the integer model
alone passes every assertion the GPU results must pass; the model's store
layout reproduces the golden Gt bytes; the Karabina formulas it uses agree with
plain Fp12 squaring; the probe source exposes the operations the model knows."""
import os
import random
import re

import pytest

import oracle.bls_oracle as o
import pair_probe_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = m.P


@pytest.mark.parametrize("name", m.op_names())
def test_case_table_and_reference(name):
    """operands within the documented bounds, neighbouring pairs different,
    and the reference's own result (reduced into the promised range) passes
    the residue, range, lane-agreement and exact-limb assertions"""
    op = m.get_op(name)
    op.check_contract()
    assert len(op.cases) >= m.PAIR_COUNTS[-1]
    for i in range(len(op.cases)):
        got = m.model_result(op, i)
        m.check_result(op, i, got)
        if not op.pred and not op.exact:
            # the other representation is accepted too, a value past the bound is not
            m.check_result(op, i, [(a + P, b + P) for a, b in got])
            with pytest.raises(AssertionError):
                m.check_result(op, i, [(a + P * ((op.out_bound - a + P - 1) // P), b) for a, b in got])
    if not op.pred:
        with pytest.raises(AssertionError):   # a wrong residue is refused
            g = m.model_result(op, 0)
            m.check_result(op, 0, [((g[0][0] + 1) % P, g[0][1])] + g[1:])


def test_tables_hold_the_edge_classes():
    """the cases the issue names are in the tables, inside the first 161 where
    the operation runs on 161 pairs only"""
    S = set(m.STORED_EDGES)
    assert {0, 1, P - 1, P, P + 1, 2 * P - 1, m.ONE, m.ONE + P, (1 << 380) - 1} <= S
    assert {2 * P, 4 * P - 1, 6 * P - 1, 8 * P - 1, m.TOP, m.TOP - 1, 1 << 383, (1 << 364) - 1} <= set(m.PRODUCT_EDGES)
    for name in ("pmul_scaled1", "pmul_scaled2", "pmul_scaled3", "pmul_p"):
        c = m.get_op(name).cases
        T = m.TOP
        for combo in ([(T, T), (T, T)], [(T, 0), (T, T)], [(0, T), (T, T)]):
            assert combo in c[:m.PAIR_COUNTS[-1]], name
    for name in ("pdot2", "pdot2_p"):
        assert [(m.TOP, m.TOP)] * 4 in m.get_op(name).cases[:m.PAIR_COUNTS[-1]]
    # pinv / is_zero: the four zero classes; mul_nr: a1 = 0 and a0 = 0 (the 2p summand)
    for name in ("pinv", "is_zero", "mul_nr", "mul_nr_nr", "psqr", "conj"):
        c = m.get_op(name).cases
        for z in ([(0, 0)], [(0, P)], [(P, 0)], [(P, P)]):
            assert z in c, name
    for name in ("mul_nr", "mul_nr_nr", "partner_signed"):
        first = m.get_op(name).cases[:6]
        assert [(2 * P - 1, 0)] in first and [(0, 2 * P - 1)] in first
    # x and x + p of the same residues
    for name in ("psqr", "pinv"):
        c = m.get_op(name).cases
        assert any([(m._twin(a), m._twin(b)) for a, b in x] in c for x in c[:10]), name
    for name in ("pmul6", "psqr12", "pmul014", "pmul014_one", "pmul12", "pinv12", "pfrob12_k1", "pcyc_z0"):
        c = m.get_op(name).cases[:m.PAIR_COUNTS[-1]]
        tw = sum(1 for x, y in zip(c, c[1:]) if y == [(m._twin(a), m._twin(b)) for a, b in x])
        assert tw >= 15, name
    # pis_one12 on 1 written as (ONE + p, p, 0, ...); pis_conj12 with b's coefficients 0 and p
    one = m.get_op("pis_one12_lds")
    assert any(c[0] == (m.ONE + P, P) and e for c, e in zip(one.cases, one.expected()))
    assert sum(1 for e in one.expected() if e) >= 40 and sum(1 for e in one.expected() if not e) >= 80
    cj = m.get_op("pis_conj12")
    assert any(e and 0 in sum(c[6:], ()) and P in sum(c[6:], ()) for c, e in zip(cj.cases, cj.expected()))
    assert sum(1 for e in cj.expected() if e) >= 40 and sum(1 for e in cj.expected() if not e) >= 80
    # z1: z2 a zero class with z3 != 0, z2 = z3 = 0, general
    for name in ("pcyc_z1_frac", "pcyc_z1_den"):
        op = m.get_op(name)
        kinds = set()
        for c in op.cases:
            z2, z3 = m.res2(c[0]), m.res2(c[1])
            kinds.add((m.f2_is_zero(z2), m.f2_is_zero(z3), c[0] if m.f2_is_zero(z2) else None))
        for zc in ((0, 0), (0, P), (P, 0), (P, P)):
            assert (True, False, zc) in kinds and (True, True, zc) in kinds, name
        assert (False, False, None) in kinds
    # the element 1 among the cyclotomic operands (FE_CHAIN's degenerate path)
    ch = m.get_op("pcyc_chain")
    ones = [i for i, a in enumerate(m.cyc_elements()) if a == o.F12_ONE]
    assert len(ones) >= 4 and any(i < 33 for i in ones)
    for i in ones:
        assert ch.expected()[i] == m.to_store(o.F12_ONE) * 3


def test_store_layout_matches_golden_gt(vectors):
    """coefficient <-> store index, component <-> lane and the Gt byte order of
    the model reproduce the golden `gt` bytes from the oracle's Fp12"""
    case = next(c for c in vectors["cases"] if c.get("gt") and c["code"] == 5)
    gt = bytes.fromhex(case["gt"])
    sig, pk = o.g1_from_compressed(bytes.fromhex(case["sig"])), o.g2_from_compressed(bytes.fromhex(case["pk"]))
    f = o.verify_gt(sig, bytes.fromhex(case["msg"]), pk)
    assert f != o.F12_ONE and o.gt_to_bytes(f) == gt
    store = [m.mont2(x) for x in m.to_store(f)]                      # the accumulator image, canonical
    assert m.store_to_gt_bytes(store) == gt
    assert m.store_to_gt_bytes([(a + P, b + P) for a, b in store]) == gt    # any representation
    assert m.from_store(m.to_store(f)) == f
    # Karabina's names by store index (staged.hpp): z0 = c0.c0, z4 = c0.c1, z3 = c0.c2, z2 = c1.c0, z1 = c1.c1, z5 = c1.c2
    s = m.to_store(f)
    assert (s[m.Z_INDEX["z0"]], s[m.Z_INDEX["z4"]], s[m.Z_INDEX["z3"]]) == f[0]
    assert (s[m.Z_INDEX["z2"]], s[m.Z_INDEX["z1"]], s[m.Z_INDEX["z5"]]) == f[1]
    one = next(c for c in vectors["cases"] if c.get("gt") and c["code"] == 0)
    assert m.store_to_gt_bytes([m.mont2(x) for x in m.to_store(o.F12_ONE)]) == bytes.fromhex(one["gt"])


def test_karabina_formulas_match_f12_sqr():
    """compressed squaring + decompression, written as formulas, equal f12_sqr
    iterated on cyclotomic elements; the z2 = 0 formula in its constructible
    limit (z2..z5 all zero)"""
    rng = random.Random(77)
    for t in range(6):
        a = m.easy_part(m.from_store([(rng.randrange(P), rng.randrange(P)) for _ in range(6)]))
        s = m.to_store(a)
        z = tuple(s[m.Z_INDEX[k]] for k in ("z2", "z3", "z4", "z5"))
        assert m.kcyc_decompress(*z) == a
        want = a
        for n in range(1, 5):
            z = m.kcyc_square(*z)
            want = o.f12_sqr(want)
            ws = m.to_store(want)
            assert z == tuple(ws[m.Z_INDEX[k]] for k in ("z2", "z3", "z4", "z5")), (t, n)
            assert m.kcyc_decompress(*z) == want, (t, n)
    # the shared powers of the GPU test are these iterates
    el, pw = m.cyc_elements(), m.cyc_powers()
    for i in (0, 1, 33, 160):
        z = tuple(m.to_store(el[i])[m.Z_INDEX[k]] for k in ("z2", "z3", "z4", "z5"))
        for n in range(1, 17):
            z = m.kcyc_square(*z)
            if n in (1, 2, 16):
                assert z == tuple(m.to_store(pw[i][n])[m.Z_INDEX[k]] for k in ("z2", "z3", "z4", "z5")), (i, n)
    # limit case: z2 = z3 = z4 = z5 = 0 (the element 1) squares to itself; the
    # z2 = 0 formula gives num = 2 z4 z5 = 0 over den = z3 = 0: not decompressible
    zero = (o.F2_ZERO,) * 4
    assert m.kcyc_square(*zero) == zero
    assert m.z1_frac(*zero) == (o.F2_ZERO, o.F2_ZERO) and m.kcyc_decompress(*zero) is None
    # with z1 = 0 (what 0 / den stands for in that limit) the z0 formula gives 1
    assert m.z0_of(o.F2_ZERO, *zero) == o.F2_ONE
    # z2 = 0, z3 != 0: num = 2 z4 z5 over den = z3
    z3, z4, z5 = [(rng.randrange(P), rng.randrange(P)) for _ in range(3)]
    num, den = m.z1_frac(o.F2_ZERO, z3, z4, z5)
    assert den == z3 and num == o.f2_add(o.f2_mul(z4, z5), o.f2_mul(z4, z5))


def test_pkcyc_operand_layout_matches_header():
    """(u, w) per lane -- lane 0 (z4, z5), lane 1 (z3, z2) -- as the comment of
    pkcyc_run_ps and the store indices in pcyc_chain say, and as the probe
    passes them"""
    hdr = open(os.path.join(ROOT, "cess_amd", "csrc", "bls", "pair_fe.hpp")).read()
    assert "Lane 0 holds (u, w) = (z4, z5), lane 1 (u, w) = (z3, z2)" in hdr
    mm = re.search(r"const int ku = hi \? (\d) : (\d), kw = hi \? (\d) : (\d);", hdr)
    assert mm, "pcyc_chain's store indices of (u, w)"
    ku1, ku0, kw1, kw0 = map(int, mm.groups())
    assert ((ku0, kw0), (ku1, kw1)) == m.PS_LANE_UW
    assert m.PS_LANE_UW == ((1, 5), (2, 3))
    # the same update on what each lane receives: u' = P - 2u, w' = 2 (w + Q) with
    # lane 0's (P, Q) = lane 1's (A, b3) and the reverse, against kcyc_square
    rng = random.Random(5)
    z2, z3, z4, z5 = [(rng.randrange(P), rng.randrange(P)) for _ in range(4)]
    lanes = {0: (z4, z5), 1: (z3, z2)}
    sent = {}
    for h, (u, w) in lanes.items():
        b3 = m.f2_muli(o.f2_mul(u, w), 3)
        if h == 0:
            A = m.f2_muli(o.f2_add(o.f2_sqr(u), o.f2_mul_nr(o.f2_sqr(w))), 3)
            sent[h] = (A, o.f2_mul_nr(b3))
        else:
            A = m.f2_muli(o.f2_add(o.f2_sqr(w), o.f2_mul_nr(o.f2_sqr(u))), 3)
            sent[h] = (A, b3)
    new = {}
    for h, (u, w) in lanes.items():
        Pv, Q = sent[1 - h]
        new[h] = (o.f2_sub(Pv, m.f2_muli(u, 2)), m.f2_muli(o.f2_add(w, Q), 2))
    assert (new[1][1], new[1][0], new[0][0], new[0][1]) == m.kcyc_square(z2, z3, z4, z5)
    # the probe hands lane h the operands (z2, z3, z4, z5)[vu], [vw]
    src = open(os.path.join(ROOT, "tests", "probe", "pair_probe.hip")).read()
    assert "const int vu = h ? 1 : 2, vw = h ? 0 : 3;" in src


def test_probe_source_lists_the_model_operations():
    """every operation of the model has an entry point in the probe source with
    the same operand / result counts, and the reverse"""
    src = open(os.path.join(ROOT, "tests", "probe", "pair_probe.hip")).read()
    listed = {n: (int(a), int(b)) for n, a, b in re.findall(r"^\s+X\((\w+), (\d+), (\d+)\)", src, re.M)}
    assert len(listed) >= 37
    used = set()
    for op in m.ops():
        assert listed.get(op.entry) == (op.n_in, op.n_out), op.name
        used.add(op.entry)
    assert used == set(listed)
    mk = open(os.path.join(ROOT, "cess_amd", "csrc", "Makefile")).read()
    assert "$(OUT)/libcess_pair_probe.so" in mk.split("all:")[1].split("\n")[0]
