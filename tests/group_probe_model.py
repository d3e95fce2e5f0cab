"""Operand tables and integer references of the lane-group layer
(cess_amd/csrc/bls/group.hpp: grp_mul_comp, grp_sqr_comp, grp_operand, the LIN
and INV forms of group_eval_comp; the two programs of gen_group.py run by
k_group and k_group_fe), shared by the host build
(tests/test_group_primitives.py) and the GPU probe
(tests/test_gpu_group_primitives.py, tests/probe/group_probe.hip).

Plain Python integers mod p; nothing is taken from group.hpp.  A register-file
component is raw limbs with raw = x R (mod p), R = 2^392, anywhere in [0, 2p);
the model works on the raw integers themselves: a product is A B / R, a
combination a sum, an inverse R^2 / A.  Whole programs are gen_group.simulate()
(group rows built from arbitrary field values) and oracle/bls_oracle.py
(final exponentiations, real records).

Everything is exact: a result is right when it is congruent to the model's
value mod p AND below 2p (the register-file contract), an unwritten word when
it is bit-identical.

`mut` (None in every real use) plants ONE deliberate error in the model, for
the self-test that the tables notice each of them: "k28" (NEG_K28 off by one
in one digit), "nosub" (the subtract flag ignored), "xisign" (LIN's xi sign
flipped), "early" (writes landing before the reads of later operations).
"""
import importlib.util
import os
import random
import re

import oracle.bls_oracle as o
from lane_probe_model import ONE, P, POISON, R, RINV, mont, val, words
from pair_probe_model import _twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cess_amd", "csrc")
M28 = (1 << 28) - 1
OP_MUL, OP_SQR, OP_LIN, OP_INV = 0, 1, 2, 3
OPS = {"grp_mul_comp": (48, 24), "grp_sqr_comp": (24, 24), "round": (129, 0), "group_fe": (144, 145), "group": (96, 145)}
PAIR_COUNTS = (1, 65, 321)            # rows: lanes 2, 130, 642 (one pair; two waves and a pair; ten waves and a pair)
BLOCK_COUNTS = (1, 2, 65)             # one-wave blocks of the whole-kernel entries
ROUND_SLOTS, ROUND_USED = 64, 56      # the round table's image: 56 slots of values, 8 of poison
INF_SIG, INF_PK = 1, 2
GT_ONE = o.gt_to_bytes(o.F12_ONE)
_cache = {}


# --- the generator and the constants the code under test was built with ----------------
def gen():
    if "gen" not in _cache:
        spec = importlib.util.spec_from_file_location("gen_group", os.path.join(CSRC, "gen_group.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _cache["gen"] = m
    return _cache["gen"]


def programs():
    """{"full": generate(), "fe": generate(build_fe(pool))}: (g, rounds, slot, nslots, heads, ents) each"""
    if "progs" not in _cache:
        m = gen()
        full = m.generate()
        _cache["progs"] = {"full": full, "fe": m.generate(m.build_fe(full[0].consts))}
    return _cache["progs"]


def pool():
    """the constant pool as raw Montgomery Fp2 values"""
    return [(mont(c[0]), mont(c[1])) for c in programs()["full"][0].consts]


def _array(name):
    with open(os.path.join(CSRC, "bls", "consts.hpp")) as f:
        m = re.search(r"\b%s\[14\] = \{([^}]*)\}" % name, f.read())
    return [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]


NEG_K28 = _array("NEG_K28")
P28 = _array("P28")
K_VALUE = sum(k << (28 * i) for i, k in enumerate(NEG_K28))


def digits(v):
    """unpack28 of a 12-word value"""
    assert 0 <= v < 1 << 384
    return [(v >> (28 * i)) & M28 for i in range(13)] + [v >> 364]


def program_forms(prog):
    """the (kind, flag byte) of every MUL / SQR entry, the (n0, n1, n2, n3) of every LIN entry, the INV count"""
    heads, ents = prog[4], prog[5]
    flags, shapes, inv = set(), set(), 0
    for kind, cnt, off in heads:
        for e in ents[off:off + cnt]:
            if kind in (OP_MUL, OP_SQR):
                flags.add((kind, e[5]))
            elif kind == OP_LIN:
                shapes.add((e[1] & 15, e[1] >> 4, e[2] & 15, e[2] >> 4))
            else:
                inv += 1
    return flags, shapes, inv


def found_forms():
    out = [program_forms(p) for p in programs().values()]
    return out[0][0] | out[1][0], out[0][1] | out[1][1], out[0][2] + out[1][2]


# --- operand classes (what grp_operand can hand to a product) -----------------------------
def operand_class(f, present, subtract, is_const, conj):
    """the class of the operand a flag byte selects, as grp_operand and group_eval_comp are written"""
    base = "const" if f & is_const else "slot"
    if f & present:
        return base + ("-slot" if f & subtract else "+slot")
    return "conj" if f & conj else base


def flag_classes(kind, f):
    a = operand_class(f, 1, 2, 16, 64)
    return (a, a) if kind == OP_SQR else (a, operand_class(f, 4, 8, 32, 0))


# the largest component each class can hold (exclusive bounds 2p, p, 4p, 3p; sub() and neg() return < 2p)
CLASS_MAX = {"slot": 2 * P - 1, "const": P - 1, "slot+slot": 4 * P - 2, "const+slot": 3 * P - 2, "slot-slot": 2 * P - 1,
             "const-slot": 2 * P - 1, "conj": 2 * P - 1}


def _digit_edges(bound):
    """one-hot digits, one digit at its maximum, every digit 0xfffffff below each admissible top digit"""
    top = (bound - 1) >> 364
    out = [1 << (28 * i) for i in range(14)] + [M28 << (28 * i) for i in range(13)] + [top << 364]
    out += [(t << 364) | ((1 << 364) - 1) for t in (0, 1, top - 1, top)]
    out += [((1 << 364) - 1) ^ (M28 << (28 * i)) for i in (0, 6, 12)]
    return [v for v in out if v < bound]


def class_edges(cls):
    """a class's extremes: 0, 1, R mod p, p - 1, p, p + 1, 2p - 1 (4p - 2 for sums), the digit patterns, and
    x + p beside every x < p"""
    if cls == "const":
        vals = [0, 1, ONE, P - 1] + [c for v in pool()[:6] for c in v]
        return sorted(set(vals))
    bound = CLASS_MAX[cls] + 1
    vals = [0, 1, ONE, P - 1, P, P + 1, 2 * P - 1] + _digit_edges(bound)
    if cls == "conj":                    # c1 = 2p - x of a stored x, 0 for 0
        vals = [0 if v == 0 else 2 * P - v for v in vals if v < 2 * P] + [0, 1]
    if "+" in cls:
        vals += [bound - 1, bound - 2, 2 * P, 3 * P - 1, 3 * P, 2 * P + ONE]
    vals += [v + P for v in vals if v < P and v + P < bound]
    return sorted(set(v for v in vals if v < bound))


def _class_pairs():
    return sorted({flag_classes(kind, f) for kind, f in found_forms()[0] if kind == OP_MUL})


def _class_singles():
    flags = found_forms()[0]
    return sorted({flag_classes(kind, f)[0] for kind, f in flags})       # a SQR riding in a MUL round squares class A too


def _separate(rows, tags):
    keep = [i for i in range(len(rows)) if i == 0 or rows[i] != rows[i - 1]]
    return [rows[i] for i in keep], [tags[i] for i in keep]


def mul_rows():
    """(A, B) raw Fp2 pairs, components below 4p, and a tag each"""
    if "mul" in _cache:
        return _cache["mul"]
    rng = random.Random("group-probe-mul")
    rows, tags = [], []
    for ca, cb in _class_pairs():                    # the product of the two maxima, then each class's extremes
        ma, mb = CLASS_MAX[ca], CLASS_MAX[cb]
        rows.append(((ma, ma), (mb, mb)))
        tags.append(("maxima", ca, cb))
        ea, eb = class_edges(ca), class_edges(cb)
        for e in ea:
            rows += [((e, rng.choice(ea)), (rng.choice(eb), mb)), ((rng.randrange(ma + 1), e), (mb, rng.randrange(mb + 1)))]
            tags += [("edge a0", ca, cb, hex(e)), ("edge a1", ca, cb, hex(e))]
        for e in eb:
            rows += [((ma, rng.choice(ea)), (e, rng.choice(eb))), ((rng.randrange(ma + 1), ma), (rng.randrange(mb + 1), e))]
            tags += [("edge b0", ca, cb, hex(e)), ("edge b1", ca, cb, hex(e))]
        for _ in range(12):
            rows.append(((rng.randrange(ma + 1), rng.randrange(ma + 1)), (rng.randrange(mb + 1), rng.randrange(mb + 1))))
            tags.append(("random", ca, cb))
    for cls in sorted(CLASS_MAX):                    # every class against itself, uniform extremes
        for e in class_edges(cls)[::3]:
            rows.append(((e, e), (e, e)))
            tags.append(("uniform", cls, hex(e)))
    for _ in range(60):
        rows.append(tuple((rng.randrange(4 * P - 1), rng.randrange(4 * P - 1)) for _ in range(2)))
        tags.append(("random", "any", "any"))
    _cache["mul"] = _separate(rows, tags)
    return _cache["mul"]


def sqr_rows():
    if "sqr" in _cache:
        return _cache["sqr"]
    rng = random.Random("group-probe-sqr")
    rows, tags = [], []
    for cls in sorted(set(_class_singles()) | set(CLASS_MAX)):
        m = CLASS_MAX[cls]
        rows.append((m, m))
        tags.append(("maximum", cls))
        edges = class_edges(cls)
        for e in edges:
            rows += [(e, rng.choice(edges)), (rng.randrange(m + 1), e), (e, m), (m, e)]
            tags += [("edge a0", cls, hex(e)), ("edge a1", cls, hex(e)), ("edge a0, max", cls, hex(e)), ("max, edge a1", cls, hex(e))]
        for _ in range(12):
            rows.append((rng.randrange(m + 1), rng.randrange(m + 1)))
            tags.append(("random", cls))
    _cache["sqr"] = _separate(rows, tags)
    return _cache["sqr"]


def mul_ref(A, B):
    return ((A[0] * B[0] - A[1] * B[1]) * RINV % P, (A[0] * B[1] + A[1] * B[0]) * RINV % P)


def half_product(x0, y0, x1, y1):
    """sum_k 2^(28k) sum_{i+j=k} (x0_i y0_j + x1_i y1_j) of digit vectors, and its largest column"""
    cols = [0] * 27
    for i in range(14):
        for j in range(14):
            cols[i + j] += x0[i] * y0[j] + x1[i] * y1[j]
    return sum(c << (28 * k) for k, c in enumerate(cols)), max(cols)


def mul_comp_digits(A, B, comp, K=NEG_K28):
    """the double-width value grp_mul_comp reduces, from the digits (K - b1 digit-wise for -b1), and its largest column"""
    a0, a1, b0, b1 = (digits(v) for v in (A[0], A[1], B[0], B[1]))
    nb1 = [k - d for k, d in zip(K, b1)]
    assert min(nb1) >= 0
    return half_product(a0, b1, a1, b0) if comp else half_product(a0, b0, a1, nb1)


def sqr_comp_digits(A, comp, K=NEG_K28):
    a0, a1 = digits(A[0]), digits(A[1])
    zero = [0] * 14
    if comp:
        return half_product(a0, [2 * d for d in a1], zero, zero)
    return half_product([x + y for x, y in zip(a0, a1)], [x + k - y for x, k, y in zip(a0, K, a1)], zero, zero)


def k28_mutant():
    K = list(NEG_K28)
    K[5] += 1
    return K


def expect_comp(name, row, mut=None):
    """both components of a row's result, as residues"""
    if mut == "k28":
        f = (lambda c: mul_comp_digits(row[0], row[1], c, k28_mutant())) if name == "grp_mul_comp" else \
            (lambda c: sqr_comp_digits(row, c, k28_mutant()))
        return tuple(f(c)[0] * RINV % P for c in (0, 1))
    return mul_ref(row[0], row[1]) if name == "grp_mul_comp" else mul_ref(row, row)


def comp_table(name):
    return mul_rows() if name == "grp_mul_comp" else sqr_rows()


def comp_words(name, row):
    if name == "grp_mul_comp":
        return words(row[0][0]) + words(row[0][1]) + words(row[1][0]) + words(row[1][1])
    return words(row[0]) + words(row[1])


def active_rows(n, half):
    """all rows live, or rows i mod 4 in {1, 2} switched off"""
    return [0 if half and i % 4 in (1, 2) else 1 for i in range(n)]


def _p(x):
    import ctypes
    return x.ctypes.data_as(ctypes.c_void_p)


def run_comp(call, name, n_rows, active):
    """rows 0..n_rows of the table through call(name, lanes, active, in, out) -> status; the (2 n_rows, 12) results"""
    import numpy as np
    rows, _ = comp_table(name)
    inp = np.array([comp_words(name, r) for r in rows[:n_rows]], dtype=np.uint32)
    out = np.full((2 * n_rows, 12), POISON, dtype=np.uint32)
    act = np.array(active, dtype=np.uint8)
    assert inp.shape == (n_rows, OPS[name][0]) and len(act) == n_rows
    return call(name, 2 * n_rows, _p(act), _p(inp), _p(out)), out


def check_comp(name, out, active, mut=None):
    """every lane: the named component of A B / R (A^2 / R) mod p, below 2p; a switched-off row's lanes still poison"""
    rows, tags = comp_table(name)
    for r, live in enumerate(active):
        if not live:
            assert (out[2 * r:2 * r + 2] == POISON).all(), (name, r, "an inactive row's result was written")
            continue
        want = expect_comp(name, rows[r], mut)
        for c in (0, 1):
            got = val(out[2 * r + c])
            assert got < 2 * P, (name, r, c, tags[r], "bound", hex(got))
            assert got % P == want[c], (name, r, c, tags[r], "value", hex(got))


# --- one round --------------------------------------------------------------------------------
class Case:
    """one row of the round table: a header, 32 entries (16 bytes each), the image as raw Fp2 values"""

    def __init__(self, kind, ents, image, off=0, tag=None):
        self.kind, self.cnt, self.off, self.tag = kind, len(ents), off, tag
        assert 1 <= self.cnt <= 32 and off + self.cnt <= 32
        filler = [0xEE] * 16                      # never fetched: lanes of ops >= cnt idle
        self.ents = [filler] * off + [list(e) for e in ents] + [filler] * (32 - off - self.cnt)
        self.image = list(image)

    def head(self):
        return self.kind | (self.cnt << 8) | (self.off << 16)

    def ent_words(self):
        return [e[4 * q] | (e[4 * q + 1] << 8) | (e[4 * q + 2] << 16) | (e[4 * q + 3] << 24) for e in self.ents for q in range(4)]


def mul_entry(d, a0, a1, b0, b1, f):
    return [d, a0, a1, b0, b1, f] + [0] * 10


def lin_entry(d, classes):
    n = [len(c) for c in classes]
    assert sum(n) <= 12
    e = [d, n[0] | (n[1] << 4), n[2] | (n[3] << 4)] + [s for c in classes for s in c]
    return e + [0] * (16 - len(e))


def inv_entry(d, a):
    return [d, a] + [0] * 14


def _operand(img, x0, x1, f, present, subtract, is_const, mut):
    v = pool()[x0] if f & is_const else img[x0]
    if f & present:
        t = img[x1]
        if f & subtract and mut != "nosub":
            v = (v[0] - t[0], v[1] - t[1])
        else:
            v = (v[0] + t[0], v[1] + t[1])
    return v


def eval_entry(kind, e, img, mut=None):
    """-> (destination slot, (c0, c1) residues of raw values): the operation on integers"""
    if kind in (OP_MUL, OP_SQR):
        d, a0, a1, b0, b1, f = e[:6]
        A = _operand(img, a0, a1, f, 1, 2, 16, mut)
        if f & 64:
            A = (A[0], -A[1])
        B = A if kind == OP_SQR else _operand(img, b0, b1, f, 4, 8, 32, mut)
        return d, mul_ref(A, B)
    if kind == OP_LIN:
        n = (e[1] & 15, e[1] >> 4, e[2] & 15, e[2] >> 4)
        acc, accx, p = [0, 0], [0, 0], 3
        for cls, cnt in enumerate(n):
            for _ in range(cnt):
                t, sign, tgt = img[e[p]], -1 if cls & 1 else 1, acc if cls < 2 else accx
                tgt[0] += sign * t[0]
                tgt[1] += sign * t[1]
                p += 1
        s = -1 if mut == "xisign" else 1          # xi (x0 + x1 u) = (x0 - x1) + (x0 + x1) u
        return e[0], ((acc[0] + accx[0] - s * accx[1]) % P, (acc[1] + accx[0] + s * accx[1]) % P)
    a = img[e[1]]
    x = (a[0] % P, a[1] % P)
    if x == (0, 0):
        return e[0], (0, 0)
    y = o.f2_inv(x)                               # (x R)^-1 R^2
    return e[0], (y[0] * R * R % P, y[1] * R * R % P)


def round_model(case, mut=None):
    """{slot: (c0, c1) residues} of the slots the round writes: every operation reads the image as it was"""
    img = list(case.image)
    writes = {}
    for e in case.ents[case.off:case.off + case.cnt]:
        d, v = eval_entry(case.kind, e, img, mut)
        assert d not in writes, "two operations of a round write one slot"
        writes[d] = v
        if mut == "early":
            img[d] = v
    return writes


def _edge_cycle(seed):
    rng = random.Random(seed)
    edges = class_edges("slot")
    rng.shuffle(edges)
    return edges


def images(n_used=ROUND_USED, n_slots=ROUND_SLOTS):
    """three images: random values, the extremes, every slot at 2p - 1"""
    rng = random.Random("group-probe-images")
    e = _edge_cycle("group-probe-image-edges")
    out = [[(rng.randrange(2 * P), rng.randrange(2 * P)) for _ in range(n_used)],
           [(e[(2 * i) % len(e)], e[(2 * i + 7) % len(e)]) for i in range(n_used)],
           [(2 * P - 1, 2 * P - 1)] * n_used]
    return out


def table_flags():
    """the MUL / SQR flag bytes of the round table: every combination of bits 1..32 with bit 64 clear (what the
    programs use and what they do not), and the programs' bytes with bit 64"""
    found = {f for _, f in found_forms()[0]}
    return sorted(set(range(64)) | found)


def table_shapes():
    return sorted(found_forms()[1] | {(12, 0, 0, 0), (0, 12, 0, 0), (0, 0, 12, 0), (0, 0, 0, 12), (3, 3, 3, 3)})


def _chunks(items, sizes):
    out, at = [], 0
    for s in sizes:
        if at < len(items):
            out.append(items[at:at + s])
            at += s
    while at < len(items):
        out.append(items[at:at + 32])
        at += 32
    return out


def round_cases():
    if "round" in _cache:
        return _cache["round"]
    rng = random.Random("group-probe-round")
    nc, nu = len(pool()), ROUND_USED
    imgs = images()
    cases = []

    def mul_ops(flags, dests):
        return [mul_entry(d, rng.choice((0, nc - 1, rng.randrange(nc))) if f & 16 else rng.randrange(nu), rng.randrange(nu),
                          rng.choice((0, nc - 1, rng.randrange(nc))) if f & 32 else rng.randrange(nu), rng.randrange(nu), f)
                for f, d in zip(flags, dests)]

    for kind in (OP_MUL, OP_SQR):                         # every flag byte, in rounds of 32, 31 and the rest
        for chunk in _chunks(table_flags(), (32, 31)):
            for k, img in enumerate(imgs):
                dests = rng.sample(range(nu), len(chunk))    # operands may be other operations' destinations
                cases.append(Case(kind, mul_ops(chunk, dests), img, off=32 - len(chunk) if k == 1 else 0,
                                  tag=("flags", kind, chunk[0], k)))
    shape_chunks = _chunks(table_shapes(), (32, 31))       # every LIN shape, in rounds of 32 and 31
    assert len(shape_chunks) == 2
    shape_chunks[1] = (shape_chunks[1] + shape_chunks[0])[:31]
    for chunk in shape_chunks:
        for k, img in enumerate(imgs):
            dests = rng.sample(range(nu), len(chunk))
            ents = [lin_entry(d, [[rng.randrange(nu) for _ in range(n)] for n in shape]) for shape, d in zip(chunk, dests)]
            cases.append(Case(OP_LIN, ents, img, tag=("shapes", chunk[0], k)))
    a = mont(rng.randrange(1, P))
    b = mont(rng.randrange(1, P))
    for k, v in enumerate([None, None, (a, 0), (a + P, P), (0, b), (P, b + P), (_twin(a), _twin(b)), (2 * P - 1, 2 * P - 1)]):
        img = list(imgs[0])
        if v is not None:
            img[9] = v
        cases.append(Case(OP_INV, [inv_entry(3 + k, 9)], img, tag=("inv", k)))      # c1 = 0, c0 = 0, both representations
    for k, img in enumerate(imgs):                         # one operation a round
        cases.append(Case(OP_MUL, mul_ops([5], [7]), img, tag=("cnt 1", OP_MUL, k)))
        cases.append(Case(OP_SQR, mul_ops([15], [8]), img, off=31, tag=("cnt 1", OP_SQR, k)))
        cases.append(Case(OP_LIN, [lin_entry(0, [[1, 2], [3], [4, 5], [6]])], img, tag=("cnt 1", OP_LIN, k)))
    for k, img in enumerate(imgs[:2]):                     # operation 0 writes slot d; operations 1..31 read slot d
        d = 11
        others = [s for s in range(nu) if s != d]
        dests = rng.sample(others, 31)
        ents = [mul_entry(d, d, 0, 20, 0, 0)] + [mul_entry(t, d, d, (d, 21)[i & 1], d, (0, 5, 12, 15, 64, 1, 4)[i % 7])
                                                  for i, t in enumerate(dests)]
        cases.append(Case(OP_MUL, ents, img, tag=("alias", OP_MUL, k)))
        ents = [mul_entry(d, d, 0, 0, 0, 0)] + [mul_entry(t, d, d, 0, 0, (0, 1, 3)[i % 3]) for i, t in enumerate(dests)]
        cases.append(Case(OP_SQR, ents, img, tag=("alias", OP_SQR, k)))
        ents = [lin_entry(d, [[d, 1], [2], [d], [3]])] + [lin_entry(t, [[d], [d], [d, 4], [d]][:1 + i % 4] + [[]] * (3 - i % 4))
                                                           for i, t in enumerate(dests)]
        cases.append(Case(OP_LIN, ents, img, tag=("alias", OP_LIN, k)))
    for c in cases:
        round_model(c)                                      # (no two operations write one slot)
    _cache["round"] = cases
    return cases


def wide_cases():
    """a full-size image (the kernel's own slot count): the highest slots as destinations and operands"""
    if "wide" not in _cache:
        ns = programs()["full"][3]
        rng = random.Random("group-probe-wide")
        img = [(rng.randrange(2 * P), rng.randrange(2 * P)) for _ in range(ns)]
        hi = ns - 1
        _cache["wide"] = [Case(OP_MUL, [mul_entry(hi, hi - 1, hi - 2, 0, hi, 15), mul_entry(0, hi, 0, len(pool()) - 1, 0, 32)], img),
                          Case(OP_LIN, [lin_entry(hi - 3, [[hi], [hi - 1], [hi - 2], [0]])], img, off=5),
                          Case(OP_INV, [inv_entry(hi, hi - 5)], img)]
    return _cache["wide"]


def rotate_images(cases):
    """the same rounds, each on its neighbour's image (for the second of two launches)"""
    return [Case(c.kind, c.ents[c.off:c.off + c.cnt], cases[(i + 1) % len(cases)].image, off=c.off, tag=c.tag)
            for i, c in enumerate(cases)]


def run_round(call, cases, active, n_slots=ROUND_SLOTS):
    """call(n, n_slots, active, heads, ents, img) -> status; returns status, the images before and after
    (n, n_slots, 24): slots past a case's image hold poison"""
    import numpy as np
    n = len(cases)
    before = np.full((n, n_slots, 24), POISON, dtype=np.uint32)
    for i, c in enumerate(cases):
        assert len(c.image) <= n_slots
        for s, v in enumerate(c.image):
            before[i, s] = words(v[0]) + words(v[1])
    heads = np.array([c.head() for c in cases], dtype=np.uint32)
    ents = np.array([c.ent_words() for c in cases], dtype=np.uint32)
    assert ents.shape == (n, 128)
    act = np.array(active, dtype=np.uint8)
    after = before.copy()
    return call(n, n_slots, _p(act), _p(heads), _p(ents), _p(after)), before, after


def check_round(cases, active, before, after, mut=None):
    """written components: the model's residue, below 2p; every other word, the poison past the image included,
    bit-identical; a switched-off row untouched"""
    import numpy as np
    for i, c in enumerate(cases):
        if not active[i]:
            assert np.array_equal(before[i], after[i]), (i, c.tag, "an inactive row's image was written")
            continue
        writes = round_model(c, mut)
        for s in range(before.shape[1]):
            if s not in writes:
                assert np.array_equal(before[i, s], after[i, s]), (i, c.tag, "slot %d was written" % s)
                continue
            for h in (0, 1):
                got = val(after[i, s, 12 * h:12 * h + 12])
                assert got < 2 * P, (i, c.tag, s, h, "bound", hex(got))
                assert got % P == writes[s][h], (i, c.tag, s, h, "value", hex(got))


# --- k_group_fe -----------------------------------------------------------------------------------
def _f12(coeffs):
    """w-basis coefficients f_0..f_5 -> the oracle's tower element"""
    return o._f12_from_w(list(coeffs))


def golden_miller():
    """the Miller value of the first golden record (tests/golden/vectors.json), from the oracle"""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "vectors.json")) as f:
        c = json.load(f)["cases"][0]
    s, k = o.g1_from_compressed(bytes.fromhex(c["sig"])), o.g2_from_compressed(bytes.fromhex(c["pk"]))
    f = o.multi_miller_loop([(s, o._neg_g2_prepared()), (o.hash_to_g1(bytes.fromhex(c["msg"])), o.g2_prepare(k))])
    return f, bytes.fromhex(c["gt"])


def fe_rows():
    """(tag, f, twin, expected bytes, expected code); f = 0 is excluded: zero has no defined result (the program
    inverts f) and never reaches the kernel (a Miller value or a product of them is nonzero)"""
    if "fe" in _cache:
        return _cache["fe"]
    rng = random.Random("group-probe-fe")
    r2 = lambda: (rng.randrange(P), rng.randrange(P))      # noqa: E731
    z = (0, 0)
    vals = [("random %d" % k, _f12([r2() for _ in range(6)])) for k in range(3)]
    vals.append(("Fp", _f12([(rng.randrange(1, P), 0), z, z, z, z, z])))
    vals.append(("Fp2", _f12([r2(), z, z, z, z, z])))
    vals.append(("Fp6", _f12([r2(), z, r2(), z, r2(), z])))
    for k in range(6):
        w = [z] * 6
        w[k] = r2()
        vals.append(("sparse w^%d" % k, _f12(w)))
    vals.append(("coefficients 0, 1, p - 1", _f12([(0, 1), (P - 1, 0), (1, P - 1), (0, 0), (P - 1, P - 1), (1, 1)])))
    vals.append(("coefficients 1", _f12([(1, 1)] * 6)))
    vals.append(("one", o.F12_ONE))
    vals.append(("minus one", _f12([(P - 1, 0), z, z, z, z, z])))
    gm, gt = golden_miller()
    vals.append(("golden Miller value", gm))
    rows = []
    for tag, f in vals:
        assert f != (o.F6_ZERO, o.F6_ZERO)
        want = o.gt_to_bytes(o.final_exponentiation(f))
        if tag in ("Fp", "Fp2", "Fp6", "one", "minus one"):
            assert want == GT_ONE, tag
        if tag.startswith("golden"):
            assert want == gt
        for twin in (False, True):                          # every component as x, then as x + p
            rows.append((tag, f, twin, want, 0 if want == GT_ONE else 5))
    assert any(r[4] == 0 for r in rows) and any(r[4] == 5 for r in rows)
    _cache["fe"] = rows
    return rows


def pick(rows, n, shift=0):
    """n rows by rotation (a step coprime to the row count), so that neighbours differ and 65 rows meet every row"""
    import math
    step = next(s for s in (3, 5, 7, 11, 1) if math.gcd(s, len(rows)) == 1)
    return [rows[(shift + step * i) % len(rows)] for i in range(n)]


def fe_input(rows):
    """uint4 SoA of stride m: row 6 k + q of value i at [(6 k + q) m + i], store index k = 3 h + j = tower c_h.c_j"""
    import numpy as np
    m = len(rows)
    fin = np.zeros((36, m, 4), dtype=np.uint32)
    for i, (_, f, twin, _, _) in enumerate(rows):
        for h in range(2):
            for j in range(3):
                for c in range(2):
                    raw = mont(f[h][j][c]) + (P if twin else 0)
                    fin[6 * (3 * h + j) + 3 * c:6 * (3 * h + j) + 3 * c + 3, i, :] = np.array(words(raw), dtype=np.uint32).reshape(3, 4)
    return fin


def run_fe(call, rows):
    import numpy as np
    m = len(rows)
    fin = fe_input(rows)
    code = np.full(m, 0xEE, dtype=np.uint8)
    gt = np.full((m, 576), 0xEE, dtype=np.uint8)
    return call(m, _p(fin), _p(code), _p(gt)), code, gt


def check_fe(rows, code, gt):
    for i, (tag, _, twin, want, wcode) in enumerate(rows):
        assert bytes(gt[i]) == want, ("group_fe", i, tag, twin, "Gt bytes")
        assert int(code[i]) == wcode, ("group_fe", i, tag, twin, "code", int(code[i]))


# --- k_group ----------------------------------------------------------------------------------------
class Rec:
    """one record of k_group: the decode codes and identity flags, the affine values (raw), what must come out"""

    def __init__(self, tag, sig, h, pk, inf=0, code=0, code2=0, want_code=0, want_gt=None):
        self.tag, self.sig, self.h, self.pk, self.inf = tag, sig, h, pk, inf
        self.code, self.code2, self.want_code, self.want_gt = code, code2, want_code, want_gt


def _m1(pt, twin=False):
    return tuple(mont(c) + (P if twin else 0) for c in pt)


def _m2(pt, twin=False):
    return tuple((mont(c[0]) + (P if twin else 0), mont(c[1]) + (P if twin else 0)) for c in pt)


def simulate_group(inp):
    """gen_group.simulate() of the full program on integer inputs -> (outputs, the INV operands met)"""
    m = gen()
    g, rounds, slot, nslots, _, _ = programs()["full"]
    seen, real = [], m.f2inv

    def spy(a):
        seen.append(a)
        return real(a) if a != (0, 0) else (0, 0)
    m.f2inv = spy
    try:
        out = m.simulate(g, rounds, slot, nslots, inp)
    finally:
        m.f2inv = real
    return out, seen


def _tower_bytes(out):
    return b"".join(out["gt%d" % (2 * j + h)][c].to_bytes(48, "big") for h in range(2) for j in range(3) for c in range(2))


def group_recs():
    if "group" in _cache:
        return _cache["group"]
    rng = random.Random("group-probe-group")
    junk1 = lambda: (rng.randrange(2 * P), rng.randrange(2 * P))      # noqa: E731
    recs = []
    # (a) real records, Gt and code from the oracle
    sk = rng.randrange(1, o.R)
    msg, other = b"lane-group probe", b"another message"
    pk = o.g2_from_compressed(o.public_key(sk))
    sig = o.g1_from_compressed(o.sign(sk, msg))
    gen2 = _m2(o.G2_GEN)             # the key decode keeps the generator for an identity key
    for tag, s, mm, k, twin in (("valid", sig, msg, pk, False), ("valid, x + p", sig, msg, pk, True), ("forged", sig, other, pk, False),
                                ("identity signature", None, msg, pk, False), ("identity key", sig, msg, None, False),
                                ("(O, O)", None, msg, None, False)):
        gt = o.verify_gt(s, mm, k)
        inf = (INF_SIG if s is None else 0) | (INF_PK if k is None else 0)
        recs.append(Rec(tag, _m1(s, twin) if s else junk1(), _m1(o.hash_to_g1(mm), twin), _m2(k, twin) if k else gen2, inf,
                        want_code=0 if gt == o.F12_ONE else 5, want_gt=o.gt_to_bytes(gt)))
    assert [r.want_code for r in recs] == [0, 0, 5, 5, 5, 0], [r.want_code for r in recs]
    # (b) arbitrary field values for the points, INF_PK set (no subgroup check: the Gt bytes are written);
    # (c) the same with INF_PK clear: the subgroup compare on lazily reduced values says code 4, no Gt bytes
    rf = lambda: rng.randrange(P)      # noqa: E731
    cands = [("random", (rf(), rf()), ((rf(), rf()), (rf(), rf()))),
             ("random 2", (rf(), rf()), ((rf(), rf()), (rf(), rf()))),
             ("sig 0", (0, 0), ((rf(), rf()), (rf(), rf()))),
             ("ones", (1, 1), ((1, 0), (1, 0))),
             ("p - 1", (P - 1, P - 1), ((P - 1, P - 1), (P - 1, P - 1))),
             ("key in Fp", (rf(), 1), ((rf(), 0), (rf(), 0))),
             ("key (u, 1)", (P - 1, rf()), ((0, 1), (1, 0))),
             ("key x = 0", (rf(), 0), ((0, 0), (rf(), rf())))]
    kept = 0
    for tag, s, q in cands:
        inp = {"p0x": (s[0], 0), "p0y": (s[1], 0), "p1x": (0, 0), "p1y": (0, 0), "qx": q[0], "qy": q[1], "one": (1, 0)}
        out, invs = simulate_group(inp)
        assert len(invs) == 1                               # the program's single INV
        if invs[0] == (0, 0):
            continue                                        # the inverse of zero is not defined: not a row
        kept += 1
        gt = _tower_bytes(out)
        passes = out["tz"] != (0, 0) and out["pzx"] == out["tx"] and out["pzy"] == gen().f2neg(out["ty"])
        assert not passes, tag                              # not a G2 point: psi(Q) != -[|x|]Q
        for twin in (False, True):
            t = tag + (", x + p" if twin else "")
            recs.append(Rec("values: " + t, _m1(s, twin), junk1(), _m2(q, twin), INF_PK, want_code=0 if gt == GT_ONE else 5, want_gt=gt))
            recs.append(Rec("not in G2: " + t, _m1(s, twin), _m1((rf(), rf())), _m2(q, twin), 0, want_code=4))
    assert kept >= 6, kept
    # decode codes: the signature's first, from either array; nothing else is written
    for code, code2, want in ((2, 0, 2), (0, 4, 4), (2, 4, 2), (1, 3, 1)):
        recs.append(Rec("decode codes %d, %d" % (code, code2), junk1(), junk1(), gen2, 0, code, code2, want))
    _cache["group"] = recs
    return recs


def run_group(call, recs, split, alias):
    """call(n, stride, code, inf, code2, inf2, sig, h, pk, alias, code_out, gt_out) -> status.  split: the key's
    code and identity flag travel in code2 / inf2 (else those are null and a record's code2 moves to code)"""
    import numpy as np
    n = len(recs)
    stride = n + 7
    rng = random.Random("group-probe-pad")
    sig = np.array([rng.getrandbits(32) for _ in range(24 * stride)], dtype=np.uint32).reshape(24, stride)
    h = sig[::-1].copy()
    pk = np.array([rng.getrandbits(32) for _ in range(48 * stride)], dtype=np.uint32).reshape(48, stride)
    code, inf, code2, inf2 = (np.zeros(n, dtype=np.uint8) for _ in range(4))
    for i, r in enumerate(recs):
        sig[:, i] = words(r.sig[0]) + words(r.sig[1])
        h[:, i] = words(r.h[0]) + words(r.h[1])
        pk[:, i] = words(r.pk[0][0]) + words(r.pk[0][1]) + words(r.pk[1][0]) + words(r.pk[1][1])
        if split:
            code[i], code2[i], inf[i], inf2[i] = r.code, r.code2, r.inf & INF_SIG, r.inf & INF_PK
        else:
            code[i], inf[i] = r.code or r.code2, r.inf
    out = np.full(n, 0xEE, dtype=np.uint8)
    gt = np.full((n, 576), 0xEE, dtype=np.uint8)
    status = call(n, stride, _p(code), _p(inf), _p(code2) if split else None, _p(inf2) if split else None, _p(sig), _p(h), _p(pk),
                  1 if alias else 0, _p(out), _p(gt))
    return status, out, gt


def check_group(recs, split, out, gt):
    for i, r in enumerate(recs):
        assert int(out[i]) == r.want_code, ("group", i, r.tag, "code", int(out[i]))
        if r.want_gt is None:
            assert (gt[i] == 0xEE).all(), ("group", i, r.tag, "Gt bytes were written")
        else:
            assert bytes(gt[i]) == r.want_gt, ("group", i, r.tag, "Gt bytes")
