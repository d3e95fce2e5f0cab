"""Integer model of the lane-pair primitives (cess_amd/csrc/bls/pair.hpp,
bls/pair_fe.hpp) for tests/test_gpu_pair_primitives.py (the GPU comparison)
and tests/test_pair_probe_model.py (the same tables checked with no device).

Everything here is plain Python integers mod p; the tower operations are the
oracle's (oracle/bls_oracle.py).  The kernels hold an Fp value x as raw limbs
`raw` with raw = x R (mod p), R = 2^392, anywhere in the operation's documented
range (stored values < 2p, product operands < 2^384), so a value has several
valid representations: res(raw) = raw / R mod p is the residue a raw value
stands for, and every expectation is a residue.

An operation (`Op`) has
  n_in / n_out  Fp2 operands / results per pair (as tests/probe/pair_probe.hip),
  in_bound      exclusive bound of every operand component (the contract),
  out_bound     exclusive bound of every result component (the postcondition),
  cases         the operand table: per pair a list of n_in (raw0, raw1),
  ref(xs)       the expected residues, from the operands' residues,
  exact(case)   (optional) the expected raw limbs where the header fixes them,
  pred          True if the result is a predicate (one word per lane).
Store layout (staged.hpp): store index k = 3 h + j holds the coefficient
c_h.c_j of the oracle's Fp12 ((c00, c01, c02), (c10, c11, c12)); in Karabina's
naming z0 = 0, z4 = 1, z3 = 2, z2 = 3, z1 = 4, z5 = 5; component c of an Fp2 is
on lane c of the pair.
"""
import random

import oracle.bls_oracle as o

P = o.P
R = 1 << 392
RINV = pow(R, -1, P)
ONE = R % P                     # the Montgomery one (c::ONE)
TOP = (1 << 384) - 1
PAIR_COUNTS = (1, 33, 161)      # one pair; a wave and one pair; two blocks
POISON = 0xDEADBEEF


def res(raw):
    return raw * RINV % P


def mont(x):
    return x * R % P


def res2(a):
    return (res(a[0]), res(a[1]))


def mont2(a):
    return (mont(a[0]), mont(a[1]))


# --- operand classes ----------------------------------------------------------
# stored values: < 2p
STORED_EDGES = [0, 1, P - 1, P, P + 1, 2 * P - 1, ONE, ONE + P, (1 << 380) - 1, (1 << 381) - 1,
                3 * (1 << 380) - 1, (1 << 381) - (1 << 64), 2 * P - (1 << 96)]
# product operands: < 2^384 (the edge list of test_hostemu.py test_fp2_mul_lazy_bounds on top)
PRODUCT_EDGES = STORED_EDGES + [2 * P, 4 * P - 1, 6 * P - 1, 8 * P - 1, TOP, TOP - 1, 1 << 383, (1 << 364) - 1]
assert all(0 <= v < 2 * P for v in STORED_EDGES) and all(0 <= v <= TOP for v in PRODUCT_EDGES)


def _draw(rng, edges, bound, p_edge=0.45):
    return rng.choice(edges) if rng.random() < p_edge else rng.randrange(bound)


def _twin(v):
    """the other representation of the same residue among the stored values"""
    return v + P if v < P else v - P


def _separate(cases):
    """neighbouring pairs must hold different operands (a permute that reads
    the other pair of the quad must change the result)"""
    out = []
    for c in cases:
        if out and out[-1] == c:
            continue
        out.append(c)
    for a, b in zip(out, out[1:]):
        assert a != b
    return out


def fp2_table(n_ops, edges, bound, seed, explicit=(), n_edge=260, n_rand=120):
    """cases of n_ops Fp2 operands: `explicit` first, then the full product
    edges x edges (one operand) or per-component draws from `edges`, then
    random values below `bound`, in a fixed shuffled order"""
    rng = random.Random(seed)
    body = []
    if n_ops == 1:
        body += [[(a, b)] for a in edges for b in edges]
    else:
        body += [[(rng.choice(edges), rng.choice(edges)) for _ in range(n_ops)] for _ in range(n_edge)]
    body += [[(_draw(rng, edges, bound, 0.25), _draw(rng, edges, bound, 0.25)) for _ in range(n_ops)]
             for _ in range(n_rand)]
    rng.shuffle(body)
    return _separate([list(c) for c in explicit] + body)


def tower_table(n_ops, seed, n=PAIR_COUNTS[-1], explicit=()):
    """n cases of n_ops stored Fp2 values with the edge classes spread over
    them: uniform edge cases first, then per-component draws; every eighth
    case repeats its predecessor's residues in the other representation (x and
    x + p must give congruent results)"""
    rng = random.Random(seed)
    cases = [list(c) for c in explicit]
    for v in (2 * P - 1, 0, P, ONE + P, (1 << 381) - 1):
        cases.append([(v, v)] * n_ops)
    cases.append([(0, P) if i & 1 else (P, 0) for i in range(n_ops)])
    cases.append([(2 * P - 1, 0) if i & 1 else (0, 2 * P - 1) for i in range(n_ops)])
    while len(cases) < n:
        if len(cases) % 8 == 7:
            cases.append([(_twin(a), _twin(b)) for a, b in cases[-1]])
            continue
        pe = rng.choice((0.0, 0.3, 0.8))
        cases.append([(_draw(rng, STORED_EDGES, 2 * P, pe), _draw(rng, STORED_EDGES, 2 * P, pe))
                      for _ in range(n_ops)])
    return _separate(cases)[:n]


def with_twins(cases, every=3):
    """append, for every `every`-th case, the same residues in the other
    representation (x and x + p must give congruent results)"""
    tw = [[(_twin(a), _twin(b)) for a, b in c] for c in cases[::every]]
    return _separate(cases + tw)


# --- the oracle's Fp12 <-> store order ----------------------------------------
def to_store(f):
    """oracle Fp12 -> list of 6 Fp2 by store index"""
    return [f[0][0], f[0][1], f[0][2], f[1][0], f[1][1], f[1][2]]


def from_store(s):
    return ((s[0], s[1], s[2]), (s[3], s[4], s[5]))


def store_to_gt_bytes(store_raw):
    """k_final2's Gt output of an accumulator image: lane h of the pair writes
    Fp 2k + h (tower order) of store index k, canonical, big-endian"""
    out = bytearray(576)
    for k in range(6):
        for h in range(2):
            out[96 * k + 48 * h:96 * k + 48 * h + 48] = res(store_raw[k][h]).to_bytes(48, "big")
    return bytes(out)


Z_INDEX = {"z0": 0, "z4": 1, "z3": 2, "z2": 3, "z1": 4, "z5": 5}
# pkcyc_run_ps: (u, w) per lane as store indices -- lane 0 (z4, z5), lane 1 (z3, z2)
PS_LANE_UW = ((Z_INDEX["z4"], Z_INDEX["z5"]), (Z_INDEX["z3"], Z_INDEX["z2"]))


# --- Karabina compressed squaring and decompression, as formulas --------------
def f2_muli(a, k):
    return (a[0] * k % P, a[1] * k % P)


def kcyc_square(z2, z3, z4, z5):
    """one compressed squaring (eprint 2010/542) of (z2, z3, z4, z5)"""
    n2 = f2_muli(o.f2_add(z2, f2_muli(o.f2_mul_nr(o.f2_mul(z4, z5)), 3)), 2)
    n3 = o.f2_sub(f2_muli(o.f2_add(o.f2_sqr(z4), o.f2_mul_nr(o.f2_sqr(z5))), 3), f2_muli(z3, 2))
    n4 = o.f2_sub(f2_muli(o.f2_add(o.f2_sqr(z2), o.f2_mul_nr(o.f2_sqr(z3))), 3), f2_muli(z4, 2))
    n5 = f2_muli(o.f2_add(z5, f2_muli(o.f2_mul(z2, z3), 3)), 2)
    return n2, n3, n4, n5


def f2_is_zero(a):
    return a[0] % P == 0 and a[1] % P == 0


def z1_frac(z2, z3, z4, z5):
    """numerator and denominator of z1 (staged.hpp cyc_z1_frac)"""
    if f2_is_zero(z2):
        return f2_muli(o.f2_mul(z4, z5), 2), z3
    num = o.f2_sub(o.f2_add(o.f2_mul_nr(o.f2_sqr(z5)), f2_muli(o.f2_sqr(z4), 3)), f2_muli(z3, 2))
    return num, f2_muli(z2, 4)


def z1_den(z2, z3):
    return z3 if f2_is_zero(z2) else f2_muli(z2, 4)


def z0_of(z1, z2, z3, z4, z5):
    t = o.f2_add(f2_muli(o.f2_sqr(z1), 2), o.f2_sub(o.f2_mul(z2, z5), f2_muli(o.f2_mul(z3, z4), 3)))
    return o.f2_add(o.f2_mul_nr(t), o.F2_ONE)


def kcyc_decompress(z2, z3, z4, z5):
    """the cyclotomic Fp12 with the given (z2, z3, z4, z5), or None if
    z2 = z3 = 0 (not decompressible)"""
    num, den = z1_frac(z2, z3, z4, z5)
    if f2_is_zero(den):
        return None
    z1 = o.f2_mul(num, o.f2_inv(den))
    z0 = z0_of(z1, z2, z3, z4, z5)
    return from_store([z0, z4, z3, z2, z1, z5])


def f12_frob_k(a, k):
    for _ in range(k):
        a = o.f12_frob(a)
    return a


def easy_part(f):
    """f^((p^6 - 1)(p^2 + 1)): an element of the cyclotomic subgroup"""
    m = o.f12_mul(o.f12_conj(f), o.f12_inv(f))
    return o.f12_mul(f12_frob_k(m, 2), m)


# --- cyclotomic operands and their powers (computed once, shared) -------------
N_CYC = PAIR_COUNTS[-1]
CYC_POWERS = (1, 2, 16, 48, 57)
_cyc_cache = {}


def cyc_elements():
    """N_CYC cyclotomic elements (the easy part of random Fp12 values), with
    the element 1 at a few places (FE_CHAIN's degenerate path)"""
    if "el" not in _cyc_cache:
        rng = random.Random(1201)
        el = []
        for i in range(N_CYC):
            if i in (2, 5, 32, 40, 129, 160):
                el.append(o.F12_ONE)
                continue
            f = from_store([(rng.randrange(P), rng.randrange(P)) for _ in range(6)])
            el.append(easy_part(f))
        _cyc_cache["el"] = el
    return _cyc_cache["el"]


def cyc_powers():
    """per element: {n: a^(2^n)} for n in CYC_POWERS, by repeated f12_sqr"""
    if "pw" not in _cyc_cache:
        pw = []
        for a in cyc_elements():
            d, t = {}, a
            for n in range(1, CYC_POWERS[-1] + 1):
                t = o.F12_ONE if a == o.F12_ONE else o.f12_sqr(t)
                if n in CYC_POWERS:
                    d[n] = t
            pw.append(d)
        _cyc_cache["pw"] = pw
    return _cyc_cache["pw"]


def cyc_cases(idx=range(6)):
    """raw operands of the cyclotomic elements (store indices idx), half of the
    components in the representation + p, the zeros of the element 1 as 0 or p"""
    rng = random.Random(1202)
    cases = []
    for a in cyc_elements():
        s = to_store(a)
        c = []
        for k in idx:
            raw = [mont(s[k][0]), mont(s[k][1])]
            for h in range(2):
                if rng.random() < 0.5:
                    raw[h] += P
            c.append(tuple(raw))
        cases.append(c)
    return _separate(cases)


# --- operations ---------------------------------------------------------------
class Op:
    def __init__(self, name, n_in, n_out, cases, ref=None, in_bound=2 * P, out_bound=2 * P, exact=None, pred=False,
                 arg=0, entry=None, full_table=False):
        self.name, self.n_in, self.n_out, self.cases = name, n_in, n_out, cases
        self.ref, self.exact, self.pred, self.arg = ref, exact, pred, arg
        self.in_bound, self.out_bound = in_bound, out_bound
        self.entry = entry or name          # the probe's entry point pp_<entry>
        self.full_table = full_table        # a cheap Fp2 operation: also run on the whole table
        self._expected = None

    def bound_in(self, v):
        b = self.in_bound
        return b[v] if isinstance(b, (list, tuple)) else b

    def check_contract(self):
        """every operand within the operation's documented bound, neighbours differ"""
        assert len(self.cases) >= PAIR_COUNTS[-1], (self.name, len(self.cases))
        for i, c in enumerate(self.cases):
            assert len(c) == self.n_in, (self.name, i)
            for v, (a, b) in enumerate(c):
                assert 0 <= a < self.bound_in(v) and 0 <= b < self.bound_in(v), (self.name, i, v)
            if self.n_in and i:
                assert c != self.cases[i - 1], (self.name, i)

    def expected(self):
        """per case: the expected residues (list of n_out Fp2), or the
        predicate's truth value"""
        if self._expected is None:
            exp = []
            for i, c in enumerate(self.cases):
                exp.append(self.ref([res2(x) for x in c], i) if self.ref else None)
            self._expected = exp
        return self._expected


def _f6(xs):
    return (xs[0], xs[1], xs[2])


def _f12(xs):
    return from_store(xs[:6])


def _pred_cases_is_one():
    rng = random.Random(1301)
    one_reps = [[(ONE, 0)] + [(0, 0)] * 5, [(ONE + P, P)] + [(0, 0)] * 5,
                [(ONE + P, P)] + [(P, 0), (0, P), (P, P), (0, 0), (P, P)], [(ONE, P)] + [(P, P)] * 5]
    cases = []
    while len(cases) < N_CYC:
        base = [list(x) for x in rng.choice(one_reps)]
        kind = len(cases) % 3
        if kind == 1:      # one component off
            k, h = rng.randrange(6), rng.randrange(2)
            off = [0, P, ONE + 1, 1] if (k, h) == (0, 0) else [1, P + 1, P - 1, 2 * P - 1, ONE]
            base[k][h] = rng.choice(off)
        elif kind == 2:    # unrelated
            base = [[rng.randrange(2 * P), rng.randrange(2 * P)] for _ in range(6)]
        cases.append([tuple(x) for x in base])
    return _separate(cases)


def _pred_cases_is_conj():
    rng = random.Random(1302)
    cases = []
    while len(cases) < N_CYC:
        kind = len(cases) % 3
        # b with coefficients 0 in either representation
        b = [(_draw(rng, [0, P], 2 * P, 0.4), _draw(rng, [0, P], 2 * P, 0.4)) for _ in range(6)]
        a = []
        for k in range(6):
            c = []
            for h in range(2):
                v = b[k][h] if k < 3 or b[k][h] == 0 else 2 * P - b[k][h]     # conj: the w half negated
                c.append(_twin(v) if rng.random() < 0.5 else v)
            a.append(c)
        if kind == 1:
            k, h = rng.randrange(6), rng.randrange(2)
            a[k][h] = (a[k][h] + 1) % (2 * P)
        elif kind == 2:
            a = [[rng.randrange(2 * P), rng.randrange(2 * P)] for _ in range(6)]
        cases.append([tuple(x) for x in a] + b)
    return _separate(cases)


def _cases_eq():
    rng = random.Random(1303)
    cases = []
    firsts = [(x, y) for x in STORED_EDGES for y in STORED_EDGES]
    firsts += [(rng.randrange(2 * P), rng.randrange(2 * P)) for _ in range(60)]
    for a in firsts:
        kind = len(cases) % 4
        if kind == 0:
            b = a
        elif kind == 1:
            b = (_twin(a[0]), _twin(a[1]))
        elif kind == 2:
            b = (_twin(a[0]), (a[1] + 1) % (2 * P))
        else:
            b = ((a[0] + P - 1) % (2 * P), a[1])
        cases.append([a, b])
    rng.shuffle(cases)
    return _separate(cases)


def _cases_z1(n_ops):
    """(z2, z3[, z4, z5]): z2 a zero class with z3 != 0; z2 = z3 = 0; general"""
    rng = random.Random(1304 + n_ops)
    zc = [(0, 0), (0, P), (P, 0), (P, P)]
    cases = []
    while len(cases) < N_CYC:
        kind = len(cases) % 3
        c = [(_draw(rng, STORED_EDGES, 2 * P, 0.3), _draw(rng, STORED_EDGES, 2 * P, 0.3)) for _ in range(n_ops)]
        if kind == 0:
            c[0] = zc[(len(cases) // 3) % 4]
            while f2_is_zero(res2(c[1])):
                c[1] = (rng.randrange(2 * P), rng.randrange(2 * P))
        elif kind == 1:
            c[0] = zc[(len(cases) // 3) % 4]
            c[1] = zc[(len(cases) // 12) % 4]
        cases.append(c)
    return _separate(cases)


def _ref_pkcyc(n):
    def ref(xs, i):
        s = to_store(cyc_powers()[i][n])
        return [s[Z_INDEX["z2"]], s[Z_INDEX["z3"]], s[Z_INDEX["z4"]], s[Z_INDEX["z5"]]]
    return ref


def _ref_chain(xs, i):
    pw = cyc_powers()[i]
    return to_store(pw[16]) + to_store(pw[48]) + to_store(pw[57])


def build_ops():
    S, PR = STORED_EDGES, PRODUCT_EDGES
    top_combos2 = [[(TOP, TOP), (TOP, TOP)], [(TOP, 0), (TOP, TOP)], [(0, TOP), (TOP, TOP)], [(TOP, TOP), (TOP, 0)],
                   [(TOP, TOP), (0, TOP)], [(0, TOP), (0, TOP)], [(TOP, 0), (0, TOP)]]
    top_combos4 = [a + b for a in top_combos2[:4] for b in top_combos2[:4]]
    # a1 = 0 / a0 = 0 in both representations: partner_signed's 2p summand
    nr_first = [[(a, b)] for a, b in ((2 * P - 1, 0), (0, 2 * P - 1), (2 * P - 1, P), (P, 2 * P - 1), (0, 0), (P, P))]
    ops = []

    def add(*a, **k):
        ops.append(Op(*a, **k))

    t1 = fp2_table(1, S, 2 * P, 1101, explicit=nr_first)
    add("xchg", 1, 1, t1, lambda x, i: [(x[0][1], x[0][0])], exact=lambda c: [(c[0][1], c[0][0])], full_table=True)
    add("partner_signed", 1, 1, t1, lambda x, i: [((-x[0][1]) % P, x[0][0])], out_bound=2 * P + 1, full_table=True)
    add("mul_nr", 1, 1, t1, lambda x, i: [o.f2_mul_nr(x[0])], full_table=True)
    add("mul_nr_nr", 1, 1, t1, lambda x, i: [o.f2_mul_nr(x[0])], out_bound=4 * P, full_table=True)
    txi = fp2_table(2, S, 2 * P, 1102, explicit=[[(2 * P - 1, 2 * P - 1), (2 * P - 1, 0)], [(0, 0), (0, P)]])
    add("add_xi_nr", 2, 1, txi, lambda x, i: [o.f2_add(x[0], o.f2_mul_nr(x[1]))], out_bound=6 * P, full_table=True)
    add("conj", 1, 1, t1, lambda x, i: [o.f2_conj(x[0])], full_table=True)
    add("fph_one", 0, 1, [[] for _ in range(PAIR_COUNTS[-1])], lambda x, i: [o.F2_ONE], exact=lambda c: [(ONE, 0)])
    add("is_zero", 1, 1, t1, lambda x, i: f2_is_zero(x[0]), pred=True, full_table=True)
    add("eq", 2, 1, _cases_eq(), lambda x, i: x[0] == x[1], pred=True, full_table=True)
    tp2 = fp2_table(2, PR, TOP + 1, 1103, explicit=top_combos2)
    for s in (1, 2, 3):
        add("pmul_scaled%d" % s, 2, 1, tp2, (lambda s: lambda x, i: [f2_muli(o.f2_mul(x[0], x[1]), s)])(s),
            in_bound=TOP + 1, full_table=True)
    add("psqr", 1, 1, with_twins(t1), lambda x, i: [o.f2_sqr(x[0])], full_table=True)
    tp4 = fp2_table(4, PR, TOP + 1, 1104, explicit=top_combos4)
    add("pdot2", 4, 1, tp4, lambda x, i: [o.f2_add(o.f2_mul(x[0], x[1]), o.f2_mul(x[2], x[3]))], in_bound=TOP + 1,
        full_table=True)
    add("pmul_fp", 2, 1, fp2_table(2, S, 2 * P, 1105), lambda x, i: [o.f2_muls(x[0], x[1][0])], full_table=True)
    add("pinv", 1, 1, with_twins(t1), lambda x, i: [o.f2_inv(x[0])], full_table=True)
    add("pmul_p", 2, 1, tp2, lambda x, i: [o.f2_mul(x[0], x[1])], in_bound=TOP + 1, full_table=True)
    add("pdot2_p", 4, 1, tp4, lambda x, i: [o.f2_add(o.f2_mul(x[0], x[1]), o.f2_mul(x[2], x[3]))], in_bound=TOP + 1,
        full_table=True)

    add("pmul6", 6, 3, tower_table(6, 1110), lambda x, i: list(o.f6_mul(_f6(x), _f6(x[3:]))))
    add("pmul_by_1", 4, 3, tower_table(4, 1111), lambda x, i: list(o.f6_mul(_f6(x), (o.F2_ZERO, x[3], o.F2_ZERO))))
    add("pmul_by_01_one", 4, 3, tower_table(4, 1112), lambda x, i: list(o.f6_mul(_f6(x), (o.F2_ONE, x[3], o.F2_ZERO))))
    add("psqr12", 6, 6, tower_table(6, 1113), lambda x, i: to_store(o.f12_sqr(_f12(x))))
    add("pmul014", 9, 6, tower_table(9, 1114), lambda x, i: to_store(o.f12_mul_by_014(_f12(x), x[6], x[7], x[8])))
    add("pmul014_one", 8, 6, tower_table(8, 1115), lambda x, i: to_store(o.f12_mul_by_014(_f12(x), o.F2_ONE, x[6], x[7])))
    add("pmul12", 12, 6, tower_table(12, 1116), lambda x, i: to_store(o.f12_mul(_f12(x), _f12(x[6:]))))
    add("pinv12", 6, 6, tower_table(6, 1117), lambda x, i: to_store(o.f12_inv(_f12(x))))
    for k in (1, 2, 3):
        add("pfrob12_k%d" % k, 6, 6, tower_table(6, 1118), (lambda k: lambda x, i: to_store(f12_frob_k(_f12(x), k)))(k),
            arg=k, entry="pfrob12")
    add("pfp4_square", 2, 2, fp2_table(2, S, 2 * P, 1119, explicit=[[(2 * P - 1, 2 * P - 1), (2 * P - 1, 0)]]),
        lambda x, i: [o.f2_add(o.f2_sqr(x[0]), o.f2_mul_nr(o.f2_sqr(x[1]))), f2_muli(o.f2_mul(x[0], x[1]), 2)],
        full_table=True)
    cyc6 = cyc_cases()
    cyc4 = cyc_cases([Z_INDEX["z2"], Z_INDEX["z3"], Z_INDEX["z4"], Z_INDEX["z5"]])
    for n in (1, 2, 16):
        add("pcyc_square_run_n%d" % n, 6, 6, cyc6, (lambda n: lambda x, i: to_store(cyc_powers()[i][n]))(n), arg=n,
            entry="pcyc_square_run")
        add("pkcyc_run_ps_n%d" % n, 4, 4, cyc4, _ref_pkcyc(n), arg=n, entry="pkcyc_run_ps")
    add("pcyc_z1_frac", 4, 2, _cases_z1(4), lambda x, i: list(z1_frac(*x)))
    add("pcyc_z1_den", 2, 1, _cases_z1(2), lambda x, i: [z1_den(*x)])
    add("pcyc_z0", 5, 1, tower_table(5, 1120), lambda x, i: [z0_of(*x)])
    add("pcyc_chain", 6, 18, cyc6, _ref_chain)
    add("pis_one12_lds", 6, 1, _pred_cases_is_one(), lambda x, i: _f12(x) == o.F12_ONE, pred=True, arg=0, entry="pis_one12")
    add("pis_one12_slot", 6, 1, _pred_cases_is_one(), lambda x, i: _f12(x) == o.F12_ONE, pred=True, arg=1, entry="pis_one12")
    add("pis_conj12", 12, 1, _pred_cases_is_conj(), lambda x, i: _f12(x) == o.f12_conj(_f12(x[6:])), pred=True)
    rt = tower_table(6, 1121)
    add("glob_roundtrip", 6, 12, rt, lambda x, i: x[:6] + x[:6], exact=lambda c: list(c) + list(c))
    return ops


_ops_cache = []


def ops():
    if not _ops_cache:
        _ops_cache.extend(build_ops())
    return _ops_cache


def op_names():
    return [op.name for op in ops()]


def get_op(name):
    return next(op for op in ops() if op.name == name)


def active_mask(n, half):
    """all pairs live, or one live and one dead pair in every quad: pairs with
    i mod 4 in {1, 2} switched off"""
    return [0 if half and i % 4 in (1, 2) else 1 for i in range(n)]


def check_result(op, i, got, case=None):
    """got: the n_out (raw0, raw1) results of case i (or the two lanes' words
    of a predicate).  Asserts range, lane agreement, residue and exact limbs."""
    exp = op.expected()[i]
    if op.pred:
        assert got[0][0] == got[0][1], (op.name, i, "lanes disagree", got[0])
        assert got[0][0] in (0, 1), (op.name, i, got[0])
        assert bool(got[0][0]) == bool(exp), (op.name, i, "predicate", got[0][0], exp)
        return
    for v in range(op.n_out):
        for h in range(2):
            g = got[v][h]
            assert 0 <= g < op.out_bound, (op.name, i, v, h, "out of range", hex(g))
            assert res(g) == exp[v][h] % P, (op.name, i, v, h, "residue", hex(g))
    if op.exact:
        want = op.exact(op.cases[i])
        assert [tuple(x) for x in got] == [tuple(x) for x in want], (op.name, i, "limbs")


def model_result(op, i):
    """the reference's result reduced into the promised range, as the raw limbs
    a correct kernel may return (the canonical representative)"""
    exp = op.expected()[i]
    if op.pred:
        return [(int(bool(exp)), int(bool(exp)))]
    if op.exact:
        return [tuple(x) for x in op.exact(op.cases[i])]
    return [(mont(e[0]), mont(e[1])) for e in exp]
