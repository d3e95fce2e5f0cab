"""Operand tables and integer references of the Ed25519 primitives
(cess_amd/csrc/ed25519.hpp), one operation per probe entry
(tests/probe/ed25519_probe.hip), shared by the host build
(tests/test_ed25519_primitives.py) and the GPU probe
(tests/test_gpu_ed25519_primitives.py).

Plain Python integers and tests/ed25519_model.py; nothing is taken from the
code under test.  One lane takes n_in words and returns n_out words:

  fe_mul, fe_add, fe_sub            a, b (10 limbs each) -> 10 limbs
  fe_sqr, fe_neg, fe_carry, fe_neg_tight, fe_invert, fe_pow22523
                                    a -> 10 limbs
  fe_from_words                     8 words -> 10 limbs
  fe_to_words                       a -> 8 words, fe_is_zero, fe_is_negative
  sc_lt_L                           8 words -> 1
  sc_reduce512                      16 words -> 8 words
  sc_digits                         8 words -> sc_recode, then 64 x (sc_top_digit + 8)
  ge_decode                         8 words -> flag, x, y
  ge_dbl                            X, Y, Z -> E, H, G, F, then ge_finish's X, Y, Z, T
  ge_madd                           X, Y, Z, T, entry (y + x, y - x, 2 d x y) -> the same eight
  ge_pre_digit                      table index, digit + 8 -> the entry's three fields
  key_table                         length, 8 words of key bytes -> status, 240 words
  verify_equation                   table index of the key, of the base point, S, h, R (8 words each) -> 0 / 1

Bounds (ed25519.hpp): tight = even limbs <= 2^26 + 2^12, odd <= 2^25 + 2^16;
loose = twice that; input = even < 13 * 2^24, odd < 13 * 2^23.

The field rows hold non-canonical encodings of k p + d for |d| <= 20.  Limbs
within the input bound sum to less than 3.26 * 2^255, so k = 0..3 go to every
operation and k = 4..6 (wide_rows) only where wider limbs are allowed: to
fe_carry (limbs < 2^32 - 2^7) and as fe_sub's first operand.  fe_add and
fe_neg_tight take the tight rows alone, as their contracts say.
"""
import random

import ed25519_model as model

P, L, D = model.P, model.L, model.D
C = L - 2**252
POISON = 0xDEADBEEF
LANE_COUNTS = (1, 65, 257)        # one lane; a wave and a lane; a block and a lane
BITS = [26, 25] * 5
WEIGHT = [sum(BITS[:k]) for k in range(10)]
MASK = [(1 << b) - 1 for b in BITS]
TIGHT = [2**25 + 2**16 if k & 1 else 2**26 + 2**12 for k in range(10)]
LOOSE = [2 * t for t in TIGHT]
INPUT = [13 * 2**23 - 1 if k & 1 else 13 * 2**24 - 1 for k in range(10)]
P2 = [2**27 - 38] + [2**26 - 2 if k & 1 else 2**27 - 2 for k in range(1, 10)]     # the limbs of 2p
TABLE_WORDS = 240
S_ALL_M8 = int("07" + "77" * 30 + "78", 16)      # recoded digits all -8 below the top: table row 8 alone
S_ALL_7 = int("07" + "77" * 31, 16)
S_SET = (0, 1, L - 1, S_ALL_M8, S_ALL_7, 2**252)
COL_BOUND = 2**62.4                               # the header's bound on a column sum


def limbs_of(v):
    out = []
    for b in BITS:
        out.append(v & ((1 << b) - 1))
        v >>= b
    assert v == 0
    return out


def value_of(limbs):
    return sum(int(x) << w for x, w in zip(limbs, WEIGHT))


def words_of(v, n=8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def int_of_words(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def within(limbs, bound):
    return all(0 <= int(x) <= b for x, b in zip(limbs, bound))


def neg_tight(limbs):
    """2p - a, limb by limb: what ge_pre_digit hands ge_madd for a negative digit"""
    return [p2 - a for p2, a in zip(P2, limbs)]


# --- points -------------------------------------------------------------------------
def order_of(pt):
    """the order of a torsion point (1, 2, 4 or 8), None for any other point"""
    q, n = pt, 1
    while q != (0, 1):
        if n == 8:
            return None
        q, n = model.add(q, q), 2 * n
    return n


_cache = {}


def torsion_points():
    """the eight torsion points, by order: 1, 2, 4, 4, 8, 8, 8, 8"""
    if "tors" not in _cache:
        y = 2
        while True:      # the first y whose point has a torsion part of order 8
            pt = model.decode_point(y.to_bytes(32, "little"))
            if pt is not None:
                g = model.mul(L, pt)
                if order_of(g) == 8:
                    break
            y += 1
        pts, q = [], (0, 1)
        for _ in range(8):
            pts.append(q)
            q = model.add(q, g)
        assert q == (0, 1) and len(set(pts)) == 8
        _cache["tors"] = sorted(pts, key=lambda t: (order_of(t), t[0] & 1, t[1]))
    return list(_cache["tors"])


def honest_keys(n, tag="probe"):
    rng = random.Random("ed25519-probe-keys-" + tag)
    return [model.public_key(bytes(rng.randrange(256) for _ in range(32))) for _ in range(n)]


def entry_of(pt):
    x, y = pt
    return ((y + x) % P, (y - x) % P, 2 * D * x * y % P)


def table_of_key(key):
    """the 240 words of the key's table as canonical limbs: i * (-A), i = 1..8"""
    out = []
    for e in model.neg_multiples(key):
        for v in e:
            out += limbs_of(v)
    return out


NEG_BASE_KEY = model.encode((-model.B[0] % P, model.B[1]))       # its table holds the multiples of B


# --- sc_reduce512 -------------------------------------------------------------------
def sc_reduce_subtractions(x):
    """how many times sc_reduce512's final loop subtracts L for a 512-bit x: the
    mirror of its v = x_lo + z_lo + 2 L - y_lo - c z_hi"""
    m = 2**252
    y = C * (x >> 252)
    z = C * (y >> 252)
    v = (x % m) + (z % m) + 2 * L - (y % m) - C * (z >> 252)
    assert 0 <= v < 4 * L and (v - x) % L == 0
    return v // L


def reduce_inputs():
    """64-byte inputs of sc_reduce512 as integers; every count 0..3 of final subtractions occurs"""
    if "reduce" in _cache:
        return list(_cache["reduce"])
    rng = random.Random("ed25519-probe-reduce")
    top = 2**512 - 1
    kmax = top // L
    xs = [0, top, 2**252 - 1, 2**256, 2**504]
    for k in (0, 1, 2, 3, 2**64, 2**128 + 1, 2**200, 2**252, 2**259, kmax // 3, kmax - 1, kmax):
        xs += [k * L + d for d in (-1, 0, 1) if 0 <= k * L + d <= top]
    xs += [2**252 * f for f in (1, 2, 3, 15, 16, 2**128 - 1, 2**259, 2**260 - 1)]
    # long runs of ones above bit 252 and zeros below, and the reverse
    xs += [2**512 - 2**252, 2**400 - 2**252, 2**252 * (2**100 - 1), 2**512 - 2**252 + 1, 2**300 + 2**252 - 1,
           2**253 - 1, 2**512 - 2**253]
    # no final subtraction: y_lo near 2^252, z_lo small, z_hi = 3, x_lo = 0
    y_hi = -(-3 * 2**252 // C)
    x_hi = ((y_hi + 1) * 2**252 - 1) // C
    assert x_hi < 2**260
    xs.append(x_hi << 252)
    # three: x_lo and z_lo near 2^252, y_lo small, z_hi = 0
    y_hi = (2**252 - 1) // C
    x_hi = -(-y_hi * 2**252 // C)
    xs.append((x_hi << 252) + 2**252 - 1)
    xs += [rng.randrange(2**512) for _ in range(40)] + [rng.randrange(2**256) for _ in range(10)]
    xs = list(dict.fromkeys(xs))
    assert {sc_reduce_subtractions(x) for x in xs} == {0, 1, 2, 3}
    _cache["reduce"] = xs
    return list(xs)


# --- field operands -----------------------------------------------------------------
STRUCTURED = [0, 1, 2, 19, P - 1, P, P + 18]      # as in test_field_on_host (P + 18 = 2^255 - 1)


CARRY_IN = [2**32 - 2**7 - 1] * 10        # what fe_carry takes


def loose_encoding(v, rng=None, bound=INPUT):
    """limbs of value v (< 2^258) that need not be canonical: the excess sits in
    limb 9; with rng, units also move down from a limb to the one below"""
    lim = limbs_of(v % 2**230) + [0]
    lim = lim[:9] + [v >> 230]
    if rng is not None:
        for k in range(9, 0, -1):
            room = (INPUT[k - 1] - lim[k - 1]) >> BITS[k - 1]
            take = rng.randrange(min(lim[k], room) + 1)
            lim[k] -= take
            lim[k - 1] += take << BITS[k - 1]
    assert value_of(lim) == v and within(lim, bound)
    return lim


def wide_rows():
    """k p + d for k = 4..6: above what the input bound can hold (its limbs sum
    to less than 3.26 * 2^255), so these go to fe_carry and to fe_sub's first
    operand only, whose limbs may be wider"""
    rng = random.Random("ed25519-probe-wide")
    return [loose_encoding(k * P + d, rng if (k + d) % 2 else None, CARRY_IN) for k in (4, 5, 6) for d in range(-20, 21)]


def field_rows():
    """limb vectors within the input bound"""
    if "field" in _cache:
        return list(_cache["field"])
    rng = random.Random("ed25519-probe-field")
    rows = [limbs_of(v) for v in STRUCTURED]
    for bound in (INPUT, TIGHT):
        rows.append(list(bound))
        rows.append([b if k % 2 == 0 else 0 for k, b in enumerate(bound)])
        rows.append([b if k % 2 == 1 else 0 for k, b in enumerate(bound)])
    # carry ripples: limbs 1..9 all ones, limb 0 around 2^26 and 2^27; then each limb one above or below
    ones = list(MASK)
    for v0 in list(range(2**26 - 20, 2**26 + 20)) + [2**27 - 19, 2**27, INPUT[0]]:
        rows.append([v0] + ones[1:])
    for k in range(1, 10):
        for dlt in (1, -1):
            r = [2**26 - 19] + ones[1:]
            r[k] += dlt
            rows.append(r)
    # k p + d, not canonical (k = 4..6 do not fit the input bound: wide_rows)
    for k in range(4):
        for d in range(-20, 21):
            if k * P + d >= 0:
                rows.append(loose_encoding(k * P + d, rng if (k + d) % 2 else None))
    rows += [[rng.randrange(b + 1) for b in TIGHT] for _ in range(150)]
    rows += [[rng.randrange(b + 1) for b in INPUT] for _ in range(100)]
    assert all(within(r, INPUT) for r in rows)
    _cache["field"] = rows
    return list(rows)


def tight_rows():
    return [r for r in field_rows() if within(r, TIGHT)]


def paired(rows, step=7, off=3):
    n = len(rows)
    return [(rows[i], rows[(i * step + off) % n]) for i in range(n)]


# --- operations ---------------------------------------------------------------------
class Op:
    """rows: the lanes' input words; tabs: tables for the lanes that index one
    (None: the operation reads none); check(i, out): asserts lane i's result"""

    def __init__(self, name, n_in, n_out, n_idx=0, threads=256):
        self.name, self.n_in, self.n_out, self.n_idx, self.threads = name, n_in, n_out, n_idx, threads
        self.rows, self.tabs, self.keys = [], None, None
        self._checks = []

    def add(self, inp, check):
        assert len(inp) == self.n_in, (self.name, len(inp))
        self.rows.append([int(w) for w in inp])
        self._checks.append(check)

    def check(self, i, out):
        assert len(out) == self.n_out
        self._checks[i]([int(w) for w in out])

    def fill(self, n=LANE_COUNTS[-1]):
        """repeat the rows up to n lanes (a rotation, so that no two neighbours are the same row)"""
        base = len(self.rows)
        assert base > 1
        j = 0
        while len(self.rows) < n:
            k = (j * 5 + j // base) % base
            self.rows.append(self.rows[k])
            self._checks.append(self._checks[k])
            j += 1


def _fe_check(name, want, bound, what):
    def check(out):
        assert within(out, bound), (name, what, "bound", out)
        assert value_of(out) % P == want % P, (name, what, "value")
    return check


def _build_field(ops):
    rows = field_rows()
    tight = tight_rows()
    pairs = [(limbs_of(a), limbs_of(b)) for a in STRUCTURED for b in STRUCTURED] + paired(rows)
    pairs += [(list(INPUT), list(INPUT)), (list(INPUT), limbs_of(P - 1)), (limbs_of(1), list(INPUT))]
    mul, sub = Op("fe_mul", 20, 10), Op("fe_sub", 20, 10)
    for a, b in pairs:
        va, vb = value_of(a), value_of(b)
        mul.add(a + b, _fe_check("fe_mul", va * vb, TIGHT, (a, b)))
        sub.add(a + b, _fe_check("fe_sub", va - vb, TIGHT, (a, b)))
    for i, a in enumerate(wide_rows()):
        b = rows[(11 * i + 5) % len(rows)]
        sub.add(a + b, _fe_check("fe_sub", value_of(a) - value_of(b), TIGHT, (a, b)))
    add = Op("fe_add", 20, 10)
    for a, b in paired(tight, 5, 1) + paired(tight, 3, 2):
        def check(out, a=a, b=b):
            assert out == [x + y for x, y in zip(a, b)] and within(out, LOOSE), ("fe_add", a, b)
        add.add(a + b, check)
    unary = {"fe_sqr": lambda v: v * v, "fe_neg": lambda v: -v, "fe_carry": lambda v: v,
             "fe_invert": lambda v: pow(v, P - 2, P), "fe_pow22523": lambda v: pow(v, (P - 5) // 8, P)}
    out = [mul, Op("fe_sqr", 10, 10), add, sub, Op("fe_neg", 10, 10), Op("fe_carry", 10, 10)]
    for op in out:
        if op.name in unary:
            for a in rows:
                op.add(a, _fe_check(op.name, unary[op.name](value_of(a)), TIGHT, a))
    for a in wide_rows():
        out[5].add(a, _fe_check("fe_carry", value_of(a), TIGHT, a))
    nt = Op("fe_neg_tight", 10, 10)
    for a in tight:
        nt.add(a, _fe_check("fe_neg_tight", -value_of(a), INPUT, a))
    fw = Op("fe_from_words", 8, 10)
    rng = random.Random("ed25519-probe-words")
    vals = STRUCTURED + [k * P + d for k in (1, 2) for d in range(-20, 21) if k * P + d < 2**255]
    vals += [2**255 - 20, 2**255 - 19, 2**255 - 2] + [rng.randrange(2**255) for _ in range(230)]
    for i, v in enumerate(vals):
        def check(out, v=v):
            assert out == limbs_of(v), ("fe_from_words", hex(v))
        fw.add(words_of(v | (i & 1) << 255), check)
    tw = Op("fe_to_words", 10, 10)
    for a in rows:
        def check(out, a=a):
            v = value_of(a) % P
            assert int_of_words(out[:8]) == v, ("fe_to_words", a, hex(int_of_words(out[:8])))
            assert out[8] == (1 if v == 0 else 0) and out[9] == (v & 1), ("fe_to_words flags", a)
        tw.add(a, check)
    inv, pw = Op("fe_invert", 10, 10), Op("fe_pow22523", 10, 10)
    for op in (inv, pw):
        for a in rows:
            op.add(a, _fe_check(op.name, unary[op.name](value_of(a) % P), TIGHT, a))
    ops += out + [nt, fw, tw, inv, pw]


def _build_scalar(ops):
    rng = random.Random("ed25519-probe-scalars")
    lt = Op("sc_lt_L", 8, 1)
    vals = [0, 1, L - 1, L, L + 1, 2**252, 2**252 - 1, 2**253, 2**256 - 1, S_ALL_M8, S_ALL_7, C, C - 1]
    lw = words_of(L)
    for i in range(8):        # L with one word one above or one below: every position of the borrow chain
        for dlt in (1, -1):
            w = list(lw)
            w[i] = (w[i] + dlt) % 2**32
            vals.append(int_of_words(w))
    vals += [rng.randrange(2**256) for _ in range(120)] + [L + rng.randrange(-2**128, 2**128) for _ in range(120)]
    for s in vals:
        def check(out, s=s):
            assert out == [1 if s < L else 0], ("sc_lt_L", hex(s))
        lt.add(words_of(s), check)
    red = Op("sc_reduce512", 16, 8)
    for x in reduce_inputs() + [rng.randrange(2**512) for _ in range(200)]:
        def check(out, x=x):
            assert int_of_words(out) == x % L, ("sc_reduce512", hex(x))
        red.add(words_of(x, 16), check)
    dig = Op("sc_digits", 8, 64)
    vals = list(S_SET) + [7, 8, 15, 16, 2**253 - 1, int("77" * 32, 16), int("08" * 32, 16), int("80" * 31, 16)]
    vals += [rng.randrange(L) for _ in range(250)]
    for s in vals:
        def check(out, s=s):
            d = [w - 8 for w in out]
            assert all(-8 <= x <= 7 for x in d), ("sc_digits", hex(s))
            assert sum(x * 16**(63 - i) for i, x in enumerate(d)) == s, ("sc_digits", hex(s))
        dig.add(words_of(s), check)
    ops += [lt, red, dig]


def _affine(X, Y, Z):
    zi = pow(Z, P - 2, P)
    return X * zi % P, Y * zi % P


def _group_check(name, factors, g_bound, want_point, what):
    """factors: the integer E, H, G, F; the lane returns them and ge_finish's X, Y, Z, T"""
    E, H, G, F = factors

    def check(out):
        fe = [out[10 * j:10 * j + 10] for j in range(8)]
        for j, (tag, want, bound) in enumerate((("E", E, TIGHT), ("H", H, LOOSE), ("G", G, g_bound), ("F", F, TIGHT),
                                                ("X", E * F, TIGHT), ("Y", G * H, TIGHT), ("Z", F * G, TIGHT),
                                                ("T", E * H, TIGHT))):
            assert within(fe[j], bound), (name, what, tag, "bound", fe[j])
            assert value_of(fe[j]) % P == want % P, (name, what, tag, "value")
        if want_point is not None:
            X, Y, Z, T = (value_of(f) % P for f in fe[4:])
            assert Z != 0 and _affine(X, Y, Z) == want_point and T * Z % P == X * Y % P, (name, what, "point")
    return check


def _dbl_factors(X, Y, Z):
    xx, yy, zz, a = X * X, Y * Y, Z * Z, (X + Y) ** 2
    H, G = yy + xx, yy - xx
    return a - H, H, G, 2 * zz - G


def _madd_factors(X, Y, Z, T, ypx, ymx, xy2d):
    a, b, c, d = (Y + X) * ypx, (Y - X) * ymx, xy2d * T, 2 * Z
    return a - b, a + b, d + c, d - c


def _build_group(ops):
    rng = random.Random("ed25519-probe-group")
    zero, tmax = [0] * 10, list(TIGHT)
    alt = [t if k % 2 == 0 else 0 for k, t in enumerate(TIGHT)]
    rnd = lambda: [rng.randrange(b + 1) for b in TIGHT]     # noqa: E731
    G3 = [3 * t for t in TIGHT]
    assert all(g <= i for g, i in zip(G3, INPUT))
    tors = torsion_points()
    points = tors + [model.decode_point(k) for k in honest_keys(6, "group")]

    def projective(pt):
        z = rng.randrange(1, P)
        return [limbs_of(pt[0] * z % P), limbs_of(pt[1] * z % P), limbs_of(z), limbs_of(pt[0] * pt[1] * z % P)]

    dbl = Op("ge_dbl", 30, 80)
    cases = [([x, y, z], None) for x in (zero, tmax) for y in (zero, tmax) for z in (zero, tmax)]
    cases += [([alt, tmax, alt], None), ([tmax, alt, tmax], None)]
    cases += [([rnd(), rnd(), rnd()], None) for _ in range(100)]
    cases += [(projective(pt)[:3], model.add(pt, pt)) for pt in points for _ in range(2)]
    for fes, want in cases:
        vals = [value_of(f) for f in fes]
        dbl.add(sum(fes, []), _group_check("ge_dbl", _dbl_factors(*vals), TIGHT, want, fes))

    madd = Op("ge_madd", 70, 80)
    cases = []
    for pfe in (zero, tmax):
        for ypx in (zero, tmax):
            for ymx in (zero, tmax):
                for xy2d in (zero, tmax, neg_tight(zero), neg_tight(tmax)):
                    cases.append(([pfe] * 4 + [ypx, ymx, xy2d], None))
    cases.append(([tmax, alt, tmax, alt, alt, tmax, neg_tight(alt)], None))
    for i in range(100):
        q = [rnd(), rnd(), rnd()]
        if i % 2:      # as ge_pre_digit hands over a negative digit
            q[2] = neg_tight(q[2])
        cases.append(([rnd(), rnd(), rnd(), rnd()] + q, None))
    for pt in points:
        for tag, q in (("p", pt), ("-p", (-pt[0] % P, pt[1])), ("identity", (0, 1))):
            e = [limbs_of(v) for v in entry_of(q)]
            cases.append((projective(pt) + e, model.add(pt, q)))
            # the same entry as a negative digit gives it: the entry of -q, swapped and negated
            nq = [limbs_of(v) for v in entry_of((-q[0] % P, q[1]))]
            cases.append((projective(pt) + [nq[1], nq[0], neg_tight(nq[2])], model.add(pt, q)))
    for fes, want in cases:
        vals = [value_of(f) for f in fes]
        madd.add(sum(fes, []), _group_check("ge_madd", _madd_factors(*vals), G3, want, fes))
    dbl.fill()
    madd.fill()
    ops += [dbl, madd]


def _build_keys(ops, fixture_keys):
    """fixture_keys: [(key bytes, loads, ring's x or None)] of the crafted fixture"""
    dec = Op("ge_decode", 8, 21)
    for key, loads, x in fixture_keys:
        def check(out, key=key, loads=loads, x=x):
            assert out[0] == (1 if loads else 0), ("ge_decode", key.hex())
            y = (int.from_bytes(key, "little") & (2**255 - 1))
            assert value_of(out[11:21]) % P == y % P and within(out[11:21], TIGHT), ("ge_decode y", key.hex())
            if loads:
                assert value_of(out[1:11]) % P == x and within(out[1:11], TIGHT), ("ge_decode x", key.hex())
        dec.add(words_of(int.from_bytes(key, "little")), check)
    dec.fill()

    kt = Op("key_table", 9, 1 + TABLE_WORDS, threads=64)
    keys = [(k, 32, 0 if loads else 2) for k, loads, _ in fixture_keys]
    keys += [(honest_keys(1, "len")[0], ln, 1) for ln in (0, 1, 31, 33, 64, 2**32 - 1)]
    keys += [(k, 32, 0) for k in honest_keys(max(0, 257 - len(keys)), "table")]
    keys = keys[:257]
    for key, ln, status in keys:
        def check(out, key=key, status=status):
            assert out[0] == status, ("key_table status", key.hex(), out[0])
            if status == 0:
                fes = [out[1 + 10 * q:11 + 10 * q] for q in range(24)]
                assert all(within(f, TIGHT) for f in fes), ("key_table bound", key.hex())
                got = [tuple(value_of(f) % P for f in fes[3 * i:3 * i + 3]) for i in range(8)]
                assert got == model.neg_multiples(key), ("key_table", key.hex())
        kt.add([ln] + words_of(int.from_bytes(key, "little")), check)
    ops += [dec, kt]


def _build_tables(ops):
    tors = torsion_points()
    # ge_pre_digit: two keys, all 17 digits
    pre = Op("ge_pre_digit", 2, 30, n_idx=1)
    pkeys = [honest_keys(1, "pre")[0], model.encode(tors[5])]
    pre.keys = pkeys
    pre.tabs = [table_of_key(k) for k in pkeys]
    for ti, key in enumerate(pkeys):
        mult = model.neg_multiples(key)
        for d in range(-8, 9):
            if d == 0:
                want = (1, 1, 0)
            elif d > 0:
                want = mult[d - 1]
            else:
                e = mult[-d - 1]
                want = (e[1], e[0], -e[2] % P)

            def check(out, want=want, d=d, ti=ti):
                got = tuple(value_of(out[10 * j:10 * j + 10]) % P for j in range(3))
                assert got == want, ("ge_pre_digit", ti, d)
                assert within(out[:20], TIGHT) and within(out[20:], INPUT), ("ge_pre_digit bound", ti, d)
            pre.add([ti, d + 8], check)
    pre.fill()

    # verify_equation
    rng = random.Random("ed25519-probe-verify")
    ve = Op("verify_equation", 26, 1, n_idx=2)
    vkeys = [model.encode(t) for t in tors] + honest_keys(3, "verify")
    ve.keys = vkeys + [NEG_BASE_KEY]
    ve.tabs = [table_of_key(k) for k in ve.keys]
    base_idx = len(vkeys)
    rs = lambda: rng.randrange(L)      # noqa: E731
    for ki, key in enumerate(vkeys):
        if ki == 4:
            combos = [(s, h) for s in S_SET + (rs(),) for h in S_SET + (rs(),)]
        elif ki == len(vkeys) - 1:
            combos = [(s, s) for s in S_SET] + [(s, rs()) for s in S_SET] + [(rs(), rs()), (rs(), 0)]
        else:
            combos = [(S_SET[(ki + j) % 6], S_SET[(ki + 2 * j + 1) % 6]) for j in range(3)] + [(rs(), rs()), (0, rs()),
                                                                                              (rs(), S_ALL_M8)]
        a = model.decode_point(key)
        na = (-a[0] % P, a[1])
        for s, h in combos:
            pt = model.add(model.mul(s, model.B), model.mul(h, na))
            good = int.from_bytes(model.encode(pt), "little")
            variants = [(good, 1), (good ^ 1 << rng.randrange(256), 0)]
            if pt[1] + P < 2**255:
                variants.append((good + P, 0))
            if pt[0] == 0:
                variants.append((good | 1 << 255, 0))
            for r, want in variants:
                def check(out, want=want, ki=ki, s=s, h=h, r=r):
                    assert out == [want], ("verify_equation", ki, hex(s), hex(h), hex(r))
                ve.add([ki, base_idx] + words_of(s) + words_of(h) + words_of(r), check)
    assert len(ve.rows) <= 257, len(ve.rows)
    ops += [pre, ve]


def ops(fixture_keys):
    """every operation with its table; fixture_keys: see _build_keys"""
    if "ops" not in _cache:
        out = []
        _build_field(out)
        _build_scalar(out)
        _build_group(out)
        _build_keys(out, fixture_keys)
        _build_tables(out)
        _cache["ops"] = out
    return _cache["ops"]


OP_NAMES = ["fe_mul", "fe_sqr", "fe_add", "fe_sub", "fe_neg", "fe_carry", "fe_neg_tight", "fe_from_words",
            "fe_to_words", "fe_invert", "fe_pow22523", "sc_lt_L", "sc_reduce512", "sc_digits", "ge_dbl", "ge_madd",
            "ge_decode", "key_table", "ge_pre_digit", "verify_equation"]


def get_op(name, fixture_keys):
    return next(o for o in ops(fixture_keys) if o.name == name)


def active_mask(n, half):
    """all lanes live, or lanes i mod 4 in {1, 2} switched off"""
    return [0 if half and i % 4 in (1, 2) else 1 for i in range(n)]


# --- running an operation ---------------------------------------------------------------
def run(call, op, n, active, tabs=None):
    """lanes 0..n of op through call(name, n, active, in, out, tabs, n_tabs), which
    returns a status; the (n, n_out) results, rows of inactive lanes still
    holding the poison; tabs: the tables (lists of 240 words), default op.tabs"""
    import ctypes

    import numpy as np
    tabs = op.tabs if tabs is None else tabs
    inp = np.array(op.rows[:n], dtype=np.uint32).reshape(n, op.n_in)
    out = np.full((n, op.n_out), POISON, dtype=np.uint32)
    act = np.array(active, dtype=np.uint8)
    assert len(act) == n
    t = np.array(tabs, dtype=np.uint32).reshape(-1, TABLE_WORDS) if tabs else None
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    status = call(op.name, n, p(act), p(inp), p(out), p(t) if t is not None else None, len(t) if t is not None else 0)
    return status, out


def check_lanes(op, out, active):
    for i, live in enumerate(active):        # every lane is compared
        if not live:
            assert (out[i] == POISON).all(), (op.name, len(active), i, "an inactive lane's result was written")
            continue
        op.check(i, out[i])


def tables_from(out):
    """the tables of a key_table result (status word dropped)"""
    return [[int(w) for w in row[1:]] for row in out]
