"""Operand tables and integer references of the one-lane BLS primitives
(cess_amd/csrc/bls/field.hpp Fp and Fp2, curve.hpp, h2c.hpp, the line steps of
pairing.hpp), one operation per probe entry (tests/probe/lane_probe.hip),
shared by the host build (tests/test_lane_primitives.py) and the GPU probe
(tests/test_gpu_lane_primitives.py).

Plain Python integers on oracle/bls_oracle.py; nothing is taken from the code
under test.  The kernels hold an Fp value x as raw limbs with raw = x R (mod
p), R = 2^392, anywhere in the operation's documented range, so the model
applies R itself: mont(x) = x R mod p, res(raw) = raw / R mod p.

An operation (`Op`) has
  n_in / n_out  words per lane (an Fp is 12 words, an Fp2 c0 then c1, a
                point x, y, z; as tests/probe/lane_probe.hip lists them),
  fps, in_bound the word offsets of its Fp operands and the header's
                documented (exclusive) bound on each, asserted by contract()
                before anything is launched,
  rows          the lanes' input words,
  and per row the expected result as a list of items:
    ("mod", v, bound)   an Fp congruent to v mod p and below bound (the
                        promised range: 2p for stored values, 4p for add_nr,
                        6p for add_xi_nr, p for from_mont / fp_reduce_once),
    ("raw", v)          an Fp with exactly these limbs (where the header
                        fixes the representation),
    ("w", v)            one word (predicates, flags),
    ("words", [..])     exact words,
    ("any", n)          n words the header leaves unspecified,
    ("fn", n, f)        n words handed to f, which asserts (projective points).
"""
import hashlib
import random

import oracle.bls_oracle as o
from pair_probe_model import PRODUCT_EDGES, STORED_EDGES, _twin

P = o.P
R = 1 << 392
RINV = pow(R, -1, P)
ONE = R % P
TOP = (1 << 384) - 1
POISON = 0xDEADBEEF
LANE_COUNTS = (1, 65, 321)        # one lane; a wave and a lane; a block, a wave and a lane
MSG_WORDS = 251
N_LINES = 68
X_ABS = o.BLS_X
LAMBDA = X_ABS * X_ABS - 1        # curve.hpp: r = L^2 + L + 1
XMD_LENGTHS = (0, 1, 7, 8, 9, 55, 56, 71, 72, 73, 135, 136, 137, 1000)
DEVICE_ONLY = ("hash_to_g1_parked", "g2_prepare_lds")      # they park values in LDS: no host build
# pow_fixed's exponents, by the probe's index (lp::pow_by_index)
EXPONENTS = [(P + 1) // 4, (P - 3) // 4, P - 2, 1, (1 << 383) + 1, TOP, int("8" * 96, 16)]


def mont(x):
    return x * R % P


def res(raw):
    return raw * RINV % P


def words(v, n=12):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def val(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def w2(a):
    return words(a[0]) + words(a[1])


def v2(ws):
    return (val(ws[:12]), val(ws[12:24]))


def res2(a):
    return (res(a[0]), res(a[1]))


def mont2(a):
    return (mont(a[0]), mont(a[1]))


# --- operations -----------------------------------------------------------------------
class Op:
    def __init__(self, name, n_in, n_out, fps=(), in_bound=2 * P, cheap=False):
        self.name, self.n_in, self.n_out = name, n_in, n_out
        self.fps, self.in_bound, self.cheap = tuple(fps), in_bound, cheap
        self.rows, self.items, self.tags = [], [], []
        self.n_unique = None

    def add(self, inp, items, tag=None):
        assert len(inp) == self.n_in, (self.name, len(inp))
        self.rows.append([int(w) for w in inp])
        self.items.append(items)
        self.tags.append(tag)

    def contract(self):
        """every Fp operand of every row is inside the header's documented bound"""
        for r, row in enumerate(self.rows[:self.n_unique]):
            for at in self.fps:
                assert val(row[at:at + 12]) < self.in_bound, (self.name, r, at)

    def fill(self, n=LANE_COUNTS[-1]):
        """separate equal neighbours, then repeat the rows up to n lanes (a
        rotation, so that no two neighbours are the same row)"""
        keep = [i for i in range(len(self.rows)) if i == 0 or self.rows[i] != self.rows[i - 1]]
        self.rows, self.items, self.tags = ([x[i] for i in keep] for x in (self.rows, self.items, self.tags))
        base = self.n_unique = len(self.rows)
        assert base > 2, self.name
        j = 0
        while len(self.rows) < n:
            k = (j * 5 + j // base) % base
            if self.rows[k] != self.rows[-1]:
                self.rows.append(self.rows[k])
                self.items.append(self.items[k])
                self.tags.append(self.tags[k])
            j += 1

    def check(self, i, out):
        out = [int(w) for w in out]
        assert len(out) == self.n_out
        at, what = 0, (self.name, i, self.tags[i])
        for it in self.items[i]:
            kind = it[0]
            if kind == "mod":
                got = val(out[at:at + 12])
                assert got < it[2], what + ("bound", at, hex(got))
                assert got % P == it[1] % P, what + ("value", at, hex(got))
                at += 12
            elif kind == "raw":
                assert val(out[at:at + 12]) == it[1], what + ("limbs", at, hex(val(out[at:at + 12])))
                at += 12
            elif kind == "w":
                assert out[at] == it[1], what + ("word", at, out[at])
                at += 1
            elif kind == "words":
                assert out[at:at + len(it[1])] == list(it[1]), what + ("words", at)
                at += len(it[1])
            elif kind == "any":
                at += it[1]
            else:
                it[2](out[at:at + it[1]], what)
                at += it[1]
        assert at == self.n_out, what


def M(v, bound=2 * P):
    return ("mod", v % P, bound)


def M2(a, bound=2 * P):
    return [M(a[0], bound), M(a[1], bound)]


# --- operand classes --------------------------------------------------------------------
def _ripples():
    """pairs whose sum or difference carries through all 12 words"""
    out = [((1 << 380) - 1, 1), (1, (1 << 380) - 1), (0, 1), (1 << 352, 1), ((1 << 381) - 1, (1 << 381) - 1),
           (0xFFFFFFFF, 1), ((1 << 352) - 1, (1 << 380) - (1 << 352) + 1), (2 * P - 1, 2 * P - 1), (0, 2 * P - 1),
           (P, P), (P - 1, P + 1), (2 * P - 1, 1), (1, 2 * P - 1), ((1 << 381) - 1, 1)]
    for k in range(1, 12):
        out += [((1 << (32 * k)) - 1, 1), (1 << (32 * k), 1), (0, 1 << (32 * k))]
    return [(a, b) for a, b in out if a < 2 * P and b < 2 * P]


def fp_values(edges, bound, seed, n_rand=250):
    rng = random.Random(seed)
    vals = list(edges) + [(1 << k) - 1 for k in range(29, 384, 32) if (1 << k) - 1 < bound]
    vals += [rng.randrange(bound) for _ in range(n_rand)]
    vals += [_twin(v) for v in vals[len(edges)::9] if bound >= 2 * P and v < 2 * P]
    return vals


def fp_pairs(edges, bound, seed, n_rand=200):
    rng = random.Random(seed)
    pairs = [(a, b) for a in edges for b in edges] + _ripples()
    body = [(rng.randrange(bound), rng.randrange(bound)) for _ in range(n_rand)]
    body += [(rng.choice(edges), rng.randrange(bound)) for _ in range(40)]
    body += [(rng.randrange(bound), rng.choice(edges)) for _ in range(40)]
    rng.shuffle(pairs)
    return [p for i, p in enumerate(pairs + body) if i == 0 or p != (pairs + body)[i - 1]]


def fp2_values(n_ops, edges, bound, seed, n=330):
    """n cases of n_ops Fp2 values: uniform edges, per-component edge draws, random values, twins"""
    rng = random.Random(seed)
    cases = [[(v, v)] * n_ops for v in (bound - 1, 0, P, 2 * P - 1, ONE + P)]
    cases.append([(0, P) if i & 1 else (P, 0) for i in range(n_ops)])
    cases.append([(2 * P - 1, 0) if i & 1 else (0, 2 * P - 1) for i in range(n_ops)])
    if n_ops == 1:
        cases += [[(a, b)] for a in edges for b in edges]
    while len(cases) < n:
        if len(cases) % 8 == 7 and all(a < 2 * P and b < 2 * P for a, b in cases[-1]):
            cases.append([(_twin(a), _twin(b)) for a, b in cases[-1]])
            continue
        pe = rng.choice((0.0, 0.3, 0.8))
        draw = lambda: rng.choice(edges) if rng.random() < pe else rng.randrange(bound)   # noqa: E731
        cases.append([(draw(), draw()) for _ in range(n_ops)])
    return cases


def enc(v, rng, p_twin=0.3):
    """a stored representation of the residue v: x R mod p, or that plus p"""
    m = mont(v)
    return m + P if rng.random() < p_twin else m


def enc2(a, rng):
    return (enc(a[0], rng), enc(a[1], rng))


# --- inversion: the header's divsteps, counted ---------------------------------------------
def divstep_iterations(g, f=P):
    """how many times inv()'s loop body must run until g = 0: 30 half-delta
    divsteps per iteration (zeta = -1 at the start; a swap when zeta < 0 and g
    is odd sets zeta to -zeta - 2, any other step to zeta - 1), on f = p and
    the canonical value g, as divsteps30 / update_fg30 compute them"""
    zeta, it = -1, 0
    while g != 0:
        for _ in range(30):
            if g & 1:
                if zeta < 0:
                    f, g, zeta = g, (g - f) >> 1, -zeta - 2
                else:
                    g, zeta = (g + f) >> 1, zeta - 1
            else:
                g, zeta = g >> 1, zeta - 1
        it += 1
        assert it <= 37
    return it


def divstep_iterations_matrix(g, f=P):
    """the same count the way the header runs it: the steps on the low 30 bits
    only (divsteps30), then the 2x2 matrix applied to the full f, g (update_fg30)"""
    zeta, it = -1, 0
    while g != 0:
        u, v, q, r = 1, 0, 0, 1
        fl, gl = f & 0x3FFFFFFF, g & 0x3FFFFFFF
        for _ in range(30):
            if gl & 1:
                if zeta < 0:
                    fl, gl, u, v, q, r, zeta = gl, gl - fl, q, r, q - u, r - v, -zeta - 2
                else:
                    gl, q, r, zeta = gl + fl, q + u, r + v, zeta - 1
            else:
                zeta -= 1
            gl >>= 1
            u, v = 2 * u, 2 * v
        nf, ng = u * f + v * g, q * f + r * g
        assert nf % (1 << 30) == 0 and ng % (1 << 30) == 0
        f, g = nf >> 30, ng >> 30
        it += 1
        assert it <= 37
    return it


INV_EDGES = [0, 1, 2, 3, P - 1, P, P + 1, 2 * P - 1, (P - 1) // 2, (P + 1) // 2, 1 << 380, (1 << 380) - 1,
             (1 << 381) - 1 - P, R % P, RINV] + [(1 << k) % P for k in range(0, 381, 7)] + \
            [((1 << k) - 1) % P for k in range(1, 381, 11)]          # as test_hostemu.py test_fp_inv_safegcd
INV_SEARCH = 3000


def inv_class(raw):
    """'zero0', 'zerop', or the iteration count of a raw operand of inv()"""
    if raw % P == 0:
        return "zero0" if raw == 0 else "zerop"
    return divstep_iterations(raw % P)


_cache = {}


def inv_rows():
    """the raw operands of fp_inv in lane order, and their classes.  The first
    wave (lanes 0..63) holds both zeros, the 26-iteration class and the >= 27
    class, also among the lanes that stay live when i mod 4 in {1, 2} are
    switched off; the second wave (lanes 64..127) holds the 26 class alone, so
    it leaves the loop earlier than the first."""
    if "inv" in _cache:
        return _cache["inv"]
    rng = random.Random("lane-probe-inv")
    found = {}
    for _ in range(INV_SEARCH):
        a = rng.randrange(1, P)
        found.setdefault(divstep_iterations(a), []).append(a)
    low = found[26]
    high = [a for k in sorted(found) if k >= 27 for a in found[k]]
    assert len(low) > 200 and len(high) >= 6, {k: len(v) for k, v in found.items()}
    rest = [v for v in INV_EDGES if v not in (0, P)]
    first = [None] * 64
    first[0], first[3], first[4], first[7], first[8] = 0, P, high[0], high[1], high[2] + P
    first[1], first[2], first[5], first[6] = P, 0, high[3], high[4]
    free = [i for i in range(64) if first[i] is None]
    fill = rest[:len(free) - 8] + low[:8]
    for i, v in zip(free, fill):
        first[i] = v
    second = [a + (P if i % 5 == 0 else 0) for i, a in enumerate(low[8:72])]
    tail = rest[len(free) - 8:] + high[5:] + [a for k in sorted(found) if k < 26 for a in found[k]]
    tail += [rng.randrange(2 * P) for _ in range(400 - len(tail))]
    rows = first + second + tail
    classes = [inv_class(v) for v in rows]
    _cache["inv"] = (rows, classes)
    return _cache["inv"]


def assert_inv_placement(rows, classes):
    for live in (lambda i: True, lambda i: i % 4 not in (1, 2)):
        seen = {classes[i] for i in range(64) if live(i)}
        assert {"zero0", "zerop", 26} <= seen and any(isinstance(c, int) and c >= 27 for c in seen), seen
    assert set(classes[64:128]) == {26}
    assert all(rows[i] != rows[i + 1] for i in range(len(rows) - 1))


# --- polynomials over Fp (the isogeny's kernel) ---------------------------------------------
def _ptrim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _pmod(a, m):
    a = list(a)
    inv_lead = pow(m[-1], -1, P)
    while len(a) >= len(m):
        c = a[-1] * inv_lead % P
        if c:
            for i in range(len(m)):
                a[len(a) - len(m) + i] = (a[len(a) - len(m) + i] - c * m[i]) % P
        a.pop()
    return _ptrim(a)


def _pmulmod(a, b, m):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % P
    return _pmod(out, m)


def _ppowmod(base, e, m):
    acc, base = [1], _pmod(base, m)
    for bit in bin(e)[2:]:
        acc = _pmulmod(acc, acc, m)
        if bit == "1":
            acc = _pmulmod(acc, base, m)
    return acc


def _pgcd(a, b):
    a, b = _ptrim(list(a)), _ptrim(list(b))
    while b:
        a, b = b, _pmod(a, b)
    lead = pow(a[-1], -1, P)
    return [c * lead % P for c in a]


def _psub(a, b):
    n = max(len(a), len(b))
    return _ptrim([((a[i] if i < len(a) else 0) - (b[i] if i < len(b) else 0)) % P for i in range(n)])


def fp_roots(poly):
    """the roots in Fp of a polynomial (coefficients low to high)"""
    f = _ptrim([c % P for c in poly])
    g = _pgcd(f, _psub(_ppowmod([0, 1], P, f), [0, 1]))       # the product of the distinct linear factors
    rng = random.Random("lane-probe-roots")
    out, todo = [], [g]
    while todo:
        h = todo.pop()
        if len(h) == 1:
            continue
        if len(h) == 2:
            out.append(-h[0] * pow(h[1], -1, P) % P)
            continue
        while True:
            t = _psub(_ppowmod([rng.randrange(P), 1], (P - 1) // 2, h), [1])
            d = _pgcd(h, t) if t else h
            if 1 < len(d) < len(h):
                q = list(h)
                # h / d by long division
                quo = [0] * (len(h) - len(d) + 1)
                inv_lead = pow(d[-1], -1, P)
                for k in range(len(quo) - 1, -1, -1):
                    c = q[k + len(d) - 1] * inv_lead % P
                    quo[k] = c
                    for i in range(len(d)):
                        q[k + i] = (q[k + i] - c * d[i]) % P
                assert not _ptrim(q)
                todo += [d, quo]
                break
    return sorted(out)


def iso_rhs(x):
    return (x * x * x + o.ISO_A * x + o.ISO_B) % P


def iso_kernel_points():
    """the affine points of E'(Fp) in the kernel of the 11-isogeny: the roots of
    ISO_XDEN over Fp, each with both rational y"""
    if "kernel" not in _cache:
        pts = []
        for x in fp_roots(o.ISO_XDEN):
            y = o.fp_sqrt(iso_rhs(x))
            assert y is not None
            pts += [(x, y), (x, P - y)]
        _cache["kernel"] = pts
    return _cache["kernel"]


def sswu_exceptional_u():
    """u with Z^2 u^4 + Z u^2 = 0: 0 and the two roots of -1/Z"""
    t = o.fp_sqrt(-pow(o.ISO_Z, -1, P) % P)
    assert t is not None
    return [0, t, P - t]


# --- points ---------------------------------------------------------------------------------
def iso_points(n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        x = rng.randrange(P)
        y = o.fp_sqrt(iso_rhs(x))
        if y is not None:
            out.append((x, y if rng.random() < 0.5 else P - y))
    return out


def g1_curve_points(n, seed):
    """random points of E(Fp): with overwhelming probability outside G1"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        x = rng.randrange(P)
        y = o.fp_sqrt((x * x * x + 4) % P)
        if y is not None:
            out.append((x, y))
    return out


def g2_curve_points(n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        x = (rng.randrange(P), rng.randrange(P))
        y = o.f2_sqrt(o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.B2))
        if y is not None:
            out.append((x, y))
    return out


def g1_points(n, seed):
    rng = random.Random(seed)
    return [o.G1_GEN] + [o.ec_mul(o.FP, o.G1_GEN, rng.randrange(1, o.R)) for _ in range(n - 1)]


def g2_points(n, seed):
    rng = random.Random(seed)
    return [o.G2_GEN] + [o.ec_mul(o.FP2, o.G2_GEN, rng.randrange(1, o.R)) for _ in range(n - 1)]


ORDER3 = [(0, 2), (0, P - 2)]


class Fld:
    """the words of an element, its encodings and residues, for F = Fp and F = Fp2"""

    def __init__(self, two):
        self.two = two
        self.W = 24 if two else 12
        self.F = o.FP2 if two else o.FP
        self.zero, self.one = (o.F2_ZERO, o.F2_ONE) if two else (0, 1)

    def enc(self, v, rng):
        return enc2(v, rng) if self.two else enc(v, rng)

    def w(self, raw):
        return w2(raw) if self.two else words(raw)

    def mont(self, v):
        return mont2(v) if self.two else mont(v)

    def res_of(self, ws):
        return res2(v2(ws)) if self.two else res(val(ws))

    def below(self, ws, bound=2 * P):
        return all(val(ws[k:k + 12]) < bound for k in range(0, self.W, 12))

    def rnd(self, rng):
        return (rng.randrange(1, P), rng.randrange(P)) if self.two else rng.randrange(1, P)

    def mul(self, a, b):
        return self.F.mul(a, b)

    def M(self, v):
        return M2(v) if self.two else [M(v)]

    def fps(self, n):
        return [12 * i for i in range(n * self.W // 12)]


FP_, FP2_ = Fld(False), Fld(True)


def proj_words(K, pt, rng, z=None):
    """a projective representative (x z, y z, z) of an affine point (None: (0 : y : 0))"""
    z = K.rnd(rng) if z is None else z
    if pt is None:
        t = (K.zero, K.rnd(rng), K.zero)
    else:
        t = (K.mul(pt[0], z), K.mul(pt[1], z), z)
    return sum((K.w(K.enc(c, rng)) for c in t), [])


def proj_check(K, want, jacobian=False):
    """the result is the affine point `want` (None: Z = 0) in homogeneous or Jacobian coordinates, stored values"""
    def f(ws, what):
        assert K.below(ws[:K.W]) and K.below(ws[K.W:2 * K.W]) and K.below(ws[2 * K.W:]), what + ("bound",)
        X, Y, Z = (K.res_of(ws[k * K.W:(k + 1) * K.W]) for k in range(3))
        if want is None:
            assert Z == K.zero, what + ("Z is not 0",)
            return
        assert Z != K.zero, what + ("Z = 0",)
        zi = K.F.inv(Z)
        if jacobian:
            zi2 = K.F.sqr(zi)
            got = (K.F.mul(X, zi2), K.F.mul(Y, K.F.mul(zi2, zi)))
        else:
            got = (K.F.mul(X, zi), K.F.mul(Y, zi))
        assert got == want, what + ("point",)
    return ("fn", 3 * K.W, f)


def affine_items(K, want):
    """inf, x, y as proj_to_affine and the decoders leave them"""
    if want is None:
        return [("w", 1)] + ([("raw", 0), ("raw", 0), ("raw", ONE), ("raw", 0)] if K.two else [("raw", 0), ("raw", ONE)])
    return [("w", 0)] + K.M(K.mont(want[0])) + K.M(K.mont(want[1]))


# --- building the operations ------------------------------------------------------------------
def _build_fp(ops):
    st_pairs = fp_pairs(STORED_EDGES, 2 * P, "lane-fp-pairs")
    st_vals = fp_values(STORED_EDGES, 2 * P, "lane-fp-vals")
    two = {"fp_add": lambda a, b: [M(a + b)], "fp_sub": lambda a, b: [M(a - b)],
           "fp_add_nr": lambda a, b: [("raw", a + b), ],
           "fp_eq": lambda a, b: [("w", 1 if (a - b) % P == 0 else 0)]}
    for name, ref in two.items():
        op = Op(name, 24, 1 if name == "fp_eq" else 12, fps=(0, 12), cheap=True)
        pairs = list(st_pairs)
        if name == "fp_eq":
            pairs += [(a, _twin(a)) for a in st_vals[::5]] + [(a, a) for a in st_vals[1::7]]
        for a, b in pairs:
            items = ref(a, b)
            if name == "fp_add_nr":
                assert a + b < 4 * P
            op.add(words(a) + words(b), items, (hex(a), hex(b)))
        ops.append(op)
    one = {"fp_neg": lambda a: [("raw", 0 if a == 0 else 2 * P - a)], "fp_dbl": lambda a: [M(2 * a)],
           "fp_mul3": lambda a: [M(3 * a)], "fp_mul4": lambda a: [M(4 * a)], "fp_mul8": lambda a: [M(8 * a)],
           "fp_reduce_once": lambda a: [("raw", a - P if a >= P else a)],
           "fp_is_zero": lambda a: [("w", 1 if a in (0, P) else 0)],
           "fp_sqr": lambda a: [M(a * a * RINV)], "fp_from_mont": lambda a: [("raw", a * RINV % P)],
           "fp_lex_largest": lambda a: [("w", 1 if res(a) > (P - 1) // 2 else 0)]}
    half = [mont(v) for v in ((P - 1) // 2, (P + 1) // 2, P - 1, 1, 0)]
    for name, ref in one.items():
        op = Op(name, 12, 1 if name in ("fp_is_zero", "fp_lex_largest") else 12, fps=(0,), cheap=True)
        for a in st_vals + (half + [h + P for h in half] if name == "fp_lex_largest" else []):
            op.add(words(a), ref(a), hex(a))
        ops.append(op)
    sel = Op("fp_select", 25, 12, fps=(1, 13), cheap=True)
    for i, (a, b) in enumerate(st_pairs):
        c = (0, 1, 0xFFFFFFFF, 2)[i % 4]
        sel.add([c] + words(a) + words(b), [("raw", a if c else b)], i)
    ops.append(sel)
    mul = Op("fp_mul", 24, 12, fps=(0, 12), in_bound=1 << 384, cheap=True)
    chain = Op("fp_muld_chain", 24, 12, fps=(0, 12), in_bound=1 << 384, cheap=True)
    for a, b in fp_pairs(PRODUCT_EDGES, 1 << 384, "lane-fp-mul"):
        mul.add(words(a) + words(b), [M(a * b * RINV)], (hex(a), hex(b)))
        t = a * b * RINV % P
        chain.add(words(a) + words(b), [M(t * t * RINV * a * RINV)], (hex(a), hex(b)))
    ops += [mul, chain]
    wide = fp_values(PRODUCT_EDGES, 1 << 384, "lane-fp-wide")
    tm = Op("fp_to_mont", 12, 12, fps=(0,), in_bound=1 << 384, cheap=True)
    pk = Op("fp_pack28", 12, 26, fps=(0,), in_bound=1 << 384, cheap=True)
    cmp_ = Op("fp_raw_cmp", 12, 2, fps=(0,), in_bound=1 << 384, cheap=True)
    around = [(P - 1) // 2, (P + 1) // 2, (P - 1) // 2 - 1, (P + 1) // 2 + 1, P - 1, P + 1, P, 0, TOP]
    for k in range(12):        # (p - 1) / 2 and p with one word one above or below: every position of the borrow chain
        for base in ((P - 1) // 2, P):
            for d in (1, -1):
                w = words(base)
                w[k] = (w[k] + d) % (1 << 32)
                around.append(val(w))
    for a in wide:
        tm.add(words(a), [M(a * R)], hex(a))
        pk.add(words(a), [("words", [(a >> (28 * k)) & 0xFFFFFFF for k in range(14)]), ("raw", a)], hex(a))
    for a in around + wide:
        cmp_.add(words(a), [("w", 1 if a < P else 0), ("w", 1 if a > (P - 1) // 2 else 0)], hex(a))
    ops += [tm, pk, cmp_]


def _build_fp_heavy(ops):
    rng = random.Random("lane-fp-heavy")
    pw = Op("fp_pow_fixed", 13, 12, fps=(1,))
    vals = STORED_EDGES + [rng.randrange(2 * P) for _ in range(33)]
    i = 0
    for a in vals:
        for idx, e in enumerate(EXPONENTS):
            k = (idx + i) % len(EXPONENTS)          # neighbouring lanes take different exponents
            pw.add([k] + words(a), [M(mont(pow(res(a), EXPONENTS[k], P)))], (k, hex(a)))
            i += 1
    sq = Op("fp_sqrt", 12, 13, fps=(0,))
    n_sq = 0
    for j, a in enumerate(STORED_EDGES + [rng.randrange(2 * P) for _ in range(300)] + [0]):
        if j % 3 == 0 and j >= len(STORED_EDGES):
            a = enc(pow(res(a), 2, P), rng)         # a square for certain
        x = res(a)
        is_sq = pow(x, (P - 1) // 2, P) in (0, 1)
        n_sq += is_sq
        sq.add(words(a), [("w", 1 if is_sq else 0), M(mont(pow(x, (P + 1) // 4, P)))], hex(a))
    assert 100 < n_sq < len(sq.rows) - 80
    inv = Op("fp_inv", 12, 12, fps=(0,))
    rows, classes = inv_rows()
    for a, cl in zip(rows, classes):
        x = res(a)
        inv.add(words(a), [M(mont(pow(x, -1, P)) if x else 0)], (cl, hex(a)))
    inv2 = Op("fp2_inv", 24, 24, fps=(0, 12))
    for case in [[(0, 0)], [(P, 0)], [(0, P)], [(P, P)]] + fp2_values(1, STORED_EDGES, 2 * P, "lane-fp2-inv", 320):
        a = case[0]
        x = res2(a)
        inv2.add(w2(a), M2(mont2(o.f2_inv(x)) if x != (0, 0) else (0, 0)), (hex(a[0]), hex(a[1])))
    ops += [pw, sq, inv, inv2, _build_fp2_sqrt(rng)]


def fp2_sqrt_branch(x):
    """which path of sqrt(fp2) a residue takes: 'real', 'al-square', 'al-nonsquare' or 'none' (the norm is no square)"""
    if x[1] == 0:
        return "real"
    n = (x[0] * x[0] + x[1] * x[1]) % P
    s = pow(n, (P + 1) // 4, P)
    if s * s % P != n:
        return "none"
    al = (x[0] + s) * pow(2, -1, P) % P
    return "al-square" if pow(al, (P - 1) // 2, P) == 1 else "al-nonsquare"


def _build_fp2_sqrt(rng):
    op = Op("fp2_sqrt", 24, 25, fps=(0, 12))
    seen = {}
    cases = []
    for a0 in (0, 1, 4, 5, P - 1, P - 4, rng.randrange(P), rng.randrange(P), rng.randrange(P)):     # real: c1 = 0 and c1 = p
        cases += [(mont(a0), 0), (mont(a0), P), (mont(a0) + P, P)]
    for _ in range(150):
        x = (rng.randrange(P), rng.randrange(1, P))
        cases.append(enc2(o.f2_sqr(x), rng))      # a square
        cases.append(enc2(x, rng))                # a square or not
    for a in cases:
        x = res2(a)
        root = o.f2_sqrt(x)
        br = fp2_sqrt_branch(x)
        seen[(br, root is not None)] = seen.get((br, root is not None), 0) + 1

        def f(ws, what, x=x):
            r = v2(ws)
            assert r[0] < 2 * P and r[1] < 2 * P, what + ("bound",)
            assert o.f2_sqr(res2(r)) == x, what + ("not a root",)
        op.add(w2(a), [("w", 1), ("fn", 24, f)] if root is not None else [("w", 0), ("any", 24)], (br, hex(a[0]), hex(a[1])))
    for key in (("real", True), ("al-square", True), ("al-nonsquare", True), ("none", False)):
        assert seen.get(key, 0) >= 6, seen
    assert ("al-square", False) not in seen and ("al-nonsquare", False) not in seen
    return op


def _build_fp2(ops):
    def binary(name, ref, edges=STORED_EDGES, bound=2 * P, out_bound=2 * P, exact=False):
        op = Op(name, 48, 24, fps=(0, 12, 24, 36), in_bound=bound, cheap=True)
        for a, b in fp2_values(2, edges, bound, "lane-" + name):
            want = ref(a, b)
            if exact:
                assert want[0] < out_bound and want[1] < out_bound
                items = [("raw", want[0]), ("raw", want[1])]
            else:
                items = M2(want, out_bound)
            op.add(w2(a) + w2(b), items, (a, b))
        ops.append(op)
    binary("fp2_add", lambda a, b: (a[0] + b[0], a[1] + b[1]))
    binary("fp2_sub", lambda a, b: (a[0] - b[0], a[1] - b[1]))
    binary("fp2_add_nr", lambda a, b: (a[0] + b[0], a[1] + b[1]), out_bound=4 * P, exact=True)
    binary("fp2_add_xi_nr", lambda a, b: (a[0] + b[0] + 2 * P - b[1], a[1] + b[0] + b[1]), out_bound=6 * P, exact=True)
    rmul = lambda a, b, s=1: ((a[0] * b[0] - a[1] * b[1]) * s * RINV, (a[0] * b[1] + a[1] * b[0]) * s * RINV)   # noqa: E731
    binary("fp2_mul", rmul, PRODUCT_EDGES, 1 << 384)
    binary("fp2_mul_scaled2", lambda a, b: rmul(a, b, 2), PRODUCT_EDGES, 1 << 384)
    binary("fp2_mul_scaled3", lambda a, b: rmul(a, b, 3), PRODUCT_EDGES, 1 << 384)
    dot = Op("fp2_dot2", 96, 24, fps=range(0, 96, 12), in_bound=1 << 384, cheap=True)
    for a, b, c, d in fp2_values(4, PRODUCT_EDGES, 1 << 384, "lane-fp2-dot2"):
        x, y = rmul(a, b), rmul(c, d)
        dot.add(w2(a) + w2(b) + w2(c) + w2(d), M2((x[0] + y[0], x[1] + y[1])), None)
    ops.append(dot)

    def unary(name, ref, n_out=24, edges=STORED_EDGES, bound=2 * P, extra=()):
        op = Op(name, 24, n_out, fps=(0, 12), in_bound=bound, cheap=True)
        for case in [[e] for e in extra] + fp2_values(1, edges, bound, "lane-" + name):
            a = case[0]
            op.add(w2(a), ref(a), (hex(a[0]), hex(a[1])))
        ops.append(op)
    rneg = lambda v: 0 if v == 0 else 2 * P - v      # noqa: E731
    unary("fp2_neg", lambda a: [("raw", rneg(a[0])), ("raw", rneg(a[1]))])
    unary("fp2_conj", lambda a: [("raw", a[0]), ("raw", rneg(a[1]))])
    unary("fp2_mul_nr", lambda a: M2((a[0] - a[1], a[0] + a[1])))
    unary("fp2_sqr", lambda a: M2(rmul(a, a)), edges=PRODUCT_EDGES, bound=1 << 384)
    unary("fp2_is_zero", lambda a: [("w", 1 if a[0] % P == 0 and a[1] % P == 0 else 0)], n_out=1)
    half = [mont(v) for v in ((P - 1) // 2, (P + 1) // 2, 1, P - 1)]
    lex_extra = [(h + t0, c1) for h in half for t0 in (0, P) for c1 in (0, P)] + [(0, h) for h in half] + [(P, h + P) for h in half]
    unary("fp2_lex_largest", lambda a: [("w", 1 if o.f2_lex_largest(res2(a)) else 0)], n_out=1, extra=lex_extra)
    mfp = Op("fp2_mul_fp", 36, 24, fps=(0, 12, 24), in_bound=1 << 384, cheap=True)
    for a, b in fp2_values(2, PRODUCT_EDGES, 1 << 384, "lane-fp2-mul-fp"):
        mfp.add(w2(a) + words(b[0]), M2((a[0] * b[0] * RINV, a[1] * b[0] * RINV)), None)
    ops.append(mfp)
    eq = Op("fp2_eq", 48, 1, fps=(0, 12, 24, 36), cheap=True)
    cases = fp2_values(2, STORED_EDGES, 2 * P, "lane-fp2-eq")
    for i, (a, b) in enumerate(cases):
        if i % 4 == 1:
            b = (_twin(a[0]), a[1])
        elif i % 4 == 2:
            b = (_twin(a[0]), _twin(a[1]))
        elif i % 4 == 3 and i % 8 == 3:
            b = (a[0], (a[1] + 1) % (2 * P))
        same = (a[0] - b[0]) % P == 0 and (a[1] - b[1]) % P == 0
        eq.add(w2(a) + w2(b), [("w", 1 if same else 0)], i)
    ops.append(eq)


# --- hash to curve ------------------------------------------------------------------------------
def message_rows():
    """(length, start offset, the row's words, the message): every length of
    XMD_LENGTHS at every start offset 0..3, neighbours of different lengths"""
    if "msgs" not in _cache:
        rng = random.Random("lane-probe-messages")
        out = []
        for off in range(4):
            for k, ln in enumerate(XMD_LENGTHS):
                ln = XMD_LENGTHS[(k * 5 + off) % len(XMD_LENGTHS)]
                buf = bytearray(rng.randrange(256) for _ in range(4 * MSG_WORDS))
                msg = bytes(buf[off:off + ln])
                ws = [int.from_bytes(buf[4 * i:4 * i + 4], "little") for i in range(MSG_WORDS)]
                out.append((ln, off, [ln, off] + ws, msg))
        assert {(r[0], r[1]) for r in out} == {(ln, off) for ln in XMD_LENGTHS for off in range(4)}
        _cache["msgs"] = out
    return _cache["msgs"]


def xmd_ref(msg):
    """expand_message_xmd(msg, DST, 128) built on hashlib alone"""
    dst_prime = o.DST + bytes([len(o.DST)])
    b0 = hashlib.sha256(bytes(64) + msg + (128).to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    bs = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in (2, 3, 4):
        bs.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, bs[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(bs)


def _build_h2c(ops):
    rng = random.Random("lane-h2c")
    for name in ("xmd", "xmd_select"):
        op = Op(name, 253, 32)
        for ln, off, row, msg in message_rows():
            u = xmd_ref(msg)
            op.add(row, [("words", [int.from_bytes(u[4 * i:4 * i + 4], "big") for i in range(32)])], (ln, off))
        ops.append(op)
    be = Op("fp_from_be64_words", 16, 12)
    vals = [0, (1 << 512) - 1, 1, (1 << 384) - 1, 1 << 384, ((1 << 128) - 1) << 384, (1 << 512) - (1 << 384)]
    kmax = ((1 << 512) - 1) // P
    for k in (1, 2, 3, 1 << 64, (1 << 384) // P, (1 << 384) // P + 1, kmax // 2, kmax - 1, kmax):
        vals += [k * P + d for d in (-1, 0, 1) if k * P + d < 1 << 512]
    vals += [rng.randrange(1 << 128) << 384 for _ in range(6)] + [rng.randrange(1 << 384) for _ in range(6)]
    vals += [rng.randrange(1 << 512) for _ in range(280)]
    for v in vals:
        be.add([(v >> (32 * (15 - i))) & 0xFFFFFFFF for i in range(16)], [M(v % P * R)], hex(v))
    sg = Op("sgn0", 12, 1, fps=(0,))
    for a in fp_values(STORED_EDGES, 2 * P, "lane-sgn0", 300):
        sg.add(words(a), [("w", res(a) & 1)], hex(a))
    ops += [be, sg]

    sswu = Op("map_to_curve_sswu", 12, 36, fps=(0,))
    us = []
    for u in sswu_exceptional_u():
        us += [("exceptional", mont(u)), ("exceptional", mont(u) + P)]
    for _ in range(60):
        u = rng.randrange(1, P)
        us += [("u", mont(u)), ("-u", mont(P - u)), ("u+p", mont(u) + P), ("random", enc(rng.randrange(P), rng))]
    us += [("edge", v) for v in STORED_EDGES]
    for tag, a in us:
        want = o.map_to_curve_sswu(res(a))

        def f(ws, what, want=want):
            xn, xd, y = (val(ws[k:k + 12]) for k in (0, 12, 24))
            assert xn < 2 * P and xd < 2 * P and y < 2 * P, what + ("bound",)
            assert res(xd) != 0, what + ("xd = 0",)
            assert res(xn) * pow(res(xd), -1, P) % P == want[0] and res(y) == want[1], what + ("point",)
        sswu.add(words(a), [("fn", 36, f)], (tag, hex(a)))
    ops.append(sswu)

    pts = iso_points(24, "lane-iso-points")
    kern = iso_kernel_points()
    add = Op("iso_curve_add", 72, 36, fps=range(0, 72, 12))
    pairs = []
    for i, p in enumerate(pts):
        q = pts[(i * 7 + 3) % len(pts)]
        pairs += [(p, q), (p, p), (p, (p[0], P - p[1])), (p, None), (None, p)]
    pairs += [(None, None), (kern[0], kern[1]), (kern[0], kern[2]), (kern[0], pts[0]), (kern[3], kern[3])]
    for p, q in pairs:
        for z in (None, 1):
            add.add(proj_words(FP_, p, rng, z) + proj_words(FP_, q, rng, z),
                    [proj_check(FP_, o.ec_add(o.FP, p, q, o.ISO_A))], (p, q))
    iso = Op("iso_map_proj", 36, 36, fps=(0, 12, 24))
    for p in iso_points(150, "lane-iso-map") + pts:
        want = o.iso_map_g1(p)
        assert want is not None and o.on_curve(o.FP, want, 0, 4)
        iso.add(proj_words(FP_, p, rng), [proj_check(FP_, want)], p)
    for p in kern:              # the kernel: Z = 0, on two representatives each
        for z in (None, 1, None):
            iso.add(proj_words(FP_, p, rng, z), [proj_check(FP_, None)], ("kernel", p))
    cc = Op("clear_cofactor_g1", 24, 25, fps=(0, 12))
    for p in ORDER3 + g1_curve_points(12, 29) + g1_points(4, "lane-cc"):     # as test_clear_cofactor_jacobian
        for _ in range(2):
            cc.add(words(enc(p[0], rng)) + words(enc(p[1], rng)), affine_items(FP_, o.ec_mul(o.FP, p, o.H_EFF_G1)), p)
    ops += [add, iso, cc]
    for name in ("hash_to_g1", "hash_to_g1_parked"):
        op = Op(name, 253, 25)
        for ln, off, row, msg in message_rows():
            if ("h", msg) not in _cache:
                _cache[("h", msg)] = o.hash_to_g1(msg)
            op.add(row, affine_items(FP_, _cache[("h", msg)]), (ln, off))
        ops.append(op)


# --- curve ----------------------------------------------------------------------------------------
def _scalar_list():
    rng = random.Random(31)
    L = LAMBDA
    ks = [0, 1, 2, 3, L - 1, L, L + 1, L * L, L * L + L, 1 << 128, o.R - 1, o.R, o.R + 1, (1 << 256) - 1]      # test_g1_mul_glv
    ks += [2 * o.R - 1, 2 * o.R, 2 * o.R + 1, (1 << 255) - 1, 1 << 255]
    return ks + [rng.randrange(1 << 256) for _ in range(12)] + [rng.randrange(o.R) for _ in range(12)]


def _build_curve(ops, K, tag, sub_pts, off_pts, small):
    """the templated operations for F = Fp (tag g1) or Fp2 (g2); small: points of small order"""
    rng = random.Random("lane-curve-" + tag)
    F, W = K.F, K.W
    pts = sub_pts + off_pts + small
    neg = lambda p: o.ec_neg(F, p)      # noqa: E731
    pairs = []
    for i, p in enumerate(pts):
        q = pts[(i * 5 + 2) % len(pts)]
        pairs += [(p, q), (p, p), (p, neg(p)), (p, None), (None, p)]
    pairs.append((None, None))
    dbl = Op(tag + "_proj_dbl", 3 * W, 3 * W, fps=K.fps(3))
    for p in pts + [None]:
        for z in (None, 1, None):
            dbl.add(proj_words(K, p, rng, K.one if z else None), [proj_check(K, o.ec_add(F, p, p))], p)
    add = Op(tag + "_proj_add", 6 * W, 3 * W, fps=K.fps(6))
    eq = Op(tag + "_proj_eq", 6 * W, 1, fps=K.fps(6))
    mixed = Op(tag + "_proj_add_mixed", 5 * W, 3 * W, fps=K.fps(5))
    for p, q in pairs:
        for z in (None, K.one):
            add.add(proj_words(K, p, rng, z) + proj_words(K, q, rng, z), [proj_check(K, o.ec_add(F, p, q))], (p, q))
            eq.add(proj_words(K, p, rng, z) + proj_words(K, q, rng, z), [("w", 1 if p == q else 0)], (p, q))
            if q is not None:
                mixed.add(proj_words(K, p, rng, z) + K.w(K.enc(q[0], rng)) + K.w(K.enc(q[1], rng)),
                          [proj_check(K, o.ec_add(F, p, q))], (p, q))
    aff = Op(tag + "_proj_to_affine", 3 * W, 1 + 2 * W, fps=K.fps(3))
    for p in pts + [None, None]:
        for _ in range(2):
            aff.add(proj_words(K, p, rng), affine_items(K, p), p)
    ks = [0, 1, 2, 3, X_ABS, o.H_EFF_G1, (1 << 64) - 1, 1 << 63, 0x8000000000000001] + [rng.getrandbits(64) for _ in range(6)]
    mul, mulm = Op(tag + "_proj_mul_u64", 3 * W + 2, 3 * W, fps=K.fps(3)), Op(tag + "_proj_mul_u64_mixed", 2 * W + 2, 3 * W, fps=K.fps(2))
    for i, k in enumerate(ks):
        for p in (pts[i % len(pts)], small[i % len(small)], None):
            want = o.ec_mul(F, p, k)
            kw = [k & 0xFFFFFFFF, k >> 32]
            mul.add(proj_words(K, p, rng) + kw, [proj_check(K, want)], (p, hex(k)))
            if p is not None:
                mulm.add(K.w(K.enc(p[0], rng)) + K.w(K.enc(p[1], rng)) + kw, [proj_check(K, want)], (p, hex(k)))
    ops += [dbl, add, mixed, eq, aff, mul, mulm]


def psi(q):
    """the untwist-Frobenius-twist endomorphism of E'(Fp2), from the oracle's Fp2 alone"""
    cx = o.f2_inv(o.f2_pow((1, 1), (P - 1) // 3))
    cy = o.f2_inv(o.f2_pow((1, 1), (P - 1) // 2))
    return (o.f2_mul(o.f2_conj(q[0]), cx), o.f2_mul(o.f2_conj(q[1]), cy))


def _be_words(b):
    return [int.from_bytes(b[4 * i:4 * i + 4], "big") for i in range(len(b) // 4)]


def _decode_want(K, fn, b):
    try:
        pt = fn(b)
    except o.Invalid:
        return [("w", 0), ("any", 1 + 2 * K.W)]
    return [("w", 1)] + affine_items(K, pt)


def _build_g1(ops):
    rng = random.Random("lane-g1")
    sub, off = g1_points(5, "lane-g1-sub"), g1_curve_points(4, "lane-g1-off")
    _build_curve(ops, FP_, "g1", sub, off, ORDER3)
    e2 = lambda p: words(enc(p[0], rng)) + words(enc(p[1], rng))      # noqa: E731
    ks = _scalar_list()
    sm = Op("g1_proj_mul_scalar_mixed", 32, 36, fps=(0, 12))
    sr, sp, glv = Op("sub_r_if_ge", 8, 8), Op("glv_split", 8, 8), Op("g1_mul_glv", 32, 36, fps=(0, 12))
    for i, k in enumerate(ks):
        p = (sub + off + ORDER3)[i % 11]
        sm.add(e2(p) + words(k, 8), [proj_check(FP_, o.ec_mul(o.FP, p, k))], (p, hex(k)))
        sr.add(words(k, 8), [("words", words(k - o.R if k >= o.R else k, 8))], hex(k))
        k2, k1 = divmod(k % o.R, LAMBDA)
        assert k1 + k2 * LAMBDA == k % o.R and k2 < 1 << 128
        sp.add(words(k, 8), [("words", words(k1, 4) + words(k2, 4))], hex(k))
        p = sub[i % len(sub)]
        glv.add(e2(p) + words(k, 8), [proj_check(FP_, o.ec_mul(o.FP, p, k % o.R))], (p, hex(k)))
    g32 = Op("g1_mul_glv32", 26, 36, fps=(0, 12))
    r37 = random.Random(37)
    ab = [(1, 0), (3, 0), (1, 1), (3, 3), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0xFFFFFFFF), (0xFFFFFFFF, 0),
          (0x80000001, 0x40000000), (5, 2)] + [(r37.getrandbits(32) | 1, r37.getrandbits(32)) for _ in range(10)]     # test_g1_mul_glv32
    for i, (a, b) in enumerate(ab):
        p = sub[i % len(sub)]
        g32.add(e2(p) + [a, b], [proj_check(FP_, o.ec_mul(o.FP, p, (a - b * X_ABS * X_ABS) % o.R))], (hex(a), hex(b)))
    jd, ja = Op("jac_dbl", 36, 36, fps=(0, 12, 24)), Op("jac_add_mixed", 60, 36, fps=range(0, 60, 12))

    def jac_words(p, z=None):
        z = rng.randrange(1, P) if z is None else z
        if p is None:
            t = (rng.randrange(1, P), rng.randrange(1, P), 0)
        else:
            t = (p[0] * z * z % P, p[1] * z * z * z % P, z)
        return sum((words(enc(c, rng)) for c in t), [])
    pts = sub + off + ORDER3
    for i, p in enumerate(pts + [None]):
        for z in (None, 1):
            jd.add(jac_words(p, z), [proj_check(FP_, o.ec_add(o.FP, p, p), jacobian=True)], p)
        if p is None:
            continue
        q = pts[(i * 3 + 1) % len(pts)]
        for t, want in ((q, o.ec_add(o.FP, q, p) if q[0] != p[0] else None), (p, None), (o.ec_neg(o.FP, p), None), (None, None)):
            # T = +-Q and T = O are the exceptional inputs: Z = 0 must come out
            for z in (None, 1):
                ja.add(jac_words(t, z) + e2(p), [proj_check(FP_, want, jacobian=True)], (t, p))
    tf = Op("g1_is_torsion_free", 24, 2, fps=(0, 12))
    for p in g1_points(8, "lane-g1-tf") + g1_curve_points(8, "lane-g1-tf-off") + ORDER3:
        want = 1 if o.g1_in_subgroup(p) else 0
        for _ in range(2):
            tf.add(e2(p), [("w", want), ("w", want)], p)
    assert {it[0][1] for it in tf.items} == {0, 1}
    dec = Op("g1_decompress", 12, 26)
    good, offg = sub[1], off[0]
    y2 = lambda x: (x * x * x + 4) % P      # noqa: E731
    x_off = next(x for x in range(2, 100) if o.fp_sqrt(y2(x)) is None)
    xs = [0, good[0], x_off, offg[0], P - 1, P, P + 5, (1 << 381) - 1]
    for x in xs:
        for flags in range(8):
            b = bytearray(x.to_bytes(48, "big"))
            assert b[0] < 0x20
            b[0] |= flags << 5
            dec.add(_be_words(bytes(b)), _decode_want(FP_, o.g1_from_compressed, bytes(b)), (hex(x), flags))
    comp = Op("g1_compress", 25, 12, fps=(1, 13))
    for p in sub + [o.ec_neg(o.FP, q) for q in sub] + [None]:
        b = o.g1_to_compressed(p)
        dec.add(_be_words(b), _decode_want(FP_, o.g1_from_compressed, b), ("round trip", p))
        for _ in range(2):
            xy = e2(p) if p else words(0) + words(ONE)
            comp.add([0 if p else 1] + xy, [("words", [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(12)])], p)
    assert sum(1 for it in dec.items if it[0][1] == 1) >= 12
    ops += [sm, sr, sp, glv, g32, jd, ja, tf, dec, comp]


def _build_g2(ops):
    rng = random.Random("lane-g2")
    sub, off = g2_points(4, "lane-g2-sub"), g2_curve_points(3, "lane-g2-off")
    _build_curve(ops, FP2_, "g2", sub, off, off[:1])
    e2 = lambda p: w2(enc2(p[0], rng)) + w2(enc2(p[1], rng))      # noqa: E731
    tf = Op("g2_is_torsion_free", 48, 1, fps=range(0, 48, 12))
    psi_op = Op("g2_psi_is_neg_proj", 120, 1, fps=range(0, 120, 12))
    for q in sub + off + g2_points(3, "lane-g2-tf") + g2_curve_points(3, "lane-g2-tf-off"):
        ins = o.g2_in_subgroup(q)
        t = o.ec_mul(o.FP2, q, X_ABS)
        assert (psi(q) == o.ec_neg(o.FP2, t)) == ins
        for _ in range(2):
            tf.add(e2(q), [("w", 1 if ins else 0)], q)
            psi_op.add(e2(q) + proj_words(FP2_, t, rng), [("w", 1 if ins else 0)], ("T", q))
        psi_op.add(e2(q) + proj_words(FP2_, t, rng, o.F2_ONE), [("w", 1 if ins else 0)], ("T, Z = 1", q))
        psi_op.add(e2(q) + proj_words(FP2_, None, rng), [("w", 0)], ("Z = 0", q))
        psi_op.add(e2(q) + proj_words(FP2_, o.ec_neg(o.FP2, t), rng), [("w", 0)], ("-T", q))
        psi_op.add(e2(q) + proj_words(FP2_, o.ec_add(o.FP2, t, q), rng), [("w", 0)], ("T + Q", q))
    dec = Op("g2_decompress", 25, 50)
    good, offg = sub[1], off[0]
    rhs = lambda x: o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.B2)      # noqa: E731
    x_off = next((c, 1) for c in range(2, 100) if o.f2_sqrt(rhs((c, 1))) is None)
    xs = [(0, 0), good[0], x_off, offg[0], (P - 1, P - 1), (P, 1), (1, P), (P + 5, 2), (2, P + 5), ((1 << 381) - 1, 3),
          (3, (1 << 381) - 1), (5, 0), (0, 5)]

    def g2_want(b, subgroup):
        if subgroup:
            return _decode_want(FP2_, o.g2_from_compressed, b)
        saved = o.g2_in_subgroup
        o.g2_in_subgroup = lambda pt: True      # the oracle's decoder without its subgroup check
        try:
            return _decode_want(FP2_, o.g2_from_compressed, b)
        finally:
            o.g2_in_subgroup = saved
    for x in xs:
        for flags in range(8):
            if x[1] >> 381:
                continue
            b = bytearray(x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
            b[0] |= flags << 5
            for sg in ((1, 0) if flags in (4, 5) else (1,)):
                dec.add([sg] + _be_words(bytes(b)), g2_want(bytes(b), sg), (x, flags, sg))
    comp = Op("g2_compress", 49, 24, fps=range(1, 49, 12))
    for p in sub + [o.ec_neg(o.FP2, q) for q in sub] + [None]:
        b = o.g2_to_compressed(p)
        for sg in (1, 0):
            dec.add([sg] + _be_words(b), g2_want(b, sg), ("round trip", sg))
        for _ in range(2):
            xy = e2(p) if p else w2((0, 0)) + w2((ONE, 0))
            comp.add([0 if p else 1] + xy, [("words", [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(24)])], p)
    assert sum(1 for it in dec.items if it[0][1] == 1) >= 12
    ops += [tf, psi_op, dec, comp]


# --- line steps -----------------------------------------------------------------------------------
def f2_muli(a, k):
    return (a[0] * k % P, a[1] * k % P)


def line_double(r):
    """pairing.hpp doubling_step's documented formulas over the oracle's Fp2: (c0, c1, c2), the new R"""
    X, Y, Z = r
    B, C = o.f2_sqr(Y), o.f2_sqr(Z)
    E = f2_muli(o.f2_mul_nr(C), 12)
    F = f2_muli(E, 3)
    H = f2_muli(o.f2_mul(Y, Z), 2)
    J = o.f2_sqr(X)
    A2 = o.f2_mul(X, Y)
    nx = f2_muli(o.f2_mul(A2, o.f2_sub(B, F)), 2)
    ny = o.f2_sub(o.f2_sqr(o.f2_add(B, F)), f2_muli(o.f2_sqr(E), 12))
    nz = f2_muli(o.f2_mul(B, H), 4)
    return (H, o.f2_neg(f2_muli(J, 3)), o.f2_sub(B, E)), (nx, ny, nz)


def line_add(r, q):
    """addition_step's documented formulas"""
    X, Y, Z = r
    th = o.f2_sub(Y, o.f2_mul(q[1], Z))
    la = o.f2_sub(X, o.f2_mul(q[0], Z))
    D = o.f2_sqr(la)
    E3 = o.f2_mul(la, D)
    G = o.f2_mul(X, D)
    H = o.f2_sub(o.f2_add(E3, o.f2_mul(Z, o.f2_sqr(th))), f2_muli(G, 2))
    nr = (o.f2_mul(la, H), o.f2_sub(o.f2_mul(th, o.f2_sub(G, H)), o.f2_mul(Y, E3)), o.f2_mul(Z, E3))
    return (la, o.f2_neg(th), o.f2_sub(o.f2_mul(th, q[0]), o.f2_mul(la, q[1]))), nr


def prepare_lines(q):
    """the 68 lines of g2_prepare and T = [|x|]Q (projective), by the formulas above"""
    r, lines = (q[0], q[1], o.F2_ONE), []
    for b in range(61, -1, -1):
        c, r = line_double(r)
        lines.append(c)
        if b in (61, 59, 56, 47, 15):
            c, r = line_add(r, q)
            lines.append(c)
    c, r = line_double(r)
    lines.append(c)
    assert len(lines) == N_LINES
    return lines, r


def _m6(vals):
    return sum((M2(mont2(v)) for v in vals), [])


def _build_lines(ops):
    rng = random.Random("lane-lines")
    e2 = lambda a: w2(enc2(a, rng))      # noqa: E731
    rf2 = lambda: (rng.randrange(P), rng.randrange(P))      # noqa: E731
    keys = g2_points(3, "lane-lines-keys") + g2_curve_points(1, "lane-lines-off")
    dbl, add = Op("doubling_step", 72, 288, fps=range(0, 72, 12)), Op("addition_step", 120, 288, fps=range(0, 120, 12))
    trip = []
    for q in keys:
        for k in (1, 2, 3, X_ABS >> 40):
            t = o.ec_mul(o.FP2, q, k)
            z = rf2()
            trip.append(((o.f2_mul(t[0], z), o.f2_mul(t[1], z), z), q))
    trip += [((rf2(), rf2(), rf2()), (rf2(), rf2())) for _ in range(30)]
    trip += [((o.F2_ZERO, rf2(), o.F2_ZERO), (rf2(), rf2())), ((rf2(), o.F2_ZERO, rf2()), (rf2(), rf2()))]
    for r, q in trip:
        c, nr = line_double(r)
        dbl.add(sum((e2(v) for v in r), []), _m6(c + nr) * 2, None)
        c, nr = line_add(r, q)
        add.add(sum((e2(v) for v in r + q), []), _m6(c + nr) * 2, None)
    nl = Op("normalize_line", 72, 72, fps=range(0, 72, 12))
    for _ in range(40):
        c0, c1, c2 = rf2(), rf2(), (rng.randrange(P), rng.randrange(1, P))
        i2 = o.f2_inv(c2)
        nl.add(e2(c0) + e2(c1) + e2(c2), M2(mont2(o.f2_mul(c0, i2))) + M2(mont2(o.f2_mul(c1, i2))) + [("raw", ONE), ("raw", 0)], None)
    nls = Op("normalize_lines", 72 * N_LINES, 1 + 96 * N_LINES, fps=range(0, 72 * N_LINES, 12))
    tables = [[tuple(c) for c in prepare_lines(q)[0]] for q in keys[:2]]
    tables += [[(rf2(), rf2(), rf2()) for _ in range(N_LINES)] for _ in range(3)]
    for t in tables:
        assert all(c[2] != o.F2_ZERO for c in t)
        raw = [[enc2(v, rng) for v in c] for c in t]
        row = sum((w2(v) for c in raw for v in c), [])
        items = [("w", 1)]
        for c in t:
            i2 = o.f2_inv(c[2])
            items += M2(mont2(o.f2_mul(c[0], i2))) + M2(mont2(o.f2_mul(c[1], i2))) + [("raw", ONE), ("raw", 0)]
        nls.add(row, items + [("any", 24 * N_LINES)], "no zero")
    for j, (line, zero) in enumerate([(ln, z) for ln in (0, 33, 67) for z in ((0, 0), (P, P), (0, P), (P, 0))]):
        t = tables[j % len(tables)]
        raw = [[enc2(v, rng) for v in c] for c in t]
        raw[line][2] = zero      # a zero c2: false, every line left bit for bit as it was
        row = sum((w2(v) for c in raw for v in c), [])
        nls.add(row, [("w", 0), ("words", row), ("any", 24 * N_LINES)], ("zero c2", line, zero))
    prep = Op("g2_prepare_lds", 48, 72 * N_LINES + 72, fps=range(0, 48, 12))
    for q in keys:
        lines, t = prepare_lines(q)
        want = o.ec_mul(o.FP2, q, X_ABS)
        zi = o.f2_inv(t[2])
        assert (o.f2_mul(t[0], zi), o.f2_mul(t[1], zi)) == want
        for _ in range(2):
            prep.add(e2(q[0]) + e2(q[1]), _m6([v for c in lines for v in c]) + [proj_check(FP2_, want)], q)
    ops += [dbl, add, nl, nls, prep]


def ops():
    """every operation with its table, in the probe's order"""
    if "ops" not in _cache:
        out = []
        _build_fp(out)
        _build_fp2(out)
        _build_fp_heavy(out)
        _build_h2c(out)
        _build_g1(out)
        _build_g2(out)
        _build_lines(out)
        for op in out:
            op.fill()
            op.contract()
        _cache["ops"] = out
    return _cache["ops"]


def get_op(name):
    return next(op for op in ops() if op.name == name)


def listed_in_source(text):
    """{name: (n_in, n_out)} of the probe's X-macro lists, in order; the device-only names"""
    import re
    body = text[text.index("#define LP_OPS_0(X)"):text.index("namespace lp")]
    listed = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"X\((\w+), (\d+), (\d+), \d\)", body)}
    lds = body[body.index("#define LP_LDS_OPS_3"):]
    return listed, [m.group(1) for m in re.finditer(r"X\((\w+), (\d+), (\d+), \d\)", lds)]


def _source_names():
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe", "lane_probe.hip")) as f:
        return listed_in_source(f.read())


OP_NAMES = list(_source_names()[0])        # the probe's X-macro entries (soa_layout has a signature of its own)
HOST_OP_NAMES = [n for n in OP_NAMES if n not in DEVICE_ONLY]


def active_mask(n, half):
    """all lanes live, or lanes i mod 4 in {1, 2} switched off"""
    return [0 if half and i % 4 in (1, 2) else 1 for i in range(n)]


def run(call, op, n, active):
    """lanes 0..n of op through call(name, n, active, in, out), which returns a
    status; the (n, n_out) results, rows of inactive lanes still holding the poison"""
    import ctypes

    import numpy as np
    inp = np.array(op.rows[:n], dtype=np.uint32).reshape(n, op.n_in)
    out = np.full((n, op.n_out), POISON, dtype=np.uint32)
    act = np.array(active, dtype=np.uint8)
    assert len(act) == n
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    return call(op.name, n, p(act), p(inp), p(out)), out


# --- soa.hpp: the one entry with a buffer shared by all lanes ------------------------------------
SOA_IN, SOA_OUT, SOA_ROWS, SOA_TAB, SOA_FILL = 72, 252, 324, 144, 0xA5A5A5A5


def soa_case(n):
    """n coefficient triples (72 words each), the 2-line uniform table, a stride larger than n"""
    import numpy as np
    rng = random.Random("lane-soa-%d" % n)
    rows = np.array([[rng.getrandbits(32) for _ in range(SOA_IN)] for _ in range(n)], dtype=np.uint32)
    rows[0, :] = 0xFFFFFFFF
    tab = np.array([rng.getrandbits(32) for _ in range(SOA_TAB)], dtype=np.uint32)
    return rows, tab, n + 7


def soa_run(call_soa, n, active):
    """call_soa(n, stride, active, in, slots, tab, out) -> status; returns status, rows, tab, stride, out, slots"""
    import ctypes

    import numpy as np
    rows, tab, stride = soa_case(n)
    out = np.full((n, SOA_OUT), POISON, dtype=np.uint32)
    slots = np.full(SOA_ROWS * stride, SOA_FILL, dtype=np.uint32)
    act = np.array(active, dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    status = call_soa(n, stride, p(act), p(rows), p(slots), p(tab), p(out))
    return status, rows, tab, stride, out, slots


def soa_check(rows, tab, stride, active, out, slots):
    """rows land where soa.hpp's comments say -- word k of an Fp at row k, an
    Fp2's c1 12 rows below its c0, word 4q + e of line k's triple in uint4 row
    18 k + q (st_coeff4) and 18 k + 6 j + q (st_coeff4_one) -- the loads read
    them back, and nothing is written outside the live columns or in line 0"""
    import numpy as np
    n = len(rows)
    want = np.full(SOA_ROWS * stride, SOA_FILL, dtype=np.uint32)
    a = want[:12 * stride].reshape(12, stride)
    b = want[12 * stride:36 * stride].reshape(24, stride)
    c = want[36 * stride:180 * stride].reshape(36, stride, 4)
    d = want[180 * stride:].reshape(36, stride, 4)
    for i in range(n):
        if not active[i]:
            assert (out[i] == POISON).all(), ("soa_layout", n, i, "an inactive lane's result was written")
            continue
        a[:, i] = rows[i, :12]
        b[:, i] = rows[i, 24:48]
        c[18:, i, :] = rows[i].reshape(18, 4)
        d[18:, i, :] = rows[i].reshape(18, 4)
        expect = np.concatenate([rows[i, :12], rows[i, 24:48], rows[i], rows[i], tab[72 * (i & 1):72 * (i & 1) + 72]])
        assert (out[i] == expect).all(), ("soa_layout", n, i)
    assert (slots == want).all(), ("soa_layout", n, "slots", np.nonzero(slots != want)[0][:8])


def check_lanes(op, out, active):
    for i, live in enumerate(active):        # every lane is compared
        if not live:
            assert (out[i] == POISON).all(), (op.name, len(active), i, "an inactive lane's result was written")
            continue
        op.check(i, out[i])
