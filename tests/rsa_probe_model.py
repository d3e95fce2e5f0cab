"""Operand tables and the integer model of the RSA Montgomery primitives
(cess_amd/csrc/k_rsa.hpp: mont<L, SQR>, canon, to_words; rsa_mont.hpp:
mont_rt), for the host build (tests/test_rsa_primitives.py) and the GPU probe
(tests/test_gpu_rsa_primitives.py).

Plain Python integers.  R = 2^(28 L) and ninv = -n^-1 mod 2^28 are computed
here, never taken from the code under test.  The tables hold the limb patterns
that random RSA keys never produce: all-ones and mostly-zero moduli, both
extremes of ninv, single-limb moduli, every fill of the top limb, operands at
the ends of the [0, 2n) contract and with every limb 0x0fffffff.

What a result must satisfy (check_mont / check_canon / check_words):
  * mont: the exact residue a b R^-1 mod n, the range < 2n, every limb
    <= 0x0fffffff (the top limb included; mont_rt: and a zero carry word);
    a multiply by one gives a result <= n
  * canon: the same residue, < n
  * to_words: the same integer in 32-bit words"""
import random

M28 = (1 << 28) - 1
POISON = 0xDEADBEEF
LANE_COUNTS = (1, 65, 257)        # one lane; a wave and a lane; a block and a lane
BIG_ROWS = 8                      # rsa.hpp RSA_BIG_ROWS
MAX_BITS = 4096


class Class:
    """one size class: L 28-bit limbs; loop: the run-time form (mont_rt)"""

    def __init__(self, name, L, loop):
        self.name, self.L, self.loop = name, L, loop
        self.R = 1 << (28 * L)
        # the largest modulus the host sends here (host_rsa.cpp
        # size_class_limbs): bits + 2 <= 28 L and 8 k <= 28 L; the loop form
        # takes the least multiple of RSA_BIG_ROWS with 28 L >= 8 k + 2
        if loop:
            k = min((28 * L - 2) // 8, MAX_BITS // 8)
            self.max_bits = 8 * k
        else:
            self.max_bits = max(b for b in range(28 * L - 1 - 8, 28 * L - 1) if self.holds_bits(b))

    def holds_bits(self, bits):
        k = (bits + 7) // 8
        if self.loop:
            return 8 * k + 2 <= 28 * self.L and bits <= MAX_BITS
        return bits + 2 <= 28 * self.L and 8 * k <= 28 * self.L

    def holds(self, n):
        return n >= 3 and n & 1 and self.holds_bits(n.bit_length())


CLASSES = [Class("L37", 37, False), Class("L74", 74, False),
           Class("rt80", 80, True), Class("rt88", 88, True), Class("rt152", 152, True)]


def get_class(name):
    return next(c for c in CLASSES if c.name == name)


def size_class_limbs(bits, k):
    """host_rsa.cpp size_class_limbs, restated"""
    for L in (37, 74):
        if bits + 2 <= 28 * L and 8 * k <= 28 * L:
            return L
    L0 = (8 * k + 2 + 27) // 28
    return (L0 + BIG_ROWS - 1) // BIG_ROWS * BIG_ROWS if L0 <= 147 else 0


def ninv_of(n):
    return (-pow(n, -1, 1 << 28)) % (1 << 28)


def limbs(v, L):
    assert 0 <= v < 1 << (28 * L)
    return [(v >> (28 * i)) & M28 for i in range(L)]


def from_limbs(ws):
    return sum(int(w) << (28 * i) for i, w in enumerate(ws))


def all_ones_below(bound):
    """the largest 2^j - 1 below `bound`: every limb 0x0fffffff up to a partial top"""
    j = bound.bit_length()
    v = (1 << j) - 1
    return v if v < bound else (1 << (j - 1)) - 1


def moduli(c):
    """[(tag, n)]: the structured and random moduli of class c, all odd and
    within what the host sends to the class"""
    rng = random.Random("rsa-probe-moduli-" + c.name)
    top = c.max_bits
    out = [("all_ones", (1 << top) - 1),
           ("top_and_one", (1 << (top - 1)) + 1)]
    alt = sum(M28 << (28 * i) for i in range(0, c.L, 2)) & ((1 << top) - 1)
    out.append(("alternating", alt))
    rest = lambda: (rng.getrandbits(top) | (1 << (top - 1))) >> 28 << 28   # noqa: E731
    out.append(("low_limb_one", rest() | 1))
    out.append(("low_limb_ones", rest() | M28))
    out += [("three", 3), ("one_limb_ones", M28), ("limb_boundary", (1 << 28) + 1)]
    for j in range(28):       # every residue of bits mod 28, near the class top
        bits = top - j
        out.append(("top_fill_%d" % (bits % 28), rng.getrandbits(bits) | (1 << (bits - 1)) | 1))
    lo = 2049 if c.loop else 29
    for j in range(4):
        bits = rng.randrange(lo, top + 1)
        out.append(("random_%d" % j, rng.getrandbits(bits) | (1 << (bits - 1)) | 1))
    for tag, n in out:
        assert c.holds(n), (c.name, tag)
    return out


def operands(c, n, rng):
    """the edge values of the [0, 2n) contract, then random ones"""
    vals = [0, 1, 2, n - 1, n, n + 1, 2 * n - 1, c.R % n, c.R * c.R % n, all_ones_below(2 * n),
            rng.randrange(n), rng.randrange(2 * n)]
    assert all(0 <= v < 2 * n for v in vals)
    return vals


N_EDGE_MODULI = 8        # the moduli that get the full cross of operands


class Row:
    __slots__ = ("tag", "n", "a", "b")

    def __init__(self, tag, n, a, b):
        self.tag, self.n, self.a, self.b = tag, n, a, b


_tables = {}


def table(c, kind):
    """rows of class c for kind in mul / sqr / canon / words.  mul: both
    operand orders; sqr: a = b; canon and words: a alone."""
    key = (c.name, kind)
    if key in _tables:
        return _tables[key]
    rng = random.Random("rsa-probe-rows-%s" % c.name)
    rows = []
    for mi, (tag, n) in enumerate(moduli(c)):
        vals = operands(c, n, rng)
        if kind == "mul":
            if mi < N_EDGE_MODULI:
                pairs = [(a, b) for a in vals for b in vals]
            else:
                pairs = []
                for i, a in enumerate(vals):
                    b = vals[(i + 1 + mi) % len(vals)]
                    pairs += [(a, b), (b, a)]
                pairs += [(2 * n - 1, 2 * n - 1), (vals[9], vals[9])]
            rows += [Row(tag, n, a, b) for a, b in pairs]
        elif kind == "sqr":
            rows += [Row(tag, n, a, a) for a in vals]
        elif kind == "canon":
            rows += [Row(tag, n, a, 0) for a in vals]
        elif kind == "words":
            rows += [Row(tag, n, a, 0) for a in vals + [c.R - 1]]
        else:
            raise KeyError(kind)
    _tables[key] = rows
    return rows


def interleaved(rows):
    """the same rows with neighbours from different moduli: row i of the
    result is taken round-robin over the moduli, so that adjacent GPU lanes
    hold different moduli and different operands"""
    groups = {}
    for r in rows:
        groups.setdefault(r.n, []).append(r)
    lists = list(groups.values())
    out, i = [], 0
    while len(out) < len(rows):
        for g in lists:
            if i < len(g):
                out.append(g[i])
        i += 1
    return out


def active_mask(n, half):
    """all lanes live, or lanes i mod 4 in {1, 2} switched off"""
    return [0 if half and i % 4 in (1, 2) else 1 for i in range(n)]


# --- what a result must satisfy --------------------------------------------------
def check_mont(c, row, out, what=""):
    """out: the L result limbs (loop form: L + 1 words, carry word last)"""
    ctx = (c.name, what, row.tag, hex(row.a)[:20], hex(row.b)[:20])
    assert all(0 <= int(w) <= M28 for w in out), ctx + ("a limb above 0x0fffffff",)
    if c.loop:
        assert len(out) == c.L + 1 and int(out[c.L]) == 0, ctx + ("carry word",)
    got = from_limbs(out)
    n = row.n
    assert got < 2 * n, ctx + ("not below 2n",)
    assert got % n == row.a * row.b * pow(c.R, -1, n) % n, ctx + ("residue",)
    if row.a == 1 or row.b == 1:
        assert got <= n, ctx + ("a multiply by one above n",)
    return got


def check_canon(c, row, out):
    ctx = (c.name, "canon", row.tag, hex(row.a)[:20])
    assert all(0 <= int(w) <= M28 for w in out), ctx
    got = from_limbs(out)
    assert got < row.n and got == row.a % row.n, ctx


def check_words(c, row, out):
    W = (28 * c.L + 31) // 32
    assert len(out) == W
    assert sum(int(w) << (32 * j) for j, w in enumerate(out)) == row.a, (c.name, "to_words", row.tag, hex(row.a)[:20])


# --- the probe's operations (tests/probe/rsa_probe.hip) ----------------------------
class Op:
    """entry: the probe library's rp_<entry>; kind: the table; uni: the key
    row is read through a wave-uniform index (one modulus per wave)"""

    def __init__(self, entry, cls, kind, sqr=False, uni=False):
        self.entry, self.cls, self.kind, self.sqr, self.uni = entry, cls, kind, sqr, uni
        self.name = entry if not cls.loop else "%s_%s" % (entry, cls.name)

    @property
    def rows(self):
        return table(self.cls, self.kind)

    @property
    def n_out(self):
        c = self.cls
        return (28 * c.L + 31) // 32 if self.kind == "words" else c.L + 1 if c.loop else c.L

    def check(self, row, out):
        if self.kind in ("mul", "sqr"):
            check_mont(self.cls, row, out, self.entry)
        elif self.kind == "canon":
            check_canon(self.cls, row, out)
        else:
            check_words(self.cls, row, out)


def ops():
    out = []
    for c in CLASSES:
        if c.loop:
            out.append(Op("mont_rt", c, "mul"))
            continue
        for uni in (False, True):
            u = "u" if uni else ""
            out.append(Op("mont%d%s" % (c.L, u), c, "mul", False, uni))
            out.append(Op("sqr%d%s" % (c.L, u), c, "sqr", True, uni))
        out.append(Op("canon%d" % c.L, c, "canon"))
        out.append(Op("to_words%d" % c.L, c, "words"))
    return out


def op_names():
    return [o.name for o in ops()]


def get_op(name):
    return next(o for o in ops() if o.name == name)
