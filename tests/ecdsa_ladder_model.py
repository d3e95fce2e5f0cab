"""The ladder of cess_amd/csrc/p256.hpp (double_mul) on scalars, and inputs that
steer it into the special returns of pt_madd: a doubling, a cancel to infinity
and an infinite accumulator that is re-entered.  Built on tests/ecdsa_model.py
alone; exact integers, no tolerance.

With the key Q = d G the ladder's accumulator is sigma G for a scalar sigma mod
n that the digits of u1 and u2 fix: sigma = d2[0] d, then + d1[0]; in round k
sigma <- 16 sigma, then + d2[k+1] d (the Q addition), then + d1[k+1] (the G
addition).  An addition of a is special where sigma = a (doubling), sigma = -a
(cancel) or sigma = 0 (the accumulator is infinite).  Whoever picks the key picks
d, so for digit prefixes A of u1 and B of u2 before round k

    Q addition:  16 (A + B d) = +-d2[k+1] d     d = 16 A / (+-d2[k+1] - 16 B)
    G addition:  16 A + (16 B + d2[k+1]) d = +-d1[k+1]
                                                d = (+-d1[k+1] - 16 A) / (16 B + d2[k+1])

puts the accumulator on the addend (+) or on its negative (-) at that addition.
steer() does this for free scalars u1 and u2 (the ladder alone, verify_scalars,
emu_ecdsa_record with the digest given); grind() does it for full records, whose
e is a hash: d from a reachable prefix, a fixed nonce, and messages tried until
the digits of u1 = e / s and u2 = r / s begin with that prefix.
"""
import random

import ecdsa_model as m

N, G = m.N, m.G
BIAS = int("8" * 64, 16)
ROUNDS = 64
START = -1                       # the two additions before the loop (digit 0 of u2, then of u1)
KINDS = ("dbl", "cancel")
ADDENDS = ("Q", "G")
TARGETS = [(k, a, kind) for k in range(ROUNDS) for a in ADDENDS for kind in KINDS]


def inv(a):
    return pow(a, -1, N)


_pow2g = []


def mul_g(k):
    """k G as a sum of the 2^i G with ecdsa_model.add: a third of ecdsa_model.mul's work (no doublings); the
    host test holds it to ecdsa_model.mul on every row"""
    if not _pow2g:
        p = G
        for _ in range(256):
            _pow2g.append(p)
            p = m.add(p, p)
    r, i, k = None, 0, k % N
    while k:
        if k & 1:
            r = m.add(r, _pow2g[i])
        k >>= 1
        i += 1
    return r


def recode(s):
    """the 65 signed radix-16 digits of p256.hpp's sc_recode, most significant first: digit 0 is 0 or 1"""
    t = s + BIAS
    return [t >> 256] + [((t >> (4 * i)) & 15) - 8 for i in range(63, -1, -1)]


def unrecode(ds):
    return sum(d * 16 ** (64 - j) for j, d in enumerate(ds))


def prefix(ds, k):
    """the value of the digits 0..k: what the ladder has read of the scalar before round k"""
    v = 0
    for d in ds[:k + 1]:
        v = 16 * v + d
    return v


def trace(u1, u2, d):
    """the special additions of double_mul(u1, u2) under the key d G, in order: (round, addend, kind) with kind
    "inf" (infinite accumulator: the addend is taken over), "dbl" or "cancel"; round START before the loop.
    Also returns the final sigma (0: the sum is infinite)."""
    d1, d2 = recode(u1), recode(u2)
    events, sigma = [], 0
    for k in range(START, ROUNDS):
        sigma = 16 * sigma % N
        for addend, a in (("Q", d2[k + 1] * d % N), ("G", d1[k + 1] % N)):
            if a == 0:
                continue                                  # a zero digit adds nothing (d is not 0 and n is prime)
            if sigma == 0:
                events.append((k, addend, "inf"))
                sigma = a
            elif sigma == a:
                events.append((k, addend, "dbl"))
                sigma = 2 * a % N
            elif sigma == N - a:
                events.append((k, addend, "cancel"))
                sigma = 0
            else:
                sigma = (sigma + a) % N
    assert sigma == (u1 + u2 * d) % N
    return events, sigma


def counts(events):
    """(inf, dbl, cancel): what the host build's counters of pt_madd's special returns must read"""
    return tuple(sum(1 for e in events if e[2] == kind) for kind in ("inf", "dbl", "cancel"))


def steer_d(d1, d2, k, addend, kind):
    """the d that makes the `addend` addition of round k a `kind`, from the digits 0..k+1; None: draw again"""
    A, B = prefix(d1, k), prefix(d2, k)
    sign = 1 if kind == "dbl" else -1
    if addend == "Q":
        if d2[k + 1] == 0:
            return None
        num, den = 16 * A, sign * d2[k + 1] - 16 * B
    else:
        if d1[k + 1] == 0:
            return None
        num, den = sign * d1[k + 1] - 16 * A, 16 * B + d2[k + 1]
    if den % N == 0 or num % N == 0:
        return None
    return num * inv(den) % N


def steer(rng, k, addend, kind, shape=None):
    """(d, u1, u2) with 1 <= u1, u2 < n whose trace holds (k, addend, kind).  shape(u1, u2, k) -> (u1, u2) or None
    may rewrite the digits after k + 1 (the steering reads only the digits 0..k+1)."""
    while True:
        u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
        if shape is not None:
            shaped = shape(u1, u2, k)
            if shaped is None:
                continue
            u1, u2 = shaped
        d = steer_d(recode(u1), recode(u2), k, addend, kind)
        if d is None:
            continue
        if (k, addend, kind) in trace(u1, u2, d)[0]:
            return d, u1, u2


def zero_run(j, need_g=None):
    """a shape for steer(): both scalars' digits zero for the j rounds after round k, then a non-zero digit.
    need_g: 0 makes the G digit of round k zero (a Q cancel stays infinite), 1 makes it non-zero."""
    def shape(u1, u2, k):
        d1, d2 = recode(u1), recode(u2)
        if k + 1 + j + 1 > 64:
            return None
        for i in range(k + 2, k + 2 + j):
            d1[i] = d2[i] = 0
        if d1[k + 2 + j] == 0 and d2[k + 2 + j] == 0:
            d2[k + 2 + j] = 3
        if need_g == 0:
            d1[k + 1] = 0
        elif need_g == 1 and d1[k + 1] == 0:
            d1[k + 1] = -5
        u1, u2 = unrecode(d1), unrecode(d2)
        if not (1 <= u1 < N and 1 <= u2 < N):
            return None
        assert recode(u1) == d1 and recode(u2) == d2
        return u1, u2
    return shape


def last_digit(want_zero):
    """a shape for steer() at round 63: the G digit of the last round zero (the Q addition is the last) or not"""
    def shape(u1, u2, k):
        d1 = recode(u1)
        if (d1[64] == 0) != want_zero:
            d1[64] = 0 if want_zero else 6
        u1 = unrecode(d1)
        return (u1, u2) if 1 <= u1 < N and recode(u1) == d1 else None
    return shape


class Row:
    """one steered ladder input: the key d G, u1, u2, the events and counts of its trace, the sum, and a valid
    signature (e, r, s) on integers where the sum is finite (s free and the row never valid where it is not)"""

    def __init__(self, name, target, d, u1, u2, rng):
        self.name, self.target, self.d, self.u1, self.u2 = name, target, d, u1, u2
        self.events, sigma = trace(u1, u2, d)
        self.counts = counts(self.events)
        self.key = mul_g(d)
        self.want = mul_g(sigma)                         # (u1 + u2 d) G: not the ladder's way to it
        if self.want is None:
            self.s = rng.randrange(1, N)
            self.r = u2 * self.s % N
        else:
            self.r = self.want[0] % N
            assert self.r, name
            self.s = self.r * inv(u2) % N
        self.e = u1 * self.s % N
        assert self.e * inv(self.s) % N == u1 and self.r * inv(self.s) % N == u2
        self.valid = 1 if self.want is not None else 0
        self.s_bad = (self.s + 1) % N or 1

    def judge_points(self):
        """ecdsa_model.mul's word on the key and on the expected sum (two multiplications)"""
        assert self.key == m.mul(self.d, G) and self.want == m.mul(self.u1 + self.u2 * self.d, G), self.name

    def judge(self):
        """the model's word on the key, the sum, the signature and its neighbour (six multiplications: the host
        test calls it once per row)"""
        self.judge_points()
        assert m.verify_scalars(self.e, self.r, self.s, self.key) == (m.OK if self.valid else m.MISMATCH), self.name
        assert m.verify_scalars(self.e, self.r, self.s_bad, self.key) == m.MISMATCH, self.name


_rows = {}


def rows(seed=1):
    """every steered row, once per process: the 256 targets in TARGETS' order, then the long-infinity rows, then
    the end rows.  Returns (targets, long_inf, ends): lists of Row."""
    if seed in _rows:
        return _rows[seed]
    rng = random.Random(seed)
    targets = [Row("round %d %s %s" % t, t, *steer(rng, *t), rng) for t in TARGETS]
    long_inf = []
    for k in (0, 1, 30, 59):
        for j in (1, 3):
            # a cancel at the G addition of round k, or at its Q addition under a zero G digit; j rounds of zero
            # digits; a non-zero digit in round k + j + 1: 4 (j + 1) doublings of an infinite accumulator
            for addend, need_g in (("G", None), ("Q", 0)):
                t = (k, addend, "cancel")
                row = Row("round %d %s cancel, %d zero rounds" % (k, addend, j), t, *steer(rng, *t, zero_run(j, need_g)), rng)
                at = row.events.index(t)
                assert row.events[at + 1][2] == "inf" and row.events[at + 1][0] == k + j + 1, row.name
                row.inf_doublings = 4 * (j + 1)
                long_inf.append(row)
    ends = []
    for name, t, shape in (("the last addition (G) doubles", (63, "G", "dbl"), None),
                           ("the last addition (G) cancels: infinite", (63, "G", "cancel"), None),
                           ("the last addition (Q, zero G digit) doubles", (63, "Q", "dbl"), last_digit(True)),
                           ("the last addition (Q, zero G digit) cancels: infinite", (63, "Q", "cancel"), last_digit(True)),
                           ("round 63: Q cancels, G re-enters", (63, "Q", "cancel"), last_digit(False)),
                           ("round 0: Q cancels, G re-enters", (0, "Q", "cancel"), zero_run(0, 1)),
                           ("round 31: Q cancels, G re-enters", (31, "Q", "cancel"), zero_run(0, 1))):
        ends.append(Row(name, t, *steer(rng, *t, shape), rng))
    assert ends[0].events[-1] == (63, "G", "dbl") and ends[0].want is not None
    assert ends[1].events[-1] == (63, "G", "cancel") and ends[1].want is None
    assert ends[2].events[-1] == (63, "Q", "dbl") and ends[2].want is not None
    assert ends[3].events[-1] == (63, "Q", "cancel") and ends[3].want is None
    for row in ends[4:]:
        at = row.events.index(row.target)
        assert row.events[at + 1] == (row.target[0], "G", "inf"), row.name
    _rows[seed] = (targets, long_inf, ends)
    return _rows[seed]


def all_rows(seed=1):
    t, li, e = rows(seed)
    return t + li + e


# --- full records ---------------------------------------------------------------
def grind(alg, k, addend, kind, rng, tag=b"ecdsa ladder"):
    """a valid record (d, msg, r, s) whose ladder takes (k, addend, kind): d from the digit prefix of two random
    scalars below n, a fixed nonce, and a counter in the message until u1 = e / s and u2 = r / s begin with those
    digits.  A draw is given up after 20 times the expected tries.  Also returns the tries."""
    n1 = k + 1 if addend == "G" else k            # digits of u1 after the top one that the steering reads
    n2 = k + 1                                    # and of u2; the top digits are 0 or 1: 4 * 16^(n1 + n2) tries
    cap = 20 * 4 * 16 ** (n1 + n2)
    total = 0
    while True:
        a1, a2 = rng.randrange(1, N), rng.randrange(1, N)
        d = steer_d(recode(a1), recode(a2), k, addend, kind)
        if d is None:
            continue
        want1, want2 = (a1 + BIAS) >> (256 - 4 * n1), (a2 + BIAS) >> (256 - 4 * n2)
        nonce = rng.randrange(1, N)
        r = m.mul(nonce, G)[0] % N
        if r == 0:
            continue
        ninv, rd = inv(nonce), r * d % N
        sh1, sh2 = 256 - 4 * n1, 256 - 4 * n2
        head = tag + b" %d round %d %s %s " % (alg, k, addend.encode(), kind.encode())
        for c in range(cap):
            msg = head + b"%d" % c
            e = m.digest_scalar(alg, msg)
            s = ninv * (e + rd) % N
            if s == 0:
                continue
            w = inv(s)
            if (r * w % N + BIAS) >> sh2 != want2 or (e * w % N + BIAS) >> sh1 != want1:
                continue
            u1, u2 = e * w % N, r * w % N
            if (k, addend, kind) in trace(u1, u2, d)[0]:
                assert (r, s) == m.sign(alg, d, nonce, msg)
                return d, msg, r, s, total + c + 1
        total += cap
