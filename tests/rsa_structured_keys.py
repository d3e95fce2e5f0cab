"""RSA keys whose moduli are products of Mersenne primes, with valid
signatures, for tests/test_rsa_structured.py (host build) and
tests/test_gpu_rsa_structured.py.

The rsa crate's key check has no primality test, so any odd modulus is a legal
key.  A single M_p = 2^p - 1 is all ones (ninv = 1); a product of two is
2^(a+b) - 2^a - 2^b + 1 (ninv = 2^28 - 1, long runs of zero and one bits):
the limb patterns that products of random primes never give, here with a known
factorisation, so that valid signatures exist.  A prime modulus has
phi = n - 1.  Everything is generated from the seed below with
oracle/rsa_oracle.py; the expected code of every row is oracle.verify_code."""
import random

from oracle import rsa_oracle as o

import rsa_probe_model as pm

# Mersenne exponents of the factors, and the size class host_rsa.cpp
# size_class_limbs picks for the product
KEYS = [
    ((521,), 37),
    ((521, 127, 107, 89, 61, 31), 37),          # 936 bits
    ((607, 521), 74),                           # 1128 bits
    ((1279,), 74),
    ((1279, 607), 74),                          # 1886 bits
    ((1279, 521, 127, 107), 74),                # 2034 bits
    ((2203,), 80),
    ((2281,), 88),
    ((3217,), 120),
    ((2203, 1279), 128),                        # 3482 bits
    ((2281, 1279, 521), 152),                   # 4081 bits
    ((61, 31), 37),                             # 92 bits, k = 12: the message is at most 1 byte
]
# coprime to M_p - 1 for every p above (asserted in structured()); e = 2 takes
# square roots (every M_p is 3 mod 4); e = 3 divides every M_p - 1 here
EXPONENTS = [65537, (1 << 32) + 1, 0x1fffffffd, 2]
MSG_LENS = [0, 1, 32, None]     # None: k - 11, the longest


class Key:
    def __init__(self, exps, L):
        self.exps, self.L = exps, L
        self.factors = [(1 << p) - 1 for p in exps]
        self.n = 1
        for q in self.factors:
            self.n *= q
        self.k = (self.n.bit_length() + 7) // 8
        self.name = "M" + "x".join(str(p) for p in exps)

    def crt(self, residues):
        x, m = 0, 1
        for r, q in zip(residues, self.factors):
            x += m * ((r - x) * pow(m, -1, q) % q)
            m *= q
        return x

    def root(self, v, e):
        """s with s^e = v (mod n), or None (e = 2 and v is not a square)"""
        rs = []
        for q in self.factors:
            if e == 2:
                r = pow(v, (q + 1) // 4, q)
                if r * r % q != v % q:
                    return None
            else:
                r = pow(v, pow(e, -1, q - 1), q)
            rs.append(r)
        return self.crt(rs)

    def row28(self):
        """(n28, r2_28, ninv) of the device key row, computed here"""
        R = 1 << (28 * self.L)
        return pm.limbs(self.n, self.L), pm.limbs(R * R % self.n, self.L), pm.ninv_of(self.n)


def em_of(k, msg, block_type=1, separator=True):
    return bytes([0, block_type]) + b"\xff" * (k - len(msg) - 3) + (b"\x00" if separator else b"\xff") + msg


class Row:
    __slots__ = ("key", "e", "msg", "sig", "code", "what")

    def __init__(self, key, e, msg, sig, what):
        self.key, self.e, self.msg, self.sig, self.what = key, e, msg, sig, what
        self.code = o.verify_code(key.n, e, msg, sig)


def _signed(key, e, rng, length, **em_args):
    """(msg, sig) with sig^e = EM(msg); for e = 2 messages are drawn until EM
    is a square modulo every factor (None if the length leaves no choice)"""
    for _ in range(1 if length == 0 else 4096):
        msg = bytes(rng.randrange(256) for _ in range(length))
        s = key.root(int.from_bytes(em_of(key.k, msg, **em_args), "big"), e)
        if s is not None:
            return msg, s.to_bytes(key.k, "big")
    return None


def _rows(key, e, rng):
    k, n = key.k, key.n
    rows = []
    lens = sorted({k - 11 if ln is None else ln for ln in MSG_LENS})
    for ln in lens:
        if ln > k - 11:       # the tiny key: no signature exists, the length check answers
            rows.append(Row(key, e, bytes(ln), (1).to_bytes(k, "big"), "too long"))
            continue
        got = _signed(key, e, rng, ln)
        if got is None:
            continue
        msg, sig = got
        rows.append(Row(key, e, msg, sig, "valid %d" % ln))
        if ln:
            rows.append(Row(key, e, bytes([msg[0] ^ 0x01]) + msg[1:], sig, "first byte"))
            rows.append(Row(key, e, msg[:-1] + bytes([msg[-1] ^ 0x80]), sig, "last byte"))
    rows.append(Row(key, e, bytes(k - 10), (1).to_bytes(k, "big"), "one byte too long"))
    msg = bytes(rng.randrange(256) for _ in range(min(8, k - 11)))
    for s in (0, 1, n - 1, n, n + 1, (1 << (8 * k)) - 1, pm.all_ones_below(n)):
        rows.append(Row(key, e, msg, s.to_bytes(k, "big"), "s = %s" % hex(s)[:12]))
    for what, args in (("block type 02", {"block_type": 2}), ("no separator", {"separator": False})):
        got = _signed(key, e, rng, min(8, k - 11), **args)
        if got is not None:
            rows.append(Row(key, e, got[0], got[1], what))
    return rows


_cache = []


def structured():
    """(keys, rows), generated once per process"""
    if not _cache:
        rng = random.Random(0x4d657273)
        keys = [Key(exps, L) for exps, L in KEYS]
        rows = []
        for key in keys:
            assert pm.size_class_limbs(key.n.bit_length(), key.k) == key.L, key.name
            for e in EXPONENTS:
                if e != 2:
                    assert all(pow(e, -1, q - 1) for q in key.factors)
                rows += _rows(key, e, rng)
        _cache.append((keys, rows))
    return _cache[0]
