"""Operand tables and integer checks for the ECDSA P-256 primitives
(cess_amd/csrc/p256.hpp through tests/probe/ecdsa_probe.hip), shared by the host
build's tests (tests/test_ecdsa_primitives.py, tests/test_ecdsa.py) and the GPU
probe's (tests/test_gpu_ecdsa_primitives.py).

Digits: ten 28-bit digits, digit k of weight 2^(28 k), Montgomery form with
R = 2^280.  "tight": digits 0..8 below 2^28, digit 9 below 32, value below twice
the modulus.  "lazy": digits below 3 * 2^28.
"""
import json
import os
import random

import ecdsa_model as m

Q, N = m.Q, m.N
R = 1 << 280
M28 = (1 << 28) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# entry: (words in, words out, leading table indices)
OPS = {"fe_mul": (20, 10, 0), "fe_sqr": (10, 10, 0), "fe_add": (20, 10, 0), "fe_sub": (20, 10, 0), "fe_neg": (10, 10, 0),
       "fe_mulk": (11, 10, 0), "fe_canon": (10, 11, 0), "fe_invert": (10, 10, 0), "sc_mul": (20, 10, 0),
       "sc_sqr": (10, 10, 0), "sc_invert": (10, 10, 0), "sc_canon": (10, 10, 0), "sc_digits": (8, 65, 0),
       "digest_scalar": (8, 8, 0), "pt_dbl": (30, 30, 0), "pt_madd": (50, 30, 0), "key_table": (18, 241, 0),
       "parse_sig": (82, 17, 0), "double_mul": (18, 30, 2), "verify_scalars": (26, 1, 2)}


def digits(v):
    """canonical digits of v < 2^280 (digit 9 takes what is left)"""
    return [(v >> (28 * i)) & M28 for i in range(9)] + [v >> 252]


def value(d):
    return sum(x << (28 * i) for i, x in enumerate(d))


def words(v, n=8):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def from_words(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def is_tight(d, mod):
    return all(x <= M28 for x in d[:9]) and d[9] < 32 and value(d) < 2 * mod


def lazy_max():
    """three tight maxima: every digit at its bound (value far above 6 q: only for mul / sqr / sub inputs)"""
    return [3 * M28] * 9 + [3 * 31]


def field_values(mod, rng):
    vals = [0, 1, 2, mod - 1, mod, mod + 1, 2 * mod - 1, (1 << 256) - 1 if (1 << 256) - 1 < 2 * mod else mod - 2,
            R % mod, (1 << 255), mod - (1 << 96), (1 << 224) - 1]
    vals += [rng.randrange(2 * mod) for _ in range(12)]
    return [v for v in vals if v < 2 * mod]


def bytes_words(b, n):
    b = bytes(b) + bytes(4 * n - len(b))
    return [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(n)]


def mont_pt(p):
    return digits(p[0] * R % Q), digits(p[1] * R % Q)


def jac_rows():
    """(X, Y, Z) plain integers of ring's point rows and a few scaled copies"""
    ring = json.load(open(os.path.join(GOLDEN, "ring_ecdsa.json")))
    h = lambda p: None if p is None else [int(c, 16) for c in p]  # noqa: E731
    return ring, h


def affine(X, Y, Z):
    if Z % Q == 0:
        return None
    zi = pow(Z, -1, Q)
    return (X * zi * zi % Q, Y * zi ** 3 % Q)


RECODE_PATTERNS = [0, 1, 2, 7, 8, 9, 15, 16, 17, N - 1, N - 2, 1 << 128, 1 << 255, int("7" * 64, 16),
                   (1 << 256) - int("8" * 64, 16), 16 ** 63, 7 * 16 ** 31, (1 << 256) - 1, int("8" * 64, 16),
                   int("7" * 63 + "8", 16)]


def tables(seed=20260):
    rng = random.Random(seed)
    t = {}
    fq, fn = field_values(Q, rng), field_values(N, rng)
    pairs = lambda vs: [(a, b) for a in vs[:12] for b in vs[:12:3]] + list(zip(vs[12:], reversed(vs[12:])))  # noqa: E731
    lz = lazy_max()
    t["fe_mul"] = [digits(a) + digits(b) for a, b in pairs(fq)] + [lz + lz, lz + digits(Q - 1), digits(2 * Q - 1) + lz]
    t["fe_sqr"] = [digits(a) for a in fq] + [lz]
    t["fe_add"] = [digits(a) + digits(b) for a, b in pairs(fq)]
    t["fe_sub"] = [digits(a) + digits(b) for a, b in pairs(fq)] + [digits(0) + digits(32 * Q - 1), lz + digits(32 * Q - 1),
                                                                   digits(0) + digits(6 * Q)]
    t["fe_neg"] = [digits(a) for a in fq]
    t["fe_mulk"] = [digits(a) + [k] for a in fq for k in (1, 3, 4, 8)]
    t["fe_canon"] = [digits(a) for a in fq]
    t["fe_invert"] = [digits(a) for a in fq[:6] + fq[-3:]]
    t["sc_mul"] = [digits(a) + digits(b) for a, b in pairs(fn)] + [lz + lz]
    t["sc_sqr"] = [digits(a) for a in fn] + [lz]
    t["sc_invert"] = [digits(a) for a in fn[:6] + fn[-3:]]
    t["sc_canon"] = [digits(a) for a in fn]
    t["sc_digits"] = [words(v) for v in RECODE_PATTERNS + [rng.randrange(1 << 256) for _ in range(8)]]
    t["digest_scalar"] = [bytes_words(v.to_bytes(32, "big"), 8) for v in
                          (0, 1, N - 1, N, N + 1, (1 << 256) - 1, 2 * N - (1 << 256) + 5, rng.randrange(1 << 256))]
    ring, h = jac_rows()
    mont = lambda c: digits(c * R % Q)  # noqa: E731
    inf = [mont(1), mont(1), digits(0)]
    dbl, madd = [], []
    for r in ring["point_double"]:
        a = h(r["a"])
        dbl.append(mont(a[0]) + mont(a[1]) + mont(a[2]))
    for r in ring["point_sum_mixed"]:
        a, b = h(r["a"]), h(r["b"])
        if b is not None:
            madd.append(mont(a[0]) + mont(a[1]) + mont(a[2]) + mont(b[0]) + mont(b[1]))
    for r in ring["point_sum"]:          # the Jacobian rows whose second operand has an affine form
        a, b = h(r["a"]), h(r["b"])
        pb = affine(*b)
        if pb is not None:
            madd.append(mont(a[0]) + mont(a[1]) + mont(a[2]) + mont(pb[0]) + mont(pb[1]))
    for k in (1, 2, 3, N - 1, N - 2):    # P + P, P + (-P), neighbours, with a scaled Z
        p = m.mul(k, m.G)
        z = rng.randrange(1, Q)
        X, Y = p[0] * z * z % Q, p[1] * z ** 3 % Q
        for other in (m.G, m.neg(m.G), m.mul(2, m.G)):
            madd.append(mont(X) + mont(Y) + mont(z) + mont(other[0]) + mont(other[1]))
        dbl.append(mont(X) + mont(Y) + mont(z))
        # the zero of Z and of H in its other tight form: q itself
        madd.append(mont(X) + mont(Y) + digits(Q) + mont(m.G[0]) + mont(m.G[1]))
    # the bound's corners: every coordinate in its other tight encoding, value + q (just below 2 q), and the
    # largest tight value 2 q - 1 itself (digits at their maxima) as a coordinate of a finite and of an infinite point
    up = lambda c: digits(c * R % Q + Q)  # noqa: E731
    top = digits(2 * Q - 1)
    for k in (1, 2, 5, N - 1):
        p = m.mul(k, m.G)
        z = rng.randrange(1, Q)
        X, Y = p[0] * z * z % Q, p[1] * z ** 3 % Q
        dbl.append(up(X) + up(Y) + up(z))
        for other in (m.G, m.neg(m.G), m.mul(3, m.G)):
            madd.append(up(X) + up(Y) + up(z) + up(other[0]) + up(other[1]))
            madd.append(mont(X) + up(Y) + mont(z) + up(other[0]) + mont(other[1]))
    dbl.append(top + top + digits(Q))
    dbl.append(top + top + digits(0))
    madd.append(top + top + digits(Q) + up(m.G[0]) + up(m.G[1]))
    dbl.append(sum(inf, []))
    t["pt_dbl"], t["pt_madd"] = dbl, madd
    edges = json.load(open(os.path.join(GOLDEN, "ecdsa_edges.json")))["rows"]
    keys = list(dict.fromkeys(r["key"] for r in edges if r["key"] is not None))
    keys = [bytes.fromhex(k) for k in keys if len(k) // 2 <= 68]
    keys += [bytes.fromhex(r["key"]) for r in ring["keys"]]
    t["key_table"] = [[len(k)] + bytes_words(k, 17) for k in keys]
    sigs = list(dict.fromkeys((r["alg"], r["sig"]) for r in edges))          # every row: the longest has 299 bytes
    sigs += [(r["alg"], r["sig"]) for r in ring["verify"]]
    assert max(len(s) for _, s in sigs) // 2 <= 320
    t["parse_sig"] = [[alg, len(s) // 2] + bytes_words(bytes.fromhex(s), 80) for alg, s in sigs]
    return t


def check(op, rows, outs):
    """the rows' results against integers; raises AssertionError naming the row"""
    assert len(rows) == len(outs), op
    for i, (row, out) in enumerate(zip(rows, outs)):
        tag = "%s row %d" % (op, i)
        if op in ("fe_mul", "sc_mul", "fe_sqr", "sc_sqr"):
            mod = Q if op[0] == "f" else N
            a = value(row[:10])
            b = value(row[10:20]) if op.endswith("mul") else a
            assert is_tight(out, mod) and value(out) % mod == a * b * pow(R, -1, mod) % mod, tag
        elif op == "fe_add":
            assert out == [x + y for x, y in zip(row[:10], row[10:])], tag
        elif op == "fe_sub":
            assert is_tight(out, Q) and value(out) < (1 << 256) + (1 << 230), tag
            assert value(out) % Q == (value(row[:10]) - value(row[10:])) % Q, tag
        elif op == "fe_neg":
            assert is_tight(out, Q) and (value(out) + value(row)) % Q == 0, tag
        elif op == "fe_mulk":
            assert is_tight(out, Q) and value(out) % Q == value(row[:10]) * row[10] % Q, tag
        elif op == "fe_canon":
            assert value(out[:10]) == value(row) % Q and out[:10] == digits(value(row) % Q), tag
            assert out[10] == (1 if value(row) % Q == 0 else 0), tag
        elif op == "sc_canon":
            assert out == digits(value(row) % N), tag
        elif op in ("fe_invert", "sc_invert"):
            mod = Q if op[0] == "f" else N
            a = value(row) * pow(R, -1, mod) % mod                 # the plain value
            want = pow(a, mod - 2, mod) * R % mod
            assert is_tight(out, mod) and value(out) % mod == want, tag
        elif op == "sc_digits":
            s = from_words(row)
            ds = [out[0]] + [d - 8 for d in out[1:]]
            assert out[0] in (0, 1) and all(-8 <= d <= 7 for d in ds[1:]), tag
            assert sum(d * 16 ** (64 - j) for j, d in enumerate(ds)) == s, tag
        elif op == "digest_scalar":
            b = b"".join(w.to_bytes(4, "little") for w in row)
            assert from_words(out) == m.digest_to_scalar(b), tag
        elif op in ("pt_dbl", "pt_madd"):
            un = lambda d: value(d) * pow(R, -1, Q) % Q  # noqa: E731
            p = affine(un(row[:10]), un(row[10:20]), un(row[20:30]))
            want = m.add(p, p) if op == "pt_dbl" else m.add(p, (un(row[30:40]), un(row[40:50])))
            assert all(is_tight(out[10 * j:10 * j + 10], Q) for j in range(3)), tag
            assert affine(un(out[:10]), un(out[10:20]), un(out[20:30])) == want, tag
        elif op == "key_table":
            key = b"".join(w.to_bytes(4, "little") for w in row[1:])[:row[0]]
            p = m.key_point(key)
            assert out[0] == (0 if p is not None else 1), tag
            if p is not None:
                un = lambda d: value(d) * pow(R, -1, Q) % Q  # noqa: E731
                for j in range(8):
                    e = out[1 + 30 * j:1 + 30 * j + 30]
                    assert is_tight(e[:10], Q) and is_tight(e[10:20], Q), tag
                    assert (un(e[:10]), un(e[10:20])) == m.mul(j + 1, p), tag
        elif op == "parse_sig":
            sig = b"".join(w.to_bytes(4, "little") for w in row[2:])[:row[1]]
            rs = m.split_sig(row[0], sig)
            if rs is None:
                assert out[16] == m.SIG_FORMAT, tag
            else:
                r, s = int.from_bytes(rs[0], "big"), int.from_bytes(rs[1], "big")
                if 1 <= r < N and 1 <= s < N:
                    assert out[16] == 0 and from_words(out[:8]) == r and from_words(out[8:16]) == s, tag
                else:
                    assert out[16] == m.SIG_RANGE, tag
        else:
            raise AssertionError("no check for " + op)


def verify_rows(seed=7):
    """(key table bytes, rows [e, r, s], expected) for the verify loop: e = 0 and e = n - 1 included"""
    rng = random.Random(seed)
    d = rng.randrange(1, N)
    qp = m.mul(d, m.G)
    rows, want = [], []
    for e in (0, N - 1, 1, rng.randrange(N), rng.randrange(N)):
        k = rng.randrange(1, N)
        r = m.mul(k, m.G)[0] % N
        s = pow(k, -1, N) * (e + r * d) % N
        for rr, ss in ((r, s), (r, (s + 1) % N or 1)):
            rows.append((e, rr, ss))
            want.append(1 if m.verify_scalars(e, rr, ss, qp) == m.OK else 0)
    assert want[:4] == [1, 0, 1, 0]
    return m.key_bytes(qp), rows, want


def mul_rows(seed=11):
    """(keys, rows [index of the key, u1, u2], expected affine sums or None) for the ladder alone: ring's
    point_mul rows as u2 P (u1 = 0), and u1 G + u2 P at the recoding's corner scalars.  The caller appends G's
    table after the keys' (index len(keys))."""
    rng = random.Random(seed)
    ring, h = jac_rows()
    keys, rows, want = [], [], []
    for r in ring["point_mul"]:
        p = tuple(h(r["p"]))
        kb = m.key_bytes(p)
        if kb not in keys:
            keys.append(kb)
        k = int(r["k"], 16)
        rows.append((keys.index(kb), 0, k))
        want.append(None if r["r"] is None else tuple(h(r["r"])))
        assert want[-1] == m.mul(k, p)
    p = m.key_point(keys[0])
    for u in RECODE_PATTERNS:
        v = rng.choice(RECODE_PATTERNS)
        rows.append((0, u, v))
        want.append(m.add(m.mul(u % N, m.G), m.mul(v % N, p)))
    return keys, rows, want


def check_mul(rows, outs, want):
    un = lambda d: value(d) * pow(R, -1, Q) % Q  # noqa: E731
    for i, (out, w) in enumerate(zip(outs, want)):
        assert all(is_tight(out[10 * j:10 * j + 10], Q) for j in range(3)), i
        assert affine(un(out[:10]), un(out[10:20]), un(out[20:30])) == w, ("double_mul row", i, rows[i][0])
