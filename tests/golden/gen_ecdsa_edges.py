#!/usr/bin/env python3
"""tests/golden/ecdsa_edges.json: crafted ECDSA P-256 records, each with the
code that tests/ecdsa_model.py gives it.  Pure Python and deterministic.

These rows are judged by the model alone: ring's P-256 arithmetic is assembly
and can not be built beside this project, so unlike the Ed25519 crafted rows no
compiled ring code has seen them.  The model itself agrees with every P-256 row
of ring's vector files (gen_ring_ecdsa.py).

A row: name, alg, key (hex; null: a key index outside the table), msg, sig, code.

The "equal halves" rows (u1 G = u2 Q) are named after a doubling that p256.hpp's
interleaved ladder does not take: they exercise its final r Z^2 = X test on
2 u1 G (see the comment at the rows).  Doublings and cancels inside the ladder
are gen_ecdsa_ladder.py's.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ecdsa_model as m  # noqa: E402

N, Q, G = m.N, m.Q, m.G
rng = random.Random(0xECD5A)
rows = []


def inv(a):
    return pow(a, -1, N)


def sqrt_q(v):
    y = pow(v, (Q + 1) // 4, Q)
    return y if y * y % Q == v % Q else None


def recode(s):
    """the 65 signed radix-16 digits of p256.hpp's sc_recode, most significant first"""
    t = s + int("8" * 64, 16)
    return [t >> 256] + [((t >> (4 * i)) & 15) - 8 for i in range(63, -1, -1)]


def put(name, alg, key, msg, sig, want=None):
    code = m.verify_code(alg, key, msg, sig)
    assert want is None or code == want, (name, code, want)
    rows.append({"name": name, "alg": alg, "key": None if key is None else key.hex(), "msg": msg.hex(),
                 "sig": sig.hex(), "code": code})


def put_rs(name, alg, qp, msg, r, s, want=None):
    put(name, alg, m.key_bytes(qp), msg, m.encode_sig(alg, r, s), want)


def fresh(alg, tag):
    msg = ("ecdsa edge %s %d" % (tag, alg)).encode()
    return msg, m.digest_scalar(alg, msg)


def honest(alg, tag, msg=None, cond=None):
    """a valid record under a random key: (key point, msg, r, s), with cond(r, s, e, d) if given"""
    if msg is None:
        msg = ("ecdsa edge %s %d" % (tag, alg)).encode()
    while True:
        d, k = rng.randrange(1, N), rng.randrange(1, N)
        rs = m.sign(alg, d, k, msg)
        if rs and (cond is None or cond(rs[0], rs[1], m.digest_scalar(alg, msg), d)):
            return m.mul(d, G), msg, rs[0], rs[1]


# --- the final sum: P + P, P + (-P) -------------------------------------------
# "Equal halves": u1 G = u2 Q.  A verifier that computes the two multiples apart would double here.  The
# interleaved ladder of p256.hpp does not: its accumulator is (A_k + B_k e / r) G and never meets an addend, so
# the first row exercises the final r Z^2 = X test on 2 u1 G, not a doubling branch (the name is kept: the rows
# are committed).  The opposite-halves row does cancel, at the ladder's very last addition.  Doublings and
# cancels inside the ladder: gen_ecdsa_ladder.py.
for alg in range(3):
    msg, e = fresh(alg, "equal halves")
    t = rng.randrange(1, N)
    r = m.mul(t, G)[0] % N
    s = 2 * e * inv(t) % N
    put_rs("u1 G = u2 Q: the sum is a doubling", alg, m.mul(e * inv(r) % N, G), msg, r, s, m.OK)
    put_rs("u1 G = -u2 Q: the sum is infinite", alg, m.mul(-e * inv(r) % N, G), msg, r, s, m.MISMATCH)

# the ladder's first addition doubles (key G, equal leading digits of u1 and u2) or
# cancels to infinity and goes on from there (key -G, equal leading digits)
for alg in range(3):
    for name, d in (("G", 1), ("-G", N - 1)):
        msg = ("ecdsa edge ladder %s %d" % (name, alg)).encode()
        e = m.digest_scalar(alg, msg)
        while True:
            k = rng.randrange(1, N)
            r, s = m.sign(alg, d, k, msg)
            d1, d2 = recode(e * inv(s) % N), recode(r * inv(s) % N)
            i1 = next(i for i, x in enumerate(d1) if x)
            i2 = next(i for i, x in enumerate(d2) if x)
            if i1 == i2 and d1[i1] == d2[i2]:
                break
        put_rs("key %s, equal leading digits of u1 and u2" % name, alg, m.mul(d, G), msg, r, s, m.OK)
        put_rs("key %s, equal leading digits, wrong message" % name, alg, m.mul(d, G), msg + b"!", r, s, m.MISMATCH)

# --- acceptance through r + n -------------------------------------------------
x = N
while sqrt_q(x * x * x - 3 * x + m.B) is None:
    x += 1
assert x == N + 3
T = (x, sqrt_q(x * x * x - 3 * x + m.B))
for alg in range(3):
    msg, e = fresh(alg, "r + n")
    r, s = x - N, 5
    u1, u2 = e * inv(s) % N, r * inv(s) % N
    qp = m.mul(inv(u2), m.add(T, m.neg(m.mul(u1, G))))
    put_rs("x(R) = r + n: valid through the second test only", alg, qp, msg, r, s, m.OK)
    put_rs("x(R) = r + n - 1: the neighbour", alg, qp, msg, r + 1, s, m.MISMATCH)
    qp, msg, r, s = honest(alg, "r >= q - n", cond=lambda r, s, e, d: r >= Q - N)
    put_rs("r >= q - n: the second test is skipped, still valid", alg, qp, msg, r, s, m.OK)

# --- prescribed u2 and u1 -----------------------------------------------------
ALL_MAX = int("7" * 64, 16)                     # every digit 7
ALL_MIN = (1 << 256) - int("8" * 64, 16)        # the top digit 1, every other -8
assert recode(ALL_MAX) == [0] + [7] * 64 and recode(ALL_MIN) == [1] + [-8] * 64 and ALL_MIN < N
CS = [1, 2, 8, 9, 15, 16, 17, N - 1, N - 2, 1 << 128, 1 << 255, ALL_MAX, ALL_MIN, 16 ** 63, 7 * 16 ** 31,
      (-8) % N]
for i, c in enumerate(CS):
    alg = i % 3
    msg, e = fresh(alg, "u2 = c %d" % i)
    t = rng.randrange(1, N)
    r = m.mul(t, G)[0] % N
    s = r * inv(c) % N
    d = (t - e * inv(s)) * inv(c) % N
    assert d and r * inv(s) % N == c
    put_rs("u2 = %x" % c, alg, m.mul(d, G), msg, r, s, m.OK)
    alg = (i + 1) % 3
    msg, e = fresh(alg, "u1 = c %d" % i)
    s = e * inv(c) % N
    u2 = r * inv(s) % N
    d = (t - c) * inv(u2) % N
    assert d and e * inv(s) % N == c
    put_rs("u1 = %x" % c, alg, m.mul(d, G), msg, r, s, m.OK)

# --- range ----------------------------------------------------------------------
for alg in range(3):
    qp, msg, r, s = honest(alg, "range")
    for v in (0, N, N + 1, (1 << 256) - 1):
        for which in "rs":
            rr, ss = (v, s) if which == "r" else (r, v)
            if alg == m.ALG_P256_SHA256_FIXED:
                sig = rr.to_bytes(32, "big") + ss.to_bytes(32, "big")
                want = m.SIG_RANGE
            else:
                sig = m.encode_sig(alg, rr, ss)
                want = m.SIG_FORMAT if v == 0 else m.SIG_RANGE      # ring's der.rs rejects the value zero
            put("%s = %x" % (which, v), alg, m.key_bytes(qp), msg, sig, want)
    if alg:
        # more than 32 significant bytes
        body = m.der_int(1 << 256) + m.der_int(s)
        put("r = 2^256 (33 significant bytes)", alg, m.key_bytes(qp), msg, b"\x30" + m.der_len(len(body)) + body,
            m.SIG_RANGE)
        body = m.der_int(r) + m.der_int(1 << 300)
        put("s = 2^300", alg, m.key_bytes(qp), msg, b"\x30" + m.der_len(len(body)) + body, m.SIG_RANGE)

# --- FIXED lengths ----------------------------------------------------------------
qp, msg, r, s = honest(0, "fixed lengths")
good = m.encode_sig(0, r, s)
put("FIXED, valid", 0, m.key_bytes(qp), msg, good, m.OK)
for sig in (b"", good[:63], good + b"\x00"):
    put("FIXED, %d bytes" % len(sig), 0, m.key_bytes(qp), msg, sig, m.SIG_FORMAT)
put("FIXED given an ASN.1 signature", 0, m.key_bytes(qp), msg, m.encode_sig(1, r, s))
put("ASN1 given a FIXED signature", 1, m.key_bytes(qp), msg, good)

# --- ASN.1 ------------------------------------------------------------------------
for alg in (1, 2):
    # both integers with the top bit set, so that both carry a leading zero
    qp, msg, r, s = honest(alg, "asn1", cond=lambda r, s, e, d: r >> 255 and s >> 255)
    key = m.key_bytes(qp)
    ri, si = m.der_int(r), m.der_int(s)
    body = ri + si
    seq = lambda b, tag=0x30: bytes([tag]) + m.der_len(len(b)) + b  # noqa: E731
    put("ASN.1, valid, both integers of 33 content bytes", alg, key, msg, seq(body), m.OK)
    F = m.SIG_FORMAT
    put("ASN.1: empty", alg, key, msg, b"", F)
    put("ASN.1: one byte", alg, key, msg, b"\x30", F)
    put("ASN.1: sequence tag with all low bits set", alg, key, msg, seq(body, 0x3f), F)
    put("ASN.1: sequence tag 0x1f", alg, key, msg, seq(body, 0x1f), F)
    put("ASN.1: not a sequence", alg, key, msg, seq(body, 0x31), F)
    put("ASN.1: integer tag with all low bits set", alg, key, msg, seq(b"\x1f" + ri[1:] + si), F)
    put("ASN.1: r is not an INTEGER", alg, key, msg, seq(b"\x03" + ri[1:] + si), F)
    put("ASN.1: s is not an INTEGER", alg, key, msg, seq(ri + b"\x04" + si[1:]), F)
    put("ASN.1: 0x81 length below 128 (not canonical)", alg, key, msg, b"\x30\x81" + bytes([len(body)]) + body, F)
    put("ASN.1: 0x82 length below 256", alg, key, msg, b"\x30\x82\x00" + bytes([len(body)]) + body, F)
    put("ASN.1: indefinite length", alg, key, msg, b"\x30\x80" + body, F)
    put("ASN.1: 0x83 length", alg, key, msg, b"\x30\x83\x00\x00" + bytes([len(body)]) + body, F)
    put("ASN.1: 0x81 length on r", alg, key, msg, seq(b"\x02\x81" + ri[1:] + si), F)
    put("ASN.1: length past the end", alg, key, msg, bytes([0x30, len(body) + 1]) + body, F)
    put("ASN.1: r's length past the sequence", alg, key, msg, seq(b"\x02\x7f" + ri[2:] + si), F)
    put("ASN.1: truncated", alg, key, msg, seq(body)[:-1], F)
    put("ASN.1: 0x81 without its byte", alg, key, msg, b"\x30\x81", F)
    put("ASN.1: 0x82 with one byte", alg, key, msg, b"\x30\x82\x01", F)
    put("ASN.1: empty INTEGER r", alg, key, msg, seq(b"\x02\x00" + si), F)
    put("ASN.1: empty INTEGER s", alg, key, msg, seq(ri + b"\x02\x00"), F)
    put("ASN.1: negative r", alg, key, msg, seq(b"\x02\x20" + ri[3:] + si), F)
    put("ASN.1: negative s", alg, key, msg, seq(ri + b"\x02\x20" + si[3:]), F)
    put("ASN.1: r with a leading zero it does not need", alg, key, msg, seq(b"\x02\x02\x00\x05" + si), F)
    put("ASN.1: s with two leading zeros", alg, key, msg, seq(ri + b"\x02\x22\x00" + si[2:]), F)
    put("ASN.1: r = 0", alg, key, msg, seq(b"\x02\x01\x00" + si), F)
    put("ASN.1: s = 0", alg, key, msg, seq(ri + b"\x02\x01\x00"), F)
    put("ASN.1: s missing", alg, key, msg, seq(ri), F)
    put("ASN.1: empty sequence", alg, key, msg, seq(b""), F)
    put("ASN.1: a byte after s inside the sequence", alg, key, msg, seq(body + b"\x00"), F)
    put("ASN.1: a third INTEGER", alg, key, msg, seq(body + b"\x02\x01\x01"), F)
    put("ASN.1: a byte after the sequence", alg, key, msg, seq(body) + b"\x00", F)
    # a long but canonical encoding: 0x81 with a byte >= 128 needs 128 bytes of content; they are two wide integers
    wide = m.der_int(1 << 500) + m.der_int(1 << 500)
    assert len(wide) == 130
    put("ASN.1: canonical 0x81 length, both integers wide", alg, key, msg, b"\x30\x81\x82" + wide, m.SIG_RANGE)
    big = b"\x02\x82\x01\x00" + b"\x01" + bytes(255)
    put("ASN.1: canonical 0x82 lengths", alg, key, msg, b"\x30\x82" + (len(big) + len(si)).to_bytes(2, "big") + big + si,
        m.SIG_RANGE)
    # content sizes: 1 (through r + n), 31, 32, 33
    msg1, e = fresh(alg, "one content byte")
    r1, s1 = 3, 5
    u1, u2 = e * inv(s1) % N, r1 * inv(s1) % N
    q1 = m.mul(inv(u2), m.add(T, m.neg(m.mul(u1, G))))
    assert len(m.der_int(r1)) == 3
    put_rs("ASN.1: r and s of 1 content byte", alg, q1, msg1, r1, s1, m.OK)
    for nbytes, cond in ((31, lambda v: v.bit_length() <= 247 and v.bit_length() > 240),
                         (32, lambda v: v.bit_length() <= 255 and v.bit_length() > 248),
                         (33, lambda v: v.bit_length() == 256)):
        qr, mr, rr, sr = honest(alg, "r of %d" % nbytes, cond=lambda r, s, e, d: cond(r))
        assert len(m.der_int(rr)) == 2 + nbytes
        put_rs("ASN.1: r of %d content bytes" % nbytes, alg, qr, mr, rr, sr, m.OK)
        qr, mr, rr, sr = honest(alg, "s of %d" % nbytes, cond=lambda r, s, e, d: cond(s))
        assert len(m.der_int(sr)) == 2 + nbytes
        put_rs("ASN.1: s of %d content bytes" % nbytes, alg, qr, mr, rr, sr, m.OK)

# --- keys ---------------------------------------------------------------------------
qp, msg, r, s = honest(1, "keys")
sig = m.encode_sig(1, r, s)
good = m.key_bytes(qp)
put("key, valid", 1, good, msg, sig, m.OK)
be = lambda v: v.to_bytes(32, "big")  # noqa: E731
bad_keys = [("x = q", b"\x04" + be(Q) + good[33:]), ("y = q", good[:33] + be(Q)),
            ("x = q - 1", b"\x04" + be(Q - 1) + good[33:]), ("y = q - 1", good[:33] + be(Q - 1)),
("y = 0", good[:33] + be(0)), ("x = 0, y = 0", b"\x04" + bytes(64)),
            ("y negated and first byte 0x02", b"\x02" + good[1:]), ("first byte 0x03", b"\x03" + good[1:]),
            ("first byte 0x00", b"\x00" + good[1:]), ("first byte 0x06", b"\x06" + good[1:]),
            ("compressed, 33 bytes", b"\x02" + good[1:33]), ("64 bytes", good[:64]), ("64 bytes without the first", good[1:]),
            ("66 bytes", good + b"\x00"), ("empty", b""), ("y + 1", good[:33] + be((qp[1] + 1) % Q))]
xt = 5
while sqrt_q(xt ** 3 - 3 * xt + m.B) is not None:
    xt += 1
yt = sqrt_q(-(xt ** 3 - 3 * xt + m.B))
assert yt is not None
bad_keys.append(("a point of the twist", b"\x04" + be(xt) + be(yt)))
# x + q fits 32 bytes only for x < 2^256 - q: a point with so small an x, encoded as x + q, and likewise y + q
xs = 1
while sqrt_q(xs ** 3 - 3 * xs + m.B) is None:
    xs += 1
ys = sqrt_q(xs ** 3 - 3 * xs + m.B)
assert m.key_point(b"\x04" + be(xs) + be(ys)) is not None and xs + Q < 1 << 256
bad_keys.append(("x + q for a point with a small x", b"\x04" + be(xs + Q) + be(ys)))
for name, kb in bad_keys:
    put("key: " + name, 1, kb, msg, sig, m.KEY)
# on the curve with x = 0 (b is a square): loads
y0 = sqrt_q(m.B)
k0 = (0, y0)
for alg in range(3):
    msg0, e = fresh(alg, "x = 0")
    kk = rng.randrange(1, N)
    r0 = m.mul(kk, G)[0] % N
    # no private key for (0, y0): a record that merely runs the arithmetic on it
    put_rs("key with x = 0: loads; the record does not verify", alg, k0, msg0, r0, rng.randrange(1, N), m.MISMATCH)

# --- precedence ---------------------------------------------------------------------
for alg in range(3):
    qp, msg, r, s = honest(alg, "precedence")
    key, sig = m.key_bytes(qp), m.encode_sig(alg, r, s)
    badkey = key[:64] + bytes([key[64] ^ 1])
    fmt = sig[:-1]
    rng_sig = m.encode_sig(alg, N, s)
    other = msg + b"?"
    put("precedence: valid", alg, key, msg, sig, m.OK)
    put("precedence: MISMATCH alone", alg, key, other, sig, m.MISMATCH)
    for kname, kb in (("key outside the table", None), ("key off the curve", badkey)):
        put("precedence: %s, valid signature" % kname, alg, kb, msg, sig, m.KEY)
        put("precedence: %s and SIG_FORMAT" % kname, alg, kb, msg, fmt, m.KEY)
        put("precedence: %s and SIG_RANGE" % kname, alg, kb, msg, rng_sig, m.KEY)
        put("precedence: %s and MISMATCH" % kname, alg, kb, other, sig, m.KEY)
    put("precedence: SIG_FORMAT and MISMATCH", alg, key, other, fmt, m.SIG_FORMAT)
    put("precedence: SIG_RANGE and MISMATCH", alg, key, other, rng_sig, m.SIG_RANGE)
    if alg:
        put("precedence: SIG_FORMAT (a byte after the sequence) and SIG_RANGE", alg, key, msg, rng_sig + b"\x00",
            m.SIG_FORMAT)
    else:
        put("precedence: SIG_FORMAT (65 bytes) and SIG_RANGE", alg, key, msg, rng_sig + b"\x00", m.SIG_FORMAT)

# --- message lengths ------------------------------------------------------------------
for alg in range(3):
    for ln in (0, 55, 56, 63, 64, 111, 112, 119, 120, 128, 1023):
        msg = bytes(rng.randrange(256) for _ in range(ln))
        qp, msg, r, s = honest(alg, "", msg=msg)
        put_rs("message of %d bytes" % ln, alg, qp, msg, r, s, m.OK)
        if ln in (0, 64, 1023):
            put_rs("message of %d bytes and one more" % ln, alg, qp, msg + b"\x00", r, s, m.MISMATCH)

out = {"judge": "tests/ecdsa_model.py alone (ring's P-256 arithmetic is assembly and was not built)", "rows": rows}
with open(os.path.join(HERE, "ecdsa_edges.json"), "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
from collections import Counter  # noqa: E402
print(len(rows), sorted(Counter(r["code"] for r in rows).items()))
