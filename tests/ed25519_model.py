"""Plain-Python model of the Ed25519 verification rules the GPU library
reproduces (include/cess_ed25519.h, CESS_ED25519_POLICY_RING): ring's
`signature::ED25519` as read from its source (ed25519/verification.rs,
scalar.rs, and the point decoding of third_party/fiat/curve25519.c).  hashlib,
pow and integer point arithmetic only; the library is never used.  Also signs
(RFC 8032 §5.1.6), for the generated fixture rows.

Codes (cess_ed25519_code): 0 OK, 1 SIG_LEN, 2 SIG_RANGE, 3 KEY, 4 MISMATCH.
Precedence: KEY for a missing or short key, SIG_LEN, SIG_RANGE, KEY for a key
that does not decode, MISMATCH.
"""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
OK, SIG_LEN, SIG_RANGE, KEY, MISMATCH = range(5)


def decode_point(key):
    """(x, y) of a 32-byte encoding under ring's rules, or None: y is the low 255
    bits reduced mod p with no canonical check; x = 0 with the sign bit set is
    accepted (x stays 0); no small-order or subgroup check."""
    if len(key) != 32:
        return None
    v = int.from_bytes(key, "little")
    sign, y = v >> 255, (v & (2**255 - 1)) % P
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(w, 3, P) * pow(u * pow(w, 7, P), (P - 5) // 8, P) % P
    if (w * x * x - u) % P:
        if (w * x * x + u) % P:
            return None
        x = x * SQRT_M1 % P
    if x & 1 != sign:
        x = -x % P
    return x, y


def add(p, q):
    """complete twisted Edwards addition (a = -1), affine"""
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def _ext_add(p, q):
    """the same addition on extended coordinates (X, Y, Z, T), without the inversions"""
    (x1, y1, z1, t1), (x2, y2, z2, t2) = p, q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def mul(k, p):
    """[k]p, affine in and out (double-and-add on extended coordinates, one inversion)"""
    r, q = (0, 1, 1, 0), (p[0], p[1], 1, p[0] * p[1] % P)
    while k:
        if k & 1:
            r = _ext_add(r, q)
        q = _ext_add(q, q)
        k >>= 1
    zi = pow(r[2], P - 2, P)
    return r[0] * zi % P, r[1] * zi % P


def encode(p):
    return (p[1] | (p[0] & 1) << 255).to_bytes(32, "little")


BY = 4 * pow(5, P - 2, P) % P
B = decode_point(BY.to_bytes(32, "little"))


def verify_code(key, msg, sig, key_present=True):
    """the record's code; key_present False models a key index outside the table"""
    if not key_present or len(key) != 32:
        return KEY
    if len(sig) != 64:
        return SIG_LEN
    s = int.from_bytes(sig[32:], "little")
    if s >= L:
        return SIG_RANGE
    a = decode_point(key)
    if a is None:
        return KEY
    h = int.from_bytes(hashlib.sha512(sig[:32] + key + msg).digest(), "little") % L
    r = add(mul(s, B), mul(h, (-a[0] % P, a[1])))
    return OK if encode(r) == sig[:32] else MISMATCH


def key_loads(key):
    return decode_point(key) is not None


def public_key(seed):
    a = _clamp(hashlib.sha512(seed).digest()[:32])
    return encode(mul(a, B))


def _clamp(h32):
    a = int.from_bytes(h32, "little")
    return (a & ((1 << 254) - 8)) | (1 << 254)


def sign(seed, msg):
    """RFC 8032 §5.1.6"""
    h = hashlib.sha512(seed).digest()
    a, prefix = _clamp(h[:32]), h[32:]
    pub = encode(mul(a, B))
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    rb = encode(mul(r, B))
    k = int.from_bytes(hashlib.sha512(rb + pub + msg).digest(), "little") % L
    return rb + ((r + k * a) % L).to_bytes(32, "little")


def neg_multiples(key):
    """affine table entries (y + x, y - x, 2 d x y) of i * (-A), i = 1..8"""
    a = decode_point(key)
    na = (-a[0] % P, a[1])
    out, q = [], (0, 1)
    for _ in range(8):
        q = add(q, na)
        out.append(((q[1] + q[0]) % P, (q[1] - q[0]) % P, 2 * D * q[0] * q[1] % P))
    return out
