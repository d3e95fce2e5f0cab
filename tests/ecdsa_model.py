"""ECDSA P-256 verification under ring 0.16.9's rules, in plain Python integers
(include/cess_ecdsa.h states the rules and their sources).  The judge of the
fixtures under tests/golden/ and of the host and GPU builds; it also has a
signer, for making test data only (no side-channel care, caller-chosen nonces).
"""
import hashlib

Q = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
B = 0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b
GX = 0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296
GY = 0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5
G = (GX, GY)

ALG_P256_SHA256_FIXED, ALG_P256_SHA256_ASN1, ALG_P256_SHA384_ASN1 = 0, 1, 2
OK, SIG_FORMAT, SIG_RANGE, KEY, MISMATCH = range(5)
CODE_NAMES = {0: "OK", 1: "SIG_FORMAT", 2: "SIG_RANGE", 3: "KEY", 4: "MISMATCH"}


# --- the curve, affine, None = infinity -------------------------------------
def on_curve(x, y):
    return (y * y - (x * x * x - 3 * x + B)) % Q == 0


def neg(p):
    return None if p is None else (p[0], (-p[1]) % Q)


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % Q == 0:
            return None
        lam = (3 * x1 * x1 - 3) * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return (x3, (lam * (x1 - x3) - y1) % Q)


def mul(k, p):
    k %= N
    r = None
    while k:
        if k & 1:
            r = add(r, p)
        p = add(p, p)
        k >>= 1
    return r


# --- rule 1: the key ----------------------------------------------------------
def key_point(key: bytes):
    """(x, y), or None where the key does not load."""
    if len(key) != 65 or key[0] != 4:
        return None
    x, y = int.from_bytes(key[1:33], "big"), int.from_bytes(key[33:], "big")
    if x >= Q or y >= Q or not on_curve(x, y):
        return None
    return (x, y)


def key_bytes(p) -> bytes:
    return b"\x04" + p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")


# --- rule 2: the signature split ---------------------------------------------
def _der_tlv(b: bytes, at: int):
    """ring's der::read_tag_and_get_value: (tag, value, next) or None."""
    if at + 2 > len(b):
        return None
    tag = b[at]
    if tag & 0x1f == 0x1f:
        return None
    ln = b[at + 1]
    at += 2
    if ln >= 0x80:
        if ln == 0x81:
            if at + 1 > len(b) or b[at] < 128:
                return None
            ln, at = b[at], at + 1
        elif ln == 0x82:
            if at + 2 > len(b):
                return None
            ln, at = (b[at] << 8) | b[at + 1], at + 2
            if ln < 256:
                return None
        else:
            return None
    if at + ln > len(b):
        return None
    return tag, b[at:at + ln], at + ln


def _der_positive_integer(b: bytes, at: int):
    """ring's der::positive_integer: (value bytes without the leading zero, next) or None."""
    t = _der_tlv(b, at)
    if t is None or t[0] != 0x02:
        return None
    v = t[1]
    if len(v) == 0:
        return None
    if v[0] == 0:
        if len(v) == 1:
            return None                      # the value zero
        if v[1] & 0x80 == 0:
            return None                      # a leading zero that is not needed
        return v[1:], t[2]
    if v[0] & 0x80:
        return None                          # negative
    return v, t[2]


def split_sig(alg: int, sig: bytes):
    """(r bytes, s bytes) big-endian, of any length, or None: SIG_FORMAT."""
    if alg == ALG_P256_SHA256_FIXED:
        if len(sig) != 64:
            return None
        return sig[:32], sig[32:]
    t = _der_tlv(sig, 0)
    if t is None or t[0] != 0x30 or t[2] != len(sig):
        return None
    body = t[1]
    r = _der_positive_integer(body, 0)
    if r is None:
        return None
    s = _der_positive_integer(body, r[1])
    if s is None or s[1] != len(body):
        return None
    return r[0], s[0]


# --- rule 4 -------------------------------------------------------------------
def digest_scalar(alg: int, msg: bytes) -> int:
    d = (hashlib.sha384 if alg == ALG_P256_SHA384_ASN1 else hashlib.sha256)(msg).digest()
    return digest_to_scalar(d)


def digest_to_scalar(d: bytes) -> int:
    e = int.from_bytes(d[:32], "big")
    return e - N if e >= N else e


# --- rules 3, 5, 6 on integers ------------------------------------------------
def verify_scalars(e: int, r: int, s: int, qp) -> int:
    if not (1 <= r < N and 1 <= s < N):
        return SIG_RANGE
    w = pow(s, -1, N)
    R = add(mul(e * w % N, G), mul(r * w % N, qp))
    if R is None:
        return MISMATCH
    # ring: r Z^2 = X, and (r + n) Z^2 = X if r < q - n; on affine x: x = r or x = r + n
    if R[0] == r or (r < Q - N and R[0] == r + N):
        return OK
    return MISMATCH


def verify_code(alg: int, key, msg: bytes, sig: bytes) -> int:
    """key: the key's bytes, or None for an index outside the table."""
    qp = key_point(key) if key is not None else None
    if qp is None:
        return KEY
    rs = split_sig(alg, sig)
    if rs is None:
        return SIG_FORMAT
    r, s = int.from_bytes(rs[0], "big"), int.from_bytes(rs[1], "big")
    return verify_scalars(digest_scalar(alg, msg), r, s, qp)


# --- test data ----------------------------------------------------------------
def der_int(v: int, nbytes=None) -> bytes:
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big") if nbytes is None else v.to_bytes(nbytes, "big")
    if b[0] & 0x80:
        b = b"\x00" + b
    return b"\x02" + der_len(len(b)) + b


def der_len(n: int) -> bytes:
    if n < 128:
        return bytes([n])
    if n < 256:
        return bytes([0x81, n])
    return bytes([0x82, n >> 8, n & 255])


def encode_sig(alg: int, r: int, s: int) -> bytes:
    if alg == ALG_P256_SHA256_FIXED:
        return r.to_bytes(32, "big") + s.to_bytes(32, "big")
    body = der_int(r) + der_int(s)
    return b"\x30" + der_len(len(body)) + body


def sign(alg: int, d: int, k: int, msg: bytes):
    """(r, s) with the caller's nonce k; None where r or s comes out zero.  Test data only."""
    e = digest_scalar(alg, msg)
    r = mul(k, G)[0] % N
    s = pow(k, -1, N) * (e + r * d) % N
    return (r, s) if r and s else None
