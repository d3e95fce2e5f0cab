"""Generate tests/golden/ring_rsa_pkcs1_sha256.json from the reference's ring
vectors (utils/ring/tests/rsa_pkcs1_verify_tests.txt): the 52 `Digest = SHA256`
rows, each an RSASSA-PKCS1-v1_5 / SHA-256 verification under ring's
RSA_PKCS1_2048_8192_SHA256 with its expected Result (P / F).

Per row the file keeps key (PKCS#1 RSAPublicKey DER), msg, sig, result and the
row's comment, plus two expectation fields for the GPU library:
  key_status  "ok" | "bad_key" | "unsupported": what loading the key under the
              ring policy must report (include/cess_rsa.h)
  code        the per-record code (cess_rsa_code) where the key loads, else null
Both come from the row's Result and from the plain-Python model below (hashlib,
pow, strict DER); the library is never used.  The model must reproduce every
Result, or generation fails.

Runs only where the reference tree is present.
Usage: python tests/golden/gen_ring_rsa.py [path/to/rsa_pkcs1_verify_tests.txt]
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SRC = "/root/reference/utils/ring/tests/rsa_pkcs1_verify_tests.txt"
PREFIX = bytes.fromhex("3031300d060960864801650304020105000420")
OK, SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH = range(5)
GPU_MAX_BITS = 4096


class BadKey(ValueError):
    pass


def _tlv(b, pos):
    if pos + 2 > len(b):
        raise BadKey("truncated")
    tag, ln = b[pos], b[pos + 1]
    pos += 2
    if ln & 0x80:
        nb = ln & 0x7F
        if nb == 0 or nb > 4 or pos + nb > len(b) or b[pos] == 0:
            raise BadKey("bad length")
        ln = int.from_bytes(b[pos:pos + nb], "big")
        if ln < 0x80:
            raise BadKey("non-minimal length")
        pos += nb
    if pos + ln > len(b):
        raise BadKey("truncated value")
    return tag, b[pos:pos + ln], pos + ln


def _uint(tag, v):
    if tag != 0x02 or not v or v[0] & 0x80:
        raise BadKey("not a non-negative INTEGER")
    if len(v) > 1 and v[0] == 0 and not v[1] & 0x80:
        raise BadKey("non-minimal INTEGER")
    return int.from_bytes(v, "big")


def ring_key(der):
    """(n, e) of an RSAPublicKey DER that ring's RSA_PKCS1_2048_8192_SHA256 accepts."""
    tag, body, end = _tlv(der, 0)
    if tag != 0x30 or end != len(der):
        raise BadKey("not a SEQUENCE")
    t1, vn, p = _tlv(body, 0)
    t2, ve, p = _tlv(body, p)
    if p != len(body):
        raise BadKey("trailing bytes")
    n, e = _uint(t1, vn), _uint(t2, ve)
    k = (n.bit_length() + 7) // 8
    if 8 * k < 2048 or n.bit_length() > 8192:       # ring rounds the length up to bytes for the floor
        raise BadKey("modulus size")
    if not n & 1 or not e & 1 or not 3 <= e <= (1 << 33) - 1:
        raise BadKey("parity / exponent")
    return n, e


def model_code(n, e, msg, sig):
    k = (n.bit_length() + 7) // 8
    if len(sig) != k:
        return SIG_LEN
    t = PREFIX + hashlib.sha256(msg).digest()
    if k < len(t) + 11:
        return MSG_LEN
    s = int.from_bytes(sig, "big")
    if s >= n:
        return SIG_RANGE
    em = pow(s, e, n).to_bytes(k, "big")
    return OK if em == b"\x00\x01" + b"\xff" * (k - len(t) - 3) + b"\x00" + t else MISMATCH


def rows_of(path):
    comment, cur = [], {}
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith("#"):
            comment.append(line[1:].strip())
        elif " = " in line:
            k, v = line.split(" = ", 1)
            cur[k] = v
            if k == "Result":
                cur["comment"] = " ".join(comment)
                yield cur
                comment, cur = [], {}
        elif not line.strip() and not cur:
            comment = []        # a blank line ends a comment that belongs to no row


def unhex(v):
    return b"" if v == '""' else bytes.fromhex(v)


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SRC
    out = []
    for r in rows_of(src):
        if r["Digest"] != "SHA256":
            continue
        key, msg, sig = unhex(r["Key"]), unhex(r["Msg"]), unhex(r["Sig"])
        try:
            n, e = ring_key(key)
            status = "ok" if n.bit_length() <= GPU_MAX_BITS else "unsupported"
            code = model_code(n, e, msg, sig)
        except BadKey:
            status, code = "bad_key", None
        passed = status != "bad_key" and code == OK
        assert passed == (r["Result"] == "P"), (r["comment"], status, code, r["Result"])
        out.append({"comment": r["comment"], "key": key.hex(), "msg": msg.hex(), "sig": sig.hex(),
                    "result": r["Result"], "key_status": status, "code": code if status == "ok" else None})
    assert len(out) == 52, len(out)
    dst = os.path.join(HERE, "ring_rsa_pkcs1_sha256.json")
    with open(dst, "w") as f:
        json.dump({"source": "ring tests/rsa_pkcs1_verify_tests.txt, Digest = SHA256 rows",
                   "algorithm": "RSA_PKCS1_2048_8192_SHA256", "rows": out}, f, indent=0)
        f.write("\n")
    print(dst, len(out), "rows",
          {s: sum(1 for x in out if x["key_status"] == s) for s in ("ok", "bad_key", "unsupported")})


if __name__ == "__main__":
    main()
