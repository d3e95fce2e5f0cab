"""Plain-Python model (hashlib, pow) of RSASSA-PSS verification as ring 0.16.9 does it for
RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512 (src/rsa/padding.rs `impl Verification for PSS`, PSSMetrics,
mgf1, pss_digest; src/rsa/verification.rs verify_rsa_): TEST INFRASTRUCTURE ONLY.  It is what the fixtures'
codes (tests/golden/gen_ring_rsa_pss.py, gen_rsa_pss_edges.py) and every GPU comparison come from; the
library is never used here.

The eight rules (H the digest, h its length, k the byte length of n):
 1 key     ring's Key::from_modulus_and_exponent under the 2048..8192-bit policy (ring_key of
           tests/golden/gen_ring_rsa.py: 8 k >= 2048, n odd, e odd, 3 <= e <= 2^33 - 1)
 2 length  len(sig) == k (SIG_LEN), s < n (SIG_RANGE); ring also rejects s == 0, which here is rule 5's
           failure (0^e = 0 has no 0xbc trailer): MISMATCH
 3 m       s^e mod n as k big-endian bytes
 4 lengths em_bits = mod_bits - 1, em_len = ceil(em_bits / 8), top_byte_mask = 0xff >> (8 em_len - em_bits);
           where the mask is 0xff, m's first byte must be 0 and EM is the rest
 5 layout  EM = maskedDB (em_len - h - 1) || H' (h) || 0xbc; maskedDB[0] & ~top_byte_mask == 0
 6 unmask  DB = maskedDB xor MGF1_H(H', db_len); DB[0] &= top_byte_mask
 7 padding DB = 00 x ps_len || 01 || salt (h bytes): the salt length is the digest's, nothing else
 8 hash    H(00 x 8 || H(msg) || salt) == H'
Every failure of rules 3..8 is MISMATCH (ring: error::Unspecified).
"""
import gzip
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from gen_ring_rsa import BadKey, ring_key  # noqa: E402,F401

OK, SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH, KEY = range(6)
HASH = {"SHA256": hashlib.sha256, "SHA384": hashlib.sha384, "SHA512": hashlib.sha512}
DIGEST_ID = {"SHA256": 0, "SHA384": 1, "SHA512": 2}          # CESS_RSA_DIGEST_*
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GPU_MAX_BITS = 4112      # the loop-form size class holds 8 k + 2 <= 28 x 147 bits: k <= 514 bytes


# The fixtures are hex-heavy JSON (ring_rsa_pss.json.gz, rsa_pss_edges.json.gz, rsa_pss_phase_keys.json.gz): kept gzipped, written
# without a time stamp so that regenerating them gives the same bytes.  `zcat FILE | python -m json.tool` reads one.
# Beside each lies NAME.codes.txt, one line per row with what identifies the row and its recorded code: the part
# of a fixture that a diff should show.  tests/test_rsa_pss.py holds the two together.
def load_fixture(name: str):
    with gzip.open(os.path.join(GOLDEN, name), "rt") as f:
        return json.load(f)


def codes_path(name: str) -> str:
    return os.path.join(GOLDEN, name[:-len(".json.gz")] + ".codes.txt")


def code_lines(obj) -> list:
    """the rows of either fixture as text: what names the row, then its code"""
    out = []
    for r in obj.get("verify", []):
        out.append("verify %s %s key_status=%s code=%s sig=%s.." % (r["digest"], r["result"], r["key_status"], r["code"],
                                                                   r["sig"][:16]))
    for r in obj.get("padding", []):
        out.append("padding %s bits=%d %s code=%s em=%s.." % (r["digest"], r["bits"], r["result"], r["code"], r["em"][:16]))
    names = [k["name"] for k in obj.get("keys", [])]
    for t, k in zip(obj.get("table", []), names + ["-"] * len(obj.get("table", []))):
        out.append("table %s status=%s" % (k, t["status"]))
    for r in obj.get("rows", []):
        out.append("row %s key=%s %s code=%d" % (r["digest"], names[r["key"]] if r["key"] < len(names) else r["key"],
                                                 r["case"], r["code"]))
    return out


def dump_fixture(name: str, obj) -> str:
    dst = os.path.join(GOLDEN, name)
    with open(dst, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write((json.dumps(obj, indent=0) + "\n").encode())
    with open(codes_path(name), "w") as f:
        f.write("\n".join(code_lines(obj)) + "\n")
    return dst


def mgf1(H, seed: bytes, length: int) -> bytes:
    out = b""
    for i in range((length + H().digest_size - 1) // H().digest_size):
        out += H(seed + i.to_bytes(4, "big")).digest()
    return out[:length]


def em_ok(digest: str, m_hash: bytes, m: bytes, mod_bits: int) -> bool:
    """PSS::verify over the k bytes of m (rules 4..8): ring reads m to its end, so any other length fails."""
    H = HASH[digest]
    h = H().digest_size
    if mod_bits < 1:
        return False
    em_bits = mod_bits - 1
    em_len = (em_bits + 7) // 8
    top = 0xff >> (8 * em_len - em_bits)
    db_len = em_len - 1 - h
    ps_len = db_len - h - 1
    if db_len < 0 or ps_len < 0:
        return False
    if top == 0xff:
        if not m or m[0] != 0:
            return False
        m = m[1:]
    if len(m) != em_len:
        return False
    masked, hp, trailer = m[:db_len], m[db_len:db_len + h], m[-1]
    if trailer != 0xbc or masked[0] & ~top & 0xff:
        return False
    db = bytearray(a ^ b for a, b in zip(masked, mgf1(H, hp, db_len)))
    db[0] &= top
    if any(db[:ps_len]) or db[ps_len] != 1:
        return False
    salt = bytes(db[db_len - h:])
    return H(bytes(8) + m_hash + salt).digest() == hp


def em_code(digest: str, msg: bytes, em: bytes, mod_bits: int) -> int:
    return OK if em_ok(digest, HASH[digest](msg).digest(), em, mod_bits) else MISMATCH


def verify_code(digest: str, n: int, e: int, msg: bytes, sig: bytes) -> int:
    """Rules 2..8 for a key that rule 1 accepted."""
    k = (n.bit_length() + 7) // 8
    if len(sig) != k:
        return SIG_LEN
    s = int.from_bytes(sig, "big")
    if s >= n:
        return SIG_RANGE
    return em_code(digest, msg, pow(s, e, n).to_bytes(k, "big"), n.bit_length())


def key_status(der: bytes):
    """("ok" | "unsupported" | "bad_key", (n, e) or None) of an RSAPublicKey DER under ring's policy."""
    try:
        n, e = ring_key(der)
    except BadKey:
        return "bad_key", None
    return ("ok" if n.bit_length() <= GPU_MAX_BITS else "unsupported"), (n, e)


# --- encoding (fixture generation only: ring's PSS::encode with a given salt, any salt length) ----------
def encode(digest: str, msg: bytes, salt: bytes, mod_bits: int, mgf_digest: str = None) -> bytes:
    """EMSA-PSS-ENCODE (RFC 8017 section 9.1.1) as k = ceil(mod_bits / 8) bytes."""
    H, G = HASH[digest], HASH[mgf_digest or digest]
    h = H().digest_size
    em_bits = mod_bits - 1
    em_len = (em_bits + 7) // 8
    hp = H(bytes(8) + H(msg).digest() + salt).digest()
    db = bytes(em_len - len(salt) - h - 2) + b"\x01" + salt
    masked = bytearray(a ^ b for a, b in zip(db, mgf1(G, hp, len(db))))
    masked[0] &= 0xff >> (8 * em_len - em_bits)
    em = bytes(masked) + hp + b"\xbc"
    return bytes((mod_bits + 7) // 8 - em_len) + em
