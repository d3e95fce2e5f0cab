"""Generate tests/golden/ed25519_edges.json: crafted Ed25519 records and keys on
the edges of the rule set of include/cess_ed25519.h (ring's ED25519), each with
the code the plain-Python model (tests/ed25519_model.py) gives it.  Fixed
seeds: the output is reproducible.

  keys  {"name", "key", "loads"}: encodings of y in a small range, canonical and
        + p, with both sign bits; lengths 0, 31, 33
  rows  {"name", "group", "key", "msg", "sig", "code"}

Usage: python tests/golden/gen_ed25519_edges.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ed25519_model as m  # noqa: E402

P, L = m.P, m.L


def rnd(tag, n):
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha512(b"ed25519_edges|%s|%d" % (tag.encode(), i)).digest()
        i += 1
    return out[:n]


def enc_y(y, sign):
    return (y | sign << 255).to_bytes(32, "little")


def main():
    rows, keys = [], []

    def row(name, group, key, msg, sig, expect=None):
        code = m.verify_code(key, msg, sig)
        assert expect is None or code == expect, (name, code, expect)
        rows.append({"name": name, "group": group, "key": key.hex(), "msg": msg.hex(), "sig": sig.hex(),
                     "code": code})

    # --- the identity key: [h]A is the identity, so R' = [S]B for any message
    ident = enc_y(1, 0)
    s = int.from_bytes(rnd("ident-s", 32), "little") % L
    sb = m.encode(m.mul(s, m.B)) + s.to_bytes(32, "little")
    for j, msg in enumerate((b"", rnd("ident-m1", 32), rnd("ident-m2", 100))):
        row("identity key, sig = enc([S]B) || S, message %d" % j, "identity", ident, msg, sb, m.OK)
    row("identity key with the sign bit set (x = 0 stays 0)", "identity", enc_y(1, 1), rnd("ident-m3", 32), sb, m.OK)
    row("identity key encoded as p + 1", "identity", enc_y(P + 1, 0), rnd("ident-m4", 32), sb, m.OK)
    zero_s = bytes(32)
    row("identity key, S = 0, R = 01 00..00", "identity", ident, b"m", enc_y(1, 0) + zero_s, m.OK)
    row("identity key, S = 0, R = the p + 1 encoding (never matches)", "identity", ident, b"m",
        enc_y(P + 1, 0) + zero_s, m.MISMATCH)

    # --- low-order and off-curve keys; the encodings of small y
    row("key y = 0 (order 4)", "low_order", enc_y(0, 0), rnd("lo-m", 32), rnd("lo-r", 32) + (7).to_bytes(32, "little"))
    for y in (2, 7, 8, 11):
        assert not m.key_loads(enc_y(y, 0))
        keys.append({"name": "y = %d is off the curve" % y, "key": enc_y(y, 0).hex(), "loads": False})
        row("off-curve key y = %d" % y, "bad_key", enc_y(y, 0), b"x", sb, m.KEY)
    for y in (0, 1, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18):
        for yy, form in ((y, "canonical"), (y + P, "+ p")):
            for sign in (0, 1):
                k = enc_y(yy, sign)
                assert m.key_loads(k), (y, form, sign)
                keys.append({"name": "y = %d %s, sign bit %d" % (y, form, sign), "key": k.hex(), "loads": True})
    for ln in (0, 31, 33):
        k = rnd("klen%d" % ln, ln)
        keys.append({"name": "key of %d bytes" % ln, "key": k.hex(), "loads": False})
        row("key of %d bytes" % ln, "bad_key", k, b"x", sb, m.KEY)

    # --- scalar range, on a valid row
    seed = rnd("seed0", 32)
    pub, msg = m.public_key(seed), rnd("msg0", 32)
    sig = m.sign(seed, msg)
    row("valid base row", "range", pub, msg, sig, m.OK)
    s0 = int.from_bytes(sig[32:], "little")
    assert s0 + L < 2**256
    for name, sv, expect in (("S + L", s0 + L, m.SIG_RANGE), ("S = L", L, m.SIG_RANGE), ("S = L - 1", L - 1, m.MISMATCH),
                             ("S = 2^256 - 1", 2**256 - 1, m.SIG_RANGE)):
        row(name, "range", pub, msg, sig[:32] + sv.to_bytes(32, "little"), expect)

    # --- lengths
    for ln in (0, 63, 65):
        row("signature of %d bytes" % ln, "length", pub, msg, (sig + b"\x00")[:ln], m.SIG_LEN)

    # --- ordinary failures
    row("wrong key", "failure", m.public_key(rnd("seed1", 32)), msg, sig, m.MISMATCH)
    for name, pos in (("R", 5), ("S", 40)):
        for bit in (0, 7):
            t = bytearray(sig)
            t[pos] ^= 1 << bit
            row("bit %d of byte %d flipped (%s)" % (bit, pos, name), "failure", pub, msg, bytes(t))
    t = bytearray(sig)
    t[63] ^= 0x80                     # pushes S past L
    row("top bit of S flipped", "failure", pub, msg, bytes(t), m.SIG_RANGE)
    t = bytearray(msg)
    t[0] ^= 1
    row("bit flipped in the message", "failure", pub, bytes(t), sig, m.MISMATCH)

    # --- SHA-512 padding and block edges of 64 + len, and the four byte alignments
    for ln in (0, 47, 48, 63, 64, 65, 175, 176, 191, 192, 193, 1000):
        sd, ms = rnd("sha-seed%d" % ln, 32), rnd("sha-msg%d" % ln, ln)
        row("valid, message of %d bytes" % ln, "sha512", m.public_key(sd), ms, m.sign(sd, ms), m.OK)
    # consecutive messages of 5, 6, 7, 8 bytes start at offsets 0, 5, 11, 18 of a batch buffer: 0, 1, 3, 2 mod 4
    for ln in (5, 6, 7, 8):
        sd, ms = rnd("al-seed%d" % ln, 32), rnd("al-msg%d" % ln, ln)
        row("valid, message of %d bytes (alignment group)" % ln, "align", m.public_key(sd), ms, m.sign(sd, ms), m.OK)

    dst = os.path.join(HERE, "ed25519_edges.json")
    with open(dst, "w") as f:
        json.dump({"source": "tests/golden/gen_ed25519_edges.py (tests/ed25519_model.py)", "keys": keys, "rows": rows},
                  f, indent=0)
        f.write("\n")
    print(dst, len(keys), "keys", len(rows), "rows",
          {c: sum(1 for r in rows if r["code"] == c) for c in range(5)})


if __name__ == "__main__":
    main()
