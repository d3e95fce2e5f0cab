"""Writes tests/golden/ed25519_sign_edges.json, the edge fixture of the Ed25519
signer (include/cess_ed25519_sign.h).  Pure Python on tests/ed25519_model.py
(hashlib and integers); run from anywhere:  python tests/golden/gen_ed25519_sign_edges.py

rows      seeds chosen for their clamped scalar, each signed over messages at the
          SHA-512 padding and block edges of both hash inputs (32 + len and
          64 + len bytes); pub and sig from the model
scalars   k and encode([k]B) for the fixed-base multiplication
muladd    (k, a, r, (k a + r) mod L)
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ed25519_model as model  # noqa: E402

L = model.L
MSG_LENS = [0, 1, 47, 48, 63, 64, 65, 79, 80, 95, 96, 97, 111, 112, 127, 128, 129, 1023]
RECODE_BOUND = 2**256 * 7 // 15          # sc_recode is exact below this


def clamped(seed):
    return model._clamp(hashlib.sha512(seed).digest()[:32])


def find_seed(top, nxt):
    """the first counter whose 32-byte little-endian form is a seed with these two top bytes of the clamped scalar"""
    c = 0
    while True:
        seed = c.to_bytes(32, "little")
        a = clamped(seed).to_bytes(32, "little")
        if a[31] == top and a[30] == nxt:
            return c, seed
        c += 1


def message(seed, n):
    out = b""
    while len(out) < n:
        out += hashlib.sha512(seed + len(out).to_bytes(4, "little")).digest()
    return out[:n]


def main():
    c_hi, seed_hi = find_seed(0x7f, 0xff)
    c_lo, seed_lo = find_seed(0x40, 0x00)
    assert c_hi == 5775 and clamped(seed_hi) >= RECODE_BOUND > clamped(seed_lo)
    seeds = [("clamped scalar 0x7fff.. (recode overflow), counter %d" % c_hi, seed_hi),
             ("clamped scalar 0x4000.., counter %d" % c_lo, seed_lo),
             ("bytes(range(32))", bytes(range(32))),
             ("all-zero seed", bytes(32))]
    rows = []
    for name, seed in seeds:
        pub = model.public_key(seed)
        for n in MSG_LENS:
            msg = message(seed, n)
            rows.append({"name": "%s, %d-byte message" % (name, n), "seed": seed.hex(), "msg": msg.hex(),
                         "pub": pub.hex(), "sig": model.sign(seed, msg).hex()})
    ks = [0, 1, 2, 7, 8, 9, 15, 16, int("7" * 63, 16), int("8" * 63, 16), int("f" * 62, 16),
          2**252 - 1, 2**252, L - 2, L - 1]
    for i in (1, 31, 32, 62):
        ks += [2**(4 * i), 2**(4 * i) - 1]
    assert all(k < L for k in ks)
    scalars = [{"k": "%x" % k, "enc": model.encode(model.mul(k, model.B) if k else (0, 1)).hex()} for k in ks]
    a_hi = clamped(seed_hi)
    triples = [(L - 1, 2**255 - 8, L - 1), (0, a_hi, 12345), (0, 2**255 - 8, L - 1), (L - 1, a_hi, 0), (7, a_hi % L, 0),
               (L - 1, a_hi % L, L - 1), (2**256 - 1, 2**256 - 1, 2**256 - 1), (1, 0, 0), (0, 0, 0), (2, L - 1, 2)]
    h = hashlib.sha512(b"ed25519 sign edges").digest()
    for i in range(6):
        h = hashlib.sha512(h).digest()
        k, r = int.from_bytes(h[:32], "little") % L, int.from_bytes(h[32:], "little") % L
        triples.append((k, clamped(h[:32]) % L, r))
    muladd = [{"k": "%x" % k, "a": "%x" % a, "r": "%x" % r, "s": "%x" % ((k * a + r) % L)} for k, a, r in triples]
    out = {"source": "tests/golden/gen_ed25519_sign_edges.py over tests/ed25519_model.py",
           "overflow_seed": seed_hi.hex(), "rows": rows, "scalars": scalars, "muladd": muladd}
    with open(os.path.join(HERE, "ed25519_sign_edges.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("%d rows, %d scalars, %d triples" % (len(rows), len(scalars), len(muladd)))


if __name__ == "__main__":
    main()
