"""Generate tests/golden/ring_ed25519_crafted.json: crafted Ed25519 records and
sc_reduce inputs whose expected results come from ring's own C code
(oracle/ring_ed25519_ref.py builds oracle/_ref/libring_ed25519.so from the
reference tree), not from this project's reading of it.

Groups (each record row: name, group, key, msg, sig, code; all hex):
  torsion_key   the eight torsion points as keys, their + p encodings that fit
                255 bits and the sign-bit-set encodings of those with x = 0;
                for each key two S, and R = enc([S]B + T) for all eight T
  mixed_key     an honest key plus each non-trivial torsion point; R = enc([r]B
                + T) for all eight T with S = r + h a, and an honest signature
                of the untwisted key
  noncanonical  y and y + p for y in 0..18, both sign bits, as keys, one record
                each; R as the + p encoding and as "x = 0 with the sign bit
                set" of a point that matches in its canonical encoding
  scalar        S in {0, 1, L - 1, 0x0777..78, 0x0777..77, 2^252}, each with
                the R that makes it valid
`keys`: every distinct key with ring's "decodes" and, where it does, ring's x.
`reduce`: 64-byte inputs, ring's GFp_x25519_sc_reduce output, and the number of
final subtractions sc_reduce512 takes on them (the mirror of its v formula in
tests/ed25519_probe_model.py): every count 0..3 must occur.

Generation fails if the Python model (tests/ed25519_model.py) disagrees with
the reference on any row.  Reproducible: every random value comes from a seeded
generator.  Runs only where the reference tree is present.
Usage: python tests/golden/gen_ring_ed25519_crafted.py [reference root]
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import ed25519_model as model  # noqa: E402
import ed25519_probe_model as pm  # noqa: E402
from oracle import ring_ed25519_ref  # noqa: E402

P, L = model.P, model.L
SIGN = 1 << 255
S_ALL_M8 = int("07" + "77" * 30 + "78", 16)      # recoded digits all -8 below the top
S_ALL_7 = int("07" + "77" * 31, 16)              # recoded digits all 7


def enc_int(v):
    return v.to_bytes(32, "little")


def sig_of(r_bytes, s):
    return r_bytes + s.to_bytes(32, "little")


def r_candidates(s):
    """enc([s]B + T) for the eight torsion points T, in the order of pm.torsion_points()"""
    sb = model.mul(s, model.B)
    return [model.encode(model.add(sb, t)) for t in pm.torsion_points()]


def torsion_keys():
    """(name, key bytes) of every encoding asked for"""
    out = []
    for i, t in enumerate(pm.torsion_points()):
        tag = "T%d(order %d)" % (i, pm.order_of(t))
        out.append((tag, model.encode(t)))
        x, y = t
        if y + P < 2**255:
            for sign in (0, 1):
                if x == 0 or (x & 1) == sign:
                    out.append((tag + " y + p" + (", sign bit" if sign else ""), enc_int(y + P | sign << 255)))
        if x == 0:
            out.append((tag + " sign bit", enc_int(y | SIGN)))
    return out


def main():
    oracle = ring_ed25519_ref.load(sys.argv[1] if len(sys.argv) > 1 else None)
    rng = random.Random("ring-ed25519-crafted")
    rows = []

    def add(group, name, key, msg, sig):
        code = oracle.verify_code(key, msg, sig)
        want = model.verify_code(key, msg, sig)
        assert code == want, ("the model disagrees with ring's C", group, name, code, want)
        rows.append({"name": name, "group": group, "key": key.hex(), "msg": msg.hex(), "sig": sig.hex(), "code": code})
        return code

    tors = pm.torsion_points()
    assert [pm.order_of(t) for t in tors] == [1, 2, 4, 4, 8, 8, 8, 8]

    # torsion_key
    for name, key in torsion_keys():
        for si, s in enumerate((0, rng.randrange(1, L))):
            msg = bytes([rng.randrange(256) for _ in range(1 + si)])
            for ti, rb in enumerate(r_candidates(s)):
                add("torsion_key", "%s, S%d, R = [S]B + T%d" % (name, si, ti), key, msg, sig_of(rb, s))
    codes = {r["code"] for r in rows}
    assert codes == {model.OK, model.MISMATCH}, codes

    # mixed_key
    seed = bytes(rng.randrange(256) for _ in range(32))
    a = model._clamp(hashlib.sha512(seed).digest()[:32])
    pub = model.public_key(seed)
    pub_pt = model.decode_point(pub)
    for ti, t in enumerate(tors[1:], 1):
        key = model.encode(model.add(pub_pt, t))
        msg = bytes([ti, rng.randrange(256), rng.randrange(256)])
        r = rng.randrange(1, L)
        for ri, rb in enumerate(r_candidates(r)):
            h = int.from_bytes(hashlib.sha512(rb + key + msg).digest(), "little") % L
            add("mixed_key", "honest + T%d, R = [r]B + T%d, S = r + h a" % (ti, ri), key, msg, sig_of(rb, (r + h * a) % L))
        code = add("mixed_key", "honest + T%d, the honest signature of the untwisted key" % ti, key, msg, model.sign(seed, msg))
        assert code == model.MISMATCH
    assert {r["code"] for r in rows if r["group"] == "mixed_key"} == {model.OK, model.MISMATCH}

    def matching(key, s, want_r=None):
        """(msg, R): the first message and torsion candidate that ring accepts for (key, s)"""
        for n in range(4096):
            msg = n.to_bytes(2, "little")
            for rb in r_candidates(s):
                if want_r is not None and not want_r(rb):
                    continue
                if oracle.verify_code(key, msg, sig_of(rb, s)) == model.OK:
                    return msg, rb
        raise AssertionError("no matching record")

    # noncanonical keys: one record each (valid where a small-order key allows it)
    for y in range(19):
        for plus_p in (0, 1):
            for sign in (0, 1):
                key = enc_int(y + plus_p * P | sign << 255)
                name = "key y = %d%s, sign %d" % (y, " + p" if plus_p else "", sign)
                s = rng.randrange(1, L)
                pt = model.decode_point(key)
                if pt is not None and pm.order_of(pt) is not None:
                    msg, rb = matching(key, s)
                else:
                    msg, rb = bytes([y, plus_p, sign]), model.encode(model.mul(s, model.B))
                add("noncanonical", name, key, msg, sig_of(rb, s))
    # noncanonical R: a record that matches, then the same with R re-encoded
    for ki, want_r, variants in (
            (0, lambda rb: rb == enc_int(1), [("+ p", enc_int(P + 1)), ("sign bit", enc_int(1 | SIGN)),
                                                ("+ p, sign bit", enc_int(P + 1 | SIGN))]),
            (1, lambda rb: rb == enc_int(P - 1), [("sign bit", enc_int(P - 1 | SIGN))]),
            (2, lambda rb: rb == enc_int(0), [("+ p", enc_int(P)), ("other sign", enc_int(SIGN))]),
            (2, lambda rb: rb == enc_int(SIGN), [("+ p", enc_int(P | SIGN)), ("other sign", enc_int(0))])):
        key = model.encode(tors[ki])
        msg, rb = matching(key, 0, want_r)
        base = "T%d key, S = 0, R = %s" % (ki, rb.hex()[:4] + ".." + rb.hex()[-2:])
        assert add("noncanonical", base + " canonical", key, msg, sig_of(rb, 0)) == model.OK
        for tag, alt in variants:
            assert add("noncanonical", base + " as " + tag, key, msg, sig_of(alt, 0)) == model.MISMATCH

    # scalar: each S with the R that makes it valid, under an order-8 key
    key8 = model.encode(tors[4])
    for tag, s in (("0", 0), ("1", 1), ("L - 1", L - 1), ("0x0777..78", S_ALL_M8), ("0x0777..77", S_ALL_7), ("2^252", 2**252)):
        assert s < L
        msg, rb = matching(key8, s)
        assert add("scalar", "S = " + tag, key8, msg, sig_of(rb, s)) == model.OK
        # and one bit of S away (S = 0: one above)
        s2 = s ^ 1 if s ^ 1 < L else s - 2
        assert add("scalar", "S = %s, low bit flipped" % tag, key8, msg, sig_of(rb, s2)) == model.MISMATCH

    # keys
    keys = []
    for k in dict.fromkeys(r["key"] for r in rows):
        kb = bytes.fromhex(k)
        got, want = oracle.decode(kb), model.decode_point(kb)
        assert got == want, ("decode", k, got, want)
        keys.append({"key": k, "loads": got is not None, "x": None if got is None else enc_int(got[0]).hex()})
    assert {k["loads"] for k in keys} == {True, False}

    # reduce
    reduce_rows = []
    for x in pm.reduce_inputs():
        xb = x.to_bytes(64, "little")
        out = oracle.sc_reduce(xb)
        assert int.from_bytes(out, "little") == x % L, hex(x)
        reduce_rows.append({"x": xb.hex(), "out": out.hex(), "subs": pm.sc_reduce_subtractions(x)})
    assert {r["subs"] for r in reduce_rows} == {0, 1, 2, 3}, sorted({r["subs"] for r in reduce_rows})

    dst = os.path.join(HERE, "ring_ed25519_crafted.json")
    head = {"source": "ring's third_party/fiat/curve25519.c behind oracle/ring_ed25519_driver.c; SHA-512 from hashlib",
            "algorithm": "ED25519"}
    with open(dst, "w") as f:
        f.write("{\n")
        for k, v in head.items():
            f.write("%s: %s,\n" % (json.dumps(k), json.dumps(v)))
        for sec, items in (("rows", rows), ("keys", keys), ("reduce", reduce_rows)):
            f.write("%s: [\n" % json.dumps(sec))
            f.write(",\n".join(json.dumps(it, separators=(",", ":")) for it in items))
            f.write("\n]%s\n" % ("," if sec != "reduce" else ""))
        f.write("}\n")
    size = os.path.getsize(dst)
    assert size < 200 * 1000, size
    accepted = sum(1 for r in rows if r["code"] == model.OK)
    print(dst, len(rows), "rows,", accepted, "accepted,", len(keys), "keys,", len(reduce_rows), "reduce inputs,", size, "bytes")


if __name__ == "__main__":
    main()
