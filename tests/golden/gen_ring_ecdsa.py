#!/usr/bin/env python3
"""tests/golden/ring_ecdsa.json from the vector files of ring 0.16.9 in the
reference tree (argument: the path of its utils/ring; without one, a
`reference` directory beside the repository is tried).  Only the rows' data is kept, never
the files' text: the P-256 rows of the two verify files (all 58, Result as P or
F), of suite_b_public_key_tests.txt and of ecdsa_digest_scalar_tests.txt, and a
subset of the four p256_point_* files (every row with an infinite operand, an
equal or opposite pair or an infinite result, plus the first 32 other rows of
each file).  The point files hold Montgomery-encoded coordinates (times 2^256
mod q); the fixture holds plain integers.

Generation fails unless tests/ecdsa_model.py agrees with every P-256 row of
every file, kept or not.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ecdsa_model as m  # noqa: E402

RINV = pow(1 << 256, -1, m.Q)


def blocks(path):
    cur = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                if cur and not line:
                    yield cur
                    cur = {}
                continue
            k, v = line.split("=", 1)
            k, v = k.strip(), v.strip()
            if k in cur:        # (files without blank lines between rows)
                yield cur
                cur = {}
            cur[k] = v
    if cur:
        yield cur


def value_bytes(v):
    if v.startswith('"'):
        return v[1:v.rindex('"')].encode()
    return bytes.fromhex(v)


def jac(v):
    """'X, Y, Z' or 'X, Y' (Montgomery-encoded) or 'inf' -> plain [X, Y, Z] / [x, y] / None"""
    if v == "inf":
        return None
    return [int(t.strip(), 16) * RINV % m.Q for t in v.split(",")]


def affine_of(p):
    if p is None:
        return None
    if len(p) == 2:
        return (p[0], p[1])
    if p[2] == 0:
        return None
    zi = pow(p[2], -1, m.Q)
    return (p[0] * zi * zi % m.Q, p[1] * zi * zi * zi % m.Q)


def hexes(p):
    return None if p is None else ["%064x" % c for c in p]


def special(*pts):
    aff = [affine_of(p) for p in pts]
    if any(a is None for a in aff):
        return True
    return len(aff) > 1 and aff[0][0] == aff[1][0]


def main():
    cands = sys.argv[1:] + [os.path.join(HERE, "..", "..", "..", "reference", "utils", "ring")]
    ring = next((c for c in cands if os.path.isdir(c)), None)
    if ring is None:
        sys.exit("ring's tree not found")
    out = {"source": "ring 0.16.9 test vectors: rows' data only", "verify": [], "keys": [], "digest_scalar": [],
           "point_sum": [], "point_sum_mixed": [], "point_double": [], "point_mul": []}
    algs = {("fixed", "SHA256"): m.ALG_P256_SHA256_FIXED, ("asn1", "SHA256"): m.ALG_P256_SHA256_ASN1,
            ("asn1", "SHA384"): m.ALG_P256_SHA384_ASN1}
    for form in ("fixed", "asn1"):
        for b in blocks(os.path.join(ring, "tests", "ecdsa_verify_%s_tests.txt" % form)):
            if b["Curve"] != "P-256":
                continue
            alg = algs[(form, b["Digest"])]
            key, msg, sig = value_bytes(b["Q"]), value_bytes(b["Msg"]), value_bytes(b["Sig"])
            res = b["Result"][0]
            assert res in "PF"
            code = m.verify_code(alg, key, msg, sig)
            assert (code == m.OK) == (res == "P"), b
            out["verify"].append({"alg": alg, "key": key.hex(), "msg": msg.hex(), "sig": sig.hex(), "result": res,
                                  "code": code})
    counts = [sum(1 for r in out["verify"] if r["alg"] == a) for a in range(3)]
    assert counts == [13, 28, 17], counts
    for b in blocks(os.path.join(ring, "src", "ec", "suite_b", "suite_b_public_key_tests.txt")):
        if b["Curve"] != "P-256":
            continue
        key, res = value_bytes(b["Q"]), b["Result"][0]
        assert (m.key_point(key) is not None) == (res == "P"), b
        out["keys"].append({"key": key.hex(), "result": res})
    for b in blocks(os.path.join(ring, "src", "ec", "suite_b", "ecdsa", "ecdsa_digest_scalar_tests.txt")):
        if b["Curve"] != "P-256":
            continue
        d, o = value_bytes(b["Input"]), value_bytes(b["Output"])
        assert m.digest_to_scalar(d) == int.from_bytes(o, "big"), b
        out["digest_scalar"].append({"digest": b["Digest"], "input": d.hex(), "output": o.hex()})
    ops = os.path.join(ring, "src", "ec", "suite_b", "ops")
    for name, two in (("point_sum", True), ("point_sum_mixed", True), ("point_double", False)):
        plain = 0
        for b in blocks(os.path.join(ops, "p256_%s_tests.txt" % name)):
            a, r = jac(b["a"]), jac(b["r"])
            bb = jac(b["b"]) if two else None
            if two and len(bb) == 2 and bb == [0, 0]:
                bb = None                    # ring's mixed addition takes (0, 0) as infinity
            pa, pb = affine_of(a), affine_of(bb) if two else None
            want = m.add(pa, pb) if two else m.add(pa, pa)
            assert want == affine_of(r), (name, b)
            sp = special(a, bb) if two else special(a)
            sp = sp or r is None
            if not sp:
                plain += 1
                if plain > 32:
                    continue
            row = {"a": hexes(a), "r": hexes(r)}
            if two:
                row["b"] = hexes(bb)
            out[name].append(row)
    plain = 0
    for b in blocks(os.path.join(ops, "p256_point_mul_tests.txt")):
        k, p, r = int(b["p_scalar"], 16), jac(b["p"]), jac(b["r"])
        assert m.mul(k, affine_of(p)) == affine_of(r) and k < m.N, b
        if r is not None:
            plain += 1
            if plain > 32:
                continue
        out["point_mul"].append({"k": "%064x" % k, "p": hexes(p), "r": hexes(r)})
    with open(os.path.join(HERE, "ring_ecdsa.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in out.items() if isinstance(v, list)})


if __name__ == "__main__":
    main()
