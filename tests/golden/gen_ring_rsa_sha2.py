"""Generate the SHA-384 / SHA-512 fixtures from the reference's ring vectors:

tests/golden/ring_rsa_pkcs1_sha384_sha512.json
    the 75 `Digest = SHA384 | SHA512` rows of utils/ring/tests/
    rsa_pkcs1_verify_tests.txt (38 + 37), each an RSASSA-PKCS1-v1_5
    verification under ring's RSA_PKCS1_2048_8192_SHA384 / _SHA512 with its
    expected Result (P / F).  Fields as in ring_rsa_pkcs1_sha256.json
    (gen_ring_rsa.py) plus `digest`.
tests/golden/ring_digest_sha384_sha512.json
    the 4 `Hash = SHA384 | SHA512` rows of utils/ring/tests/digest_tests.txt
    (2 + 2; the file's other 31 rows that a search for "SHA512" finds are
    `Hash = SHA512_256`, another algorithm that no signature scheme here uses)
    as (hash, input hex, repeat, output hex); `repeat` stays a number and is
    expanded where the row is used (every one of these rows has repeat 1).

key_status and code come from each row's Result and from the plain-Python model
(hashlib, pow, the strict DER parser of gen_ring_rsa.py); the library is never
used.  The model must reproduce every Result and every digest, or generation
fails.

Runs only where the reference tree is present.
Usage: python tests/golden/gen_ring_rsa_sha2.py [path/to/ring/tests]
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_ring_rsa import GPU_MAX_BITS, MISMATCH, MSG_LEN, OK, SIG_LEN, SIG_RANGE, BadKey, ring_key, rows_of, unhex  # noqa: E402

DEFAULT_DIR = "/root/reference/utils/ring/tests"
PREFIX = {"SHA384": bytes.fromhex("3041300d060960864801650304020205000430"),
          "SHA512": bytes.fromhex("3051300d060960864801650304020305000440")}
HASH = {"SHA384": hashlib.sha384, "SHA512": hashlib.sha512}
EXPECT = {"SHA384": {"rows": 38, "P": 7, MISMATCH: 30, SIG_RANGE: 1, "bits": {2048, 3072}, "lens": {0, 128}},
          "SHA512": {"rows": 37, "P": 7, MISMATCH: 29, SIG_LEN: 1, "bits": {2048, 3072, 4096}, "lens": {127, 128}}}


def model_code(digest, n, e, msg, sig):
    k = (n.bit_length() + 7) // 8
    if len(sig) != k:
        return SIG_LEN
    t = PREFIX[digest] + HASH[digest](msg).digest()
    if k < len(t) + 11:
        return MSG_LEN
    s = int.from_bytes(sig, "big")
    if s >= n:
        return SIG_RANGE
    em = pow(s, e, n).to_bytes(k, "big")
    return OK if em == b"\x00\x01" + b"\xff" * (k - len(t) - 3) + b"\x00" + t else MISMATCH


def signature_rows(src):
    out = []
    for r in rows_of(src):
        if r["Digest"] not in PREFIX:
            continue
        key, msg, sig = unhex(r["Key"]), unhex(r["Msg"]), unhex(r["Sig"])
        try:
            n, e = ring_key(key)
            status = "ok" if n.bit_length() <= GPU_MAX_BITS else "unsupported"
            code = model_code(r["Digest"], n, e, msg, sig)
        except BadKey:
            status, code = "bad_key", None
        passed = status != "bad_key" and code == OK
        assert passed == (r["Result"] == "P"), (r["comment"], status, code, r["Result"])
        out.append({"comment": r["comment"], "digest": r["Digest"], "key": key.hex(), "msg": msg.hex(), "sig": sig.hex(),
                    "result": r["Result"], "key_status": status, "code": code if status == "ok" else None})
    for d, want in EXPECT.items():
        rows = [x for x in out if x["digest"] == d]
        assert len(rows) == want["rows"], (d, len(rows))
        assert all(x["key_status"] == "ok" for x in rows), d
        assert sum(x["result"] == "P" for x in rows) == want["P"], d
        for c in (SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH):
            assert sum(x["code"] == c for x in rows) == want.get(c, 0), (d, c)
        assert {ring_key(bytes.fromhex(x["key"]))[0].bit_length() for x in rows} == want["bits"], d
        assert {len(x["msg"]) // 2 for x in rows} == want["lens"], d
    return out


def digest_rows(src):
    out, cur = [], {}
    for line in open(src):
        line = line.rstrip("\n")
        if line.startswith("#") or " = " not in line:
            continue
        k, v = line.split(" = ", 1)
        cur[k] = v
        if k == "Output":
            if cur["Hash"] in HASH:
                v = cur["Input"]
                data = v[1:-1].encode() if v.startswith('"') else bytes.fromhex(v)
                assert "\\" not in v
                rep = int(cur["Repeat"])
                assert HASH[cur["Hash"]](data * rep).hexdigest() == cur["Output"], cur
                out.append({"hash": cur["Hash"], "input": data.hex(), "repeat": rep, "output": cur["Output"]})
            cur = {}
    assert len(out) == 4, len(out)
    return out


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_DIR
    sig = signature_rows(os.path.join(src, "rsa_pkcs1_verify_tests.txt"))
    dst = os.path.join(HERE, "ring_rsa_pkcs1_sha384_sha512.json")
    with open(dst, "w") as f:
        json.dump({"source": "ring tests/rsa_pkcs1_verify_tests.txt, Digest = SHA384 and SHA512 rows",
                   "algorithm": "RSA_PKCS1_2048_8192_SHA384 / RSA_PKCS1_2048_8192_SHA512", "rows": sig}, f, indent=0)
        f.write("\n")
    print(dst, len(sig), "rows")
    dig = digest_rows(os.path.join(src, "digest_tests.txt"))
    dst = os.path.join(HERE, "ring_digest_sha384_sha512.json")
    with open(dst, "w") as f:
        json.dump({"source": "ring tests/digest_tests.txt, Hash = SHA384 and SHA512 rows", "rows": dig}, f, indent=0)
        f.write("\n")
    print(dst, len(dig), "rows", {h: sum(1 for x in dig if x["hash"] == h) for h in HASH},
          "max repeat", max(x["repeat"] for x in dig))


if __name__ == "__main__":
    main()
