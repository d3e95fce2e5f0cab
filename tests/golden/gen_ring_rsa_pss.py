"""Generate tests/golden/ring_rsa_pss.json.gz (gzipped JSON, model.load_fixture reads it) from the reference's
two ring vector files for RSASSA-PSS:

verify   the 54 rows of utils/ring/tests/rsa_pss_verify_tests.txt (18 per digest, all 2048-bit keys): a
         verification under ring's RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512 with its Result (P / F).
         Fields: comment, digest, key (RSAPublicKey DER), msg, sig (hex), result, and beside them the
         model's key_status ("ok" / "unsupported" / "bad_key") and code (None unless the key is "ok").
padding  the rows of utils/ring/src/rsa/rsa_pss_padding_tests.txt: an encoded message checked by
         PSS::verify alone for modulus lengths of 256 to 8192 bits.  Fields: comment, digest, msg, salt,
         em (hex), bits (the file's Len), result ("P" or the whole "F (...)" text) and the model's code.

The model is tests/rsa_pss_model.py (hashlib, pow); the library is never used.  The model must reproduce
every Result, or generation fails.  This script is the only thing that reads the reference tree.
Usage: python tests/golden/gen_ring_rsa_pss.py [path/to/ring]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_ring_rsa import rows_of, unhex  # noqa: E402
import rsa_pss_model as model  # noqa: E402

DEFAULT_DIR = "/root/reference/utils/ring"


def verify_rows(src):
    out = []
    for r in rows_of(src):
        key, msg, sig = unhex(r["Key"]), unhex(r["Msg"]), unhex(r["Sig"])
        status, ne = model.key_status(key)
        code = model.verify_code(r["Digest"], ne[0], ne[1], msg, sig) if status != "bad_key" else None
        passed = status != "bad_key" and code == model.OK
        assert passed == (r["Result"] == "P"), (r["comment"], status, code, r["Result"])
        out.append({"comment": r["comment"], "digest": r["Digest"], "key": key.hex(), "msg": msg.hex(),
                    "sig": sig.hex(), "result": r["Result"], "key_status": status,
                    "code": code if status == "ok" else None})
    assert len(out) == 54, len(out)
    for d in model.HASH:
        rows = [x for x in out if x["digest"] == d]
        assert len(rows) == 18 and all(x["key_status"] == "ok" for x in rows), d
        assert {model.ring_key(bytes.fromhex(x["key"]))[0].bit_length() for x in rows} == {2048}, d
    return out


def padding_rows(src):
    out = []
    for r in rows_of(src):
        msg, salt, em, bits = unhex(r["Msg"]), unhex(r["Salt"]), unhex(r["EM"]), int(r["Len"])
        code = model.em_code(r["Digest"], msg, em, bits)
        assert (code == model.OK) == (r["Result"] == "P"), (r["comment"], r["Digest"], bits, r["Result"], code)
        if code == model.OK:      # the file's passing rows are also what ring's encoder makes from the salt
            assert model.encode(r["Digest"], msg, salt, bits) == em, (r["Digest"], bits)
        out.append({"comment": r["comment"], "digest": r["Digest"], "msg": msg.hex(), "salt": salt.hex(),
                    "em": em.hex(), "bits": bits, "result": r["Result"], "code": code})
    assert {x["bits"] for x in out} == {256, 512, 2048, 2049, 2055, 2056, 2057, 4095, 4096, 4097, 8191, 8192}
    assert sum(x["result"] == "P" for x in out) == 60 and len(out) == 105, len(out)
    return out


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_DIR
    ver = verify_rows(os.path.join(src, "tests", "rsa_pss_verify_tests.txt"))
    pad = padding_rows(os.path.join(src, "src", "rsa", "rsa_pss_padding_tests.txt"))
    dst = model.dump_fixture("ring_rsa_pss.json.gz",
                             {"source": "ring tests/rsa_pss_verify_tests.txt and src/rsa/rsa_pss_padding_tests.txt",
                              "algorithm": "RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512", "verify": ver, "padding": pad})
    print(dst, len(ver), "verify rows", len(pad), "padding rows")


if __name__ == "__main__":
    main()
