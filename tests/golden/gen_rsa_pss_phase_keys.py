"""Generate tests/golden/rsa_pss_phase_keys.json.gz (and its .codes.txt; the layout of rsa_pss_edges.json.gz,
model.load_fixture reads it): keys for the byte phases and size-class edges of the RSASSA-PSS check that no key
of the edge fixture has, for tests/test_rsa_pss.py and tests/test_gpu_rsa_pss_sweep.py.  Pure Python and seeded;
the keys come from oracle.rsa_oracle.gen_key, generated here once and stored, so no test generates one.

keys   name, bits, n, e (hex), and d for the three keys of the compile-time class, from which the tests sign:
         p2058  k = 258, em_len = 258: phase 2 (em_len & 3), 65 words of m, compile-time class
         p2065  k = 259, em_len = 258: phase 2 with a leading zero byte in word 64
         p2070  k = 259, em_len = 259: the largest key of the compile-time class (bits + 2 <= 28 x 74), phase 3
         p3090  k = 387, em_len = 387: phase 3 in the loop-form class
         p4112  k = 514, em_len = 514: the largest key the GPU verifies (8 k + 2 <= 28 x 147), phase 2
table  the RSAPublicKey DER of each key in that order, with the model's status ("ok")
rows   digest, key (table index), case, msg, sig (hex) and the model's code: the cases of CORE of
       gen_rsa_pss_edges.py for every key and digest, and leading_byte for p2065
The two neighbours of the class edges are asserted here and need no key: a 2071-bit modulus is in the loop-form
class, a 4113-bit one is `unsupported`.
Usage: python tests/golden/gen_rsa_pss_phase_keys.py
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracle.rsa_oracle as o  # noqa: E402
import rsa_probe_model as pm  # noqa: E402
import rsa_pss_model as model  # noqa: E402
from gen_rsa_pss_edges import CORE, LEAD, craft  # noqa: E402

NAME = "rsa_pss_phase_keys.json.gz"
KEY_BITS = [("p2058", 2058), ("p2065", 2065), ("p2070", 2070), ("p3090", 3090), ("p4112", 4112)]
L2048 = 74


def class_of(bits):
    return pm.size_class_limbs(bits, (bits + 7) // 8)


def main():
    # the class edges, from the restated size_class_limbs and the model's key policy
    assert class_of(2058) == class_of(2065) == class_of(2070) == L2048
    assert class_of(2071) > L2048 and class_of(3090) > L2048 and class_of(4112) > L2048
    assert class_of(4113) == 0
    assert model.key_status(o.encode_pkcs1((1 << 2070) | 1, 65537))[0] == "ok"
    assert model.key_status(o.encode_pkcs1((1 << 4111) | 1, 65537))[0] == "ok"
    assert model.key_status(o.encode_pkcs1((1 << 4112) | 1, 65537))[0] == "unsupported"
    for (_, bits), k, em_len in zip(KEY_BITS, (258, 259, 259, 387, 514), (258, 258, 259, 387, 514)):
        assert ((bits + 7) // 8, (bits + 6) // 8) == (k, em_len), bits

    rng = random.Random(0x706b)
    keys = []
    for name, bits in KEY_BITS:
        n, e, d = o.gen_key(bits, 65537, rng)
        keys.append({"name": name, "bits": bits, "n": n, "e": e, "d": d})
        print(name, bits, file=sys.stderr)
    table = [(o.encode_pkcs1(k["n"], k["e"]), "ok") for k in keys]
    for der, st in table:
        assert model.key_status(der)[0] == st

    rows = []
    for digest in model.HASH:
        for ki, key in enumerate(keys):
            k = (key["bits"] + 7) // 8
            for case in list(CORE) + ([LEAD] if key["bits"] % 8 == 1 else []):
                msg = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 48)))
                while True:                                  # a crafted EM at or above n: draw the salt again
                    v = int.from_bytes(craft(digest, msg, key["bits"], rng, case), "big")
                    if v < key["n"]:
                        break
                sig = pow(v, key["d"], key["n"]).to_bytes(k, "big")
                code = model.verify_code(digest, key["n"], key["e"], msg, sig)
                assert (code == model.OK) == (case == "valid") and code in (model.OK, model.MISMATCH), (digest, key["name"], case)
                rows.append({"digest": digest, "key": ki, "case": case, "msg": msg.hex(), "sig": sig.hex(), "code": code})
    for digest in model.HASH:
        for ki, key in enumerate(keys):
            have = {r["case"] for r in rows if r["digest"] == digest and r["key"] == ki}
            assert have == set(CORE) | ({LEAD} if key["name"] == "p2065" else set()), (digest, key["name"], have)
    out = {"source": "tests/golden/gen_rsa_pss_phase_keys.py (seeded); codes from tests/rsa_pss_model.py",
           "keys": [{"name": k["name"], "bits": k["bits"], "n": "%x" % k["n"], "e": "%x" % k["e"],
                     **({"d": "%x" % k["d"]} if class_of(k["bits"]) == L2048 else {})} for k in keys],
           "table": [{"der": der.hex(), "status": st} for der, st in table], "rows": rows}
    dst = model.dump_fixture(NAME, out)
    size = os.path.getsize(dst)
    assert size < os.path.getsize(os.path.join(HERE, "rsa_pss_edges.json.gz")), size
    print(dst, len(rows), "rows", size, "bytes")


if __name__ == "__main__":
    main()
