"""Generate tests/golden/ring_ed25519.json from the reference's ring vectors
(utils/ring/tests/ed25519_tests.txt, 514 known-answer rows of SEED, PUB,
MESSAGE, SIG): every row whose message is at most 320 bytes, plus the
1,023-byte row; 323 rows.  Fields: seed, pub, msg, sig (hex).  Only the rows'
data is kept, never the text file's comments.

The plain-Python model (tests/ed25519_model.py) must accept every one of the
514 rows and reject every one with sig[0] ^= 1 (the tamper of ring's
ed25519_tests.rs) as MISMATCH, or generation fails.

Runs only where the reference tree is present.
Usage: python tests/golden/gen_ring_ed25519.py [path/to/ed25519_tests.txt]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ed25519_model as model  # noqa: E402

DEFAULT_SRC = "/root/reference/utils/ring/tests/ed25519_tests.txt"
MAX_MSG, LONG_MSG = 320, 1023


def rows_of(path):
    cur = {}
    for line in open(path):
        line = line.strip()
        if line.startswith("#") or " = " not in line:
            continue
        k, v = line.split(" = ", 1)
        cur[k] = v.strip()
        if k == "SIG":
            yield cur
            cur = {}


def unhex(v):
    return b"" if v == '""' else bytes.fromhex(v)


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SRC
    out, total = [], 0
    for r in rows_of(src):
        seed, pub, msg, sig = (unhex(r[k]) for k in ("SEED", "PUB", "MESSAGE", "SIG"))
        total += 1
        assert model.verify_code(pub, msg, sig) == model.OK, total
        assert model.verify_code(pub, msg, bytes([sig[0] ^ 1]) + sig[1:]) == model.MISMATCH, total
        if len(msg) <= MAX_MSG or len(msg) == LONG_MSG:
            assert model.public_key(seed) == pub and model.sign(seed, msg) == sig, total
            out.append({"seed": seed.hex(), "pub": pub.hex(), "msg": msg.hex(), "sig": sig.hex()})
    assert total == 514 and len(out) == 323, (total, len(out))
    dst = os.path.join(HERE, "ring_ed25519.json")
    with open(dst, "w") as f:
        json.dump({"source": "ring tests/ed25519_tests.txt, rows with messages of at most 320 bytes and the "
                             "1,023-byte row", "algorithm": "ED25519", "rows": out}, f, indent=0)
        f.write("\n")
    print(dst, len(out), "of", total, "rows")


if __name__ == "__main__":
    main()
