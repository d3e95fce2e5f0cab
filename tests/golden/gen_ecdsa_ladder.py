#!/usr/bin/env python3
"""tests/golden/ecdsa_ladder.json: valid ECDSA P-256 records whose ladder
(double_mul in cess_amd/csrc/p256.hpp) meets a doubling or a cancel at a chosen
addition of a chosen round, each with the same record under one more message
byte.  Pure Python and deterministic; tests/ecdsa_ladder_model.py states the
construction (grind) and finds the messages.  Rounds 0 and 1, both additions and
both kinds for every algorithm, and round 2 at the Q addition for the FIXED
one (four million hashes each expected, 1.09 and 0.67 million under these seeds;
the whole run takes two to three minutes).

Like ecdsa_edges.json these rows are judged by tests/ecdsa_model.py alone.

A row: name, alg, key, msg, sig, code, the (round, addend, kind) it takes, and
d, the key's discrete logarithm, from which a test can follow the ladder on
scalars (ecdsa_ladder_model.trace).
"""
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ecdsa_ladder_model as lm  # noqa: E402
import ecdsa_model as m  # noqa: E402

targets = [(alg, k, a, kind) for alg in range(3) for k in (0, 1) for a in lm.ADDENDS for kind in lm.KINDS]
targets += [(m.ALG_P256_SHA256_FIXED, 2, "Q", kind) for kind in lm.KINDS]
rows = []
for alg, k, addend, kind in targets:
    t0 = time.time()
    rng = random.Random("ecdsa ladder %d %d %s %s" % (alg, k, addend, kind))
    d, msg, r, s, tries = lm.grind(alg, k, addend, kind, rng)
    key, sig = m.key_bytes(m.mul(d, m.G)), m.encode_sig(alg, r, s)
    e = m.digest_scalar(alg, msg)
    events, sigma = lm.trace(e * lm.inv(s) % m.N, r * lm.inv(s) % m.N, d)
    assert (k, addend, kind) in events and sigma
    name = "ladder: round %d, %s addition, %s" % (k, addend, kind)
    for nm, mg, want in ((name, msg, m.OK), (name + ", one more message byte", msg + b"\x00", m.MISMATCH)):
        assert m.verify_code(alg, key, mg, sig) == want, nm
        rows.append({"name": nm, "alg": alg, "key": key.hex(), "msg": mg.hex(), "sig": sig.hex(), "code": want,
                     "round": k, "addend": addend, "kind": kind, "d": "%064x" % d})
    print("%-40s alg %d: %8d tries, %6.1f s" % (name, alg, tries, time.time() - t0), flush=True)

with open(os.path.join(HERE, "ecdsa_ladder.json"), "w") as f:
    f.write('{"judge": "tests/ecdsa_model.py alone (ring\'s P-256 arithmetic is assembly and was not built)",\n"rows": [\n')
    f.write(",\n".join(json.dumps(r, sort_keys=True) for r in rows))
    f.write("\n]}\n")
print(len(rows), "rows")
