"""Generate tests/golden/rsa_pss_edges.json.gz (gzipped JSON, model.load_fixture reads it): crafted RSASSA-PSS records at the edges of ring's rules
(tests/rsa_pss_model.py), for tests/test_rsa_pss.py and tests/test_gpu_rsa_pss.py.  Pure Python and seeded;
the keys come from oracle.rsa_oracle.gen_key, generated here once and stored, so no test generates one.

keys   name, bits, n, e (hex) of each key -- and d for the two 2048-bit keys, from which the GPU tests sign
       a few fresh records -- each chosen for a path of its own:
         a2048, b2048  the key-uniform and the unsorted lists of the 2048-bit class
         k2041         k = 256, em_len = 255: a leading zero byte in the compile-time class
         k2049         k = 257, em_len = 256: a leading zero byte, one byte more than 64 words
         k2056         em_len = 257: db_len is a whole number of MGF1 blocks for SHA-256 and SHA-512
         k2312         the same for SHA-384 (em_len = 289), loop-form class
         k3072, k4095, k4096   the loop-form class
         k3073         k = 385, em_len = 384: a leading zero byte through the loop-form kernel (a 2049-bit key
                       is still in the compile-time class, which holds keys of up to 2070 bits)
         k4104         k = 513: the largest limb count of the loop-form class (it holds k <= 514), 129 words of m
table  the RSAPublicKey DER of every table entry in table order: the keys above, then keys that ring's
       policy rejects (2040 bits, an even e, e = 1) and a 4120-bit key that the GPU does not verify (k = 515), with
       the model's status of each
rows   digest, key (table index, or one past the table), case, msg, sig (hex) and the model's code
Signatures are EM^d mod n for a crafted EM.  Where a crafted EM is not below n the generator draws again;
it never drops a case, and it asserts that every listed case is present for every digest.
Usage: python tests/golden/gen_rsa_pss_edges.py
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import oracle.rsa_oracle as o  # noqa: E402
import rsa_pss_model as model  # noqa: E402

KEY_BITS = [("a2048", 2048), ("b2048", 2048), ("k2041", 2041), ("k2049", 2049), ("k2056", 2056), ("k2312", 2312),
            ("k3072", 3072), ("k4095", 4095), ("k4096", 4096), ("k4104", 4104), ("k3073", 3073)]
OTHER = {"SHA256": "SHA512", "SHA384": "SHA256", "SHA512": "SHA384"}
MSG_LENS = (0, 55, 56, 64, 111, 112, 128, 1000)
PKCS1_PREFIX = {"SHA256": "3031300d060960864801650304020105000420", "SHA384": "3041300d060960864801650304020205000430",
                "SHA512": "3051300d060960864801650304020305000440"}
# every case of the issue's list; the cases of CORE go to every key, all of them to a2048
EM_CASES = ("valid", "trailer_bb", "above_em_bits", "ps_first", "ps_last", "sep_00", "sep_02", "salt_changed",
            "hprime_changed", "msg_changed", "salt_len_0", "salt_len_20", "salt_len_h_minus_1", "mgf1_other_hash",
            "pkcs1_v15")
CORE = ("valid", "above_em_bits", "ps_first", "sep_02", "salt_changed", "hprime_changed")
LEAD = "leading_byte"                       # only where em_len = k - 1 (k2041, k2049)
RANGE_CASES = ("s_zero", "s_n_minus_1", "s_n", "sig_short", "sig_long")
KEY_CASES = ("key_out_of_range", "key_2040_bits", "key_even_e", "key_e_1", "key_4120_bits")
PRECEDENCE = ("key_over_sig_len", "key_over_sig_range", "sig_len_over_sig_range", "sig_len_over_mismatch",
              "sig_range_over_mismatch")


def craft(digest, msg, bits, rng, case):
    """The k bytes of a crafted EM for `case`."""
    H = model.HASH[digest]
    h = H().digest_size
    salt_len = {"salt_len_0": 0, "salt_len_20": 20, "salt_len_h_minus_1": h - 1}.get(case, h)
    salt = bytes(rng.randrange(256) for _ in range(salt_len))
    if case == "mgf1_other_hash":
        return model.encode(digest, msg, salt, bits, mgf_digest=OTHER[digest])
    if case == "pkcs1_v15":
        k = (bits + 7) // 8
        t = bytes.fromhex(PKCS1_PREFIX[digest]) + H(msg).digest()
        return b"\x00\x01" + b"\xff" * (k - len(t) - 3) + b"\x00" + t
    em_bits = bits - 1
    em_len, k = (em_bits + 7) // 8, (bits + 7) // 8
    mask = 0xff >> (8 * em_len - em_bits)
    hp = H(bytes(8) + H(msg).digest() + salt).digest()
    db = bytearray(bytes(em_len - salt_len - h - 2) + b"\x01" + salt)
    ps_len = len(db) - salt_len - 1
    if case == "ps_first":
        db[0] |= 1 << rng.randrange(mask.bit_length())       # a bit that the top mask keeps
    elif case == "ps_last":
        db[ps_len - 1] = 1 + rng.randrange(255)
    elif case == "sep_00":
        db[ps_len] = 0
    elif case == "sep_02":
        db[ps_len] = 2
    elif case == "salt_changed":
        db[ps_len + 1 + rng.randrange(h)] ^= 1 << rng.randrange(8)
    masked = bytearray(a ^ b for a, b in zip(db, model.mgf1(H, hp, len(db))))
    masked[0] &= mask
    lead = bytes(k - em_len)
    if case == "above_em_bits":
        if mask == 0xff:
            lead = b"\x01"                                  # the bit above em_bits is the leading byte's
        else:
            masked[0] |= mask + 1
    elif case == LEAD:
        lead = b"\x01"
    if case == "hprime_changed":
        i = rng.randrange(h)
        hp = hp[:i] + bytes([hp[i] ^ (1 << rng.randrange(8))]) + hp[i + 1:]
    return lead + bytes(masked) + hp + (b"\xbb" if case == "trailer_bb" else b"\xbc")


def main():
    rng = random.Random(0x505353)
    keys = []
    for name, bits in KEY_BITS:
        n, e, d = o.gen_key(bits, 65537, rng)
        keys.append({"name": name, "bits": bits, "n": n, "e": e, "d": d})
        print(name, bits, file=sys.stderr)
    table = [(o.encode_pkcs1(k["n"], k["e"]), "ok") for k in keys]
    a = keys[0]
    n2040 = o.gen_key(2040, 65537, rng)[0]
    n4120 = o.gen_key(4120, 65537, rng)[0]
    extra = {"key_2040_bits": o.encode_pkcs1(n2040, 65537), "key_even_e": o.encode_pkcs1(a["n"], 65536),
             "key_e_1": o.encode_pkcs1(a["n"], 1), "key_4120_bits": o.encode_pkcs1(n4120, 65537)}
    extra_idx = {}
    for case, der in extra.items():
        st, _ = model.key_status(der)
        assert st == ("unsupported" if case == "key_4120_bits" else "bad_key"), (case, st)
        extra_idx[case] = len(table)
        table.append((der, st))
    for der, st in table[:len(keys)]:
        assert model.key_status(der)[0] == st

    rows = []

    def signed(key, digest, case, msg):
        while True:                                          # a crafted EM at or above n: draw the salt again
            em = craft(digest, msg, key["bits"], rng, case)
            v = int.from_bytes(em, "big")
            if v < key["n"]:
                k = (key["bits"] + 7) // 8
                return pow(v, key["d"], key["n"]).to_bytes(k, "big")

    def add(digest, ki, case, msg, sig):
        if ki < len(keys):
            k = keys[ki]
            code = model.verify_code(digest, k["n"], k["e"], msg, sig)
        else:
            code = model.KEY
        row = {"digest": digest, "key": ki, "case": case, "msg": msg.hex(), "sig": sig.hex(), "code": code}
        rows.append(row)
        return code

    for digest in model.HASH:
        for ki, key in enumerate(keys):
            k = (key["bits"] + 7) // 8
            lead = key["bits"] % 8 == 1
            cases = list(EM_CASES if ki == 0 else CORE) + ([LEAD] if lead else [])
            for case in cases:
                msg = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 48)))
                sig = signed(key, digest, case, msg)
                verify_msg = msg
                if case == "msg_changed":
                    verify_msg = bytes([msg[0] ^ 1]) + msg[1:]
                code = add(digest, ki, case, verify_msg, sig)
                assert (code == model.OK) == (case == "valid"), (digest, key["name"], case, code)
        key, k = keys[0], 256
        for ln in MSG_LENS:
            msg = bytes(rng.randrange(256) for _ in range(ln))
            assert add(digest, 0, "msg_len_%d" % ln, msg, signed(key, digest, "valid", msg)) == model.OK
        msg = b"range and length"
        good = signed(key, digest, "valid", msg)
        n_bytes = key["n"].to_bytes(k, "big")
        assert add(digest, 0, "s_zero", msg, bytes(k)) == model.MISMATCH
        assert add(digest, 0, "s_n_minus_1", msg, (key["n"] - 1).to_bytes(k, "big")) == model.MISMATCH
        assert add(digest, 0, "s_n", msg, n_bytes) == model.SIG_RANGE
        assert add(digest, 0, "sig_short", msg, good[1:]) == model.SIG_LEN
        assert add(digest, 0, "sig_long", msg, b"\x00" + good) == model.SIG_LEN
        assert add(digest, len(table), "key_out_of_range", msg, good) == model.KEY
        for case, idx in extra_idx.items():
            assert add(digest, idx, case, msg, good if case != "key_4120_bits" else bytes(515)) == model.KEY
        # one row per pair of the precedence KEY > SIG_LEN > SIG_RANGE > MISMATCH
        assert add(digest, extra_idx["key_e_1"], "key_over_sig_len", msg, good[1:]) == model.KEY
        assert add(digest, extra_idx["key_even_e"], "key_over_sig_range", msg, n_bytes) == model.KEY
        assert add(digest, 0, "sig_len_over_sig_range", msg, b"\xff" + n_bytes) == model.SIG_LEN
        assert add(digest, 0, "sig_len_over_mismatch", msg, good[:-1]) == model.SIG_LEN
        assert add(digest, 0, "sig_range_over_mismatch", msg, b"\xff" * k) == model.SIG_RANGE

    want = set(EM_CASES) | {LEAD} | set(RANGE_CASES) | set(KEY_CASES) | set(PRECEDENCE) | \
        {"msg_len_%d" % ln for ln in MSG_LENS}
    for digest in model.HASH:
        have = {r["case"] for r in rows if r["digest"] == digest}
        assert have == want, (digest, want ^ have)
        for ki in range(len(keys)):
            assert {r["case"] for r in rows if r["digest"] == digest and r["key"] == ki} >= set(CORE), (digest, ki)
    out = {"source": "tests/golden/gen_rsa_pss_edges.py (seeded); codes from tests/rsa_pss_model.py",
           "keys": [{"name": k["name"], "bits": k["bits"], "n": "%x" % k["n"], "e": "%x" % k["e"],
                     **({"d": "%x" % k["d"]} if k["bits"] == 2048 else {})} for k in keys],
           "table": [{"der": der.hex(), "status": st} for der, st in table], "rows": rows}
    dst = model.dump_fixture("rsa_pss_edges.json.gz", out)
    size = os.path.getsize(dst)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != "rsa_pss_edges.json.gz")
    assert size <= largest, (size, largest)
    print(dst, len(rows), "rows", size, "bytes")


if __name__ == "__main__":
    main()
