"""The sweep of the RSASSA-PSS EM check (cess_amd/csrc/rsa_pss.hpp) over every byte phase: TEST INFRASTRUCTURE
ONLY, pure Python and seeded.  tests/test_rsa_pss.py sends its records through the header's host build,
tests/test_gpu_rsa_pss_sweep.py through k_rsa_pss; every expected code is the model's (tests/rsa_pss_model.py).

What the check computes per key, and the sizes that drive each of them (h the digest's length):
  em_len & 3, em_bits & 7   the byte phase of the MGF1 mask against the words of m, and the top mask: all 32
                            pairs in each of three regions: the smallest sizes, 2041..2072 (the compile-time
                            class, on both sides of 64 words) and 4081..4112 (the top of the loop-form class)
  ps_len = em_len - 2h - 2  0..11: the separator in every byte of the first three mask words
  r = ((db_len - 1) % h) + 1   where the salt's mask starts in the last two MGF1 blocks: 1, 2, 3, 4, h - 1, h
                            (r == h: db_len is a whole number of blocks), from sizes of 3000 bits and more
  nblk = ceil(db_len / h)   the MGF1 trip count: 2 at the smallest sizes, 16 / 10 / 7 at 4112 bits
  em_len < 2h + 2           the eight sizes below the smallest valid one: PSSMetrics::new fails, MISMATCH
sizes() is asserted against these conditions on import; records() and sweep() assert, from the model alone, what
keeps the sweep from hiding a failure: every valid encoding is OK, every record with a flipped bit is MISMATCH,
exactly three records per valid size are OK, every tag occurs for every digest.
"""
import functools
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import rsa_pss_model as model  # noqa: E402
from gen_rsa_pss_edges import EM_CASES, LEAD, craft  # noqa: E402

DIGESTS = ("SHA256", "SHA384", "SHA512")
SEED = 0x73776565
R_MID_FROM = 3000            # the sizes chosen for r start here: the loop-form class, between the two regions
# tags: the three valid encodings ("valid" is craft's), one flipped bit at byte position P ("flip:P"), craft's
# failing cases, the records of wrong length, and the records of a size that has no valid encoding
VALID_TAGS = ("valid_first", "valid", "valid_empty_msg")
LEN_TAGS = ("short", "long", "empty")
SMALL_TAGS = ("too_small_random", "too_small_zero", "too_small_tail")
TAGS = set(VALID_TAGS) | {"flip"} | set(EM_CASES) | {LEAD} | set(LEN_TAGS) | set(SMALL_TAGS)


def metrics(digest, bits):
    """what rsa_pss::check derives from mod_bits (None for db_len, ps_len, nblk, r where the size is too small)"""
    h = model.HASH[digest]().digest_size
    em_bits = bits - 1
    em_len = (em_bits + 7) // 8
    m = {"h": h, "k": (bits + 7) // 8, "em_bits": em_bits, "em_len": em_len, "top": 0xff >> (8 * em_len - em_bits),
         "valid": em_len >= 2 * h + 2}
    if m["valid"]:
        db_len = em_len - h - 1
        nblk = (db_len + h - 1) // h
        m.update(db_len=db_len, ps_len=db_len - h - 1, nblk=nblk, r=db_len - h - (nblk - 2) * h)
    return m


def smallest(digest):
    """the smallest modulus length with a valid encoding: em_len = 2h + 2"""
    h = model.HASH[digest]().digest_size
    return 8 * (2 * h + 1) + 2


def sizes(digest):
    h = model.HASH[digest]().digest_size
    small = smallest(digest)
    out = set(range(small - 8, small + 96)) | set(range(2041, 2073)) | set(range(4081, 4113))
    for r in (1, 2, 3, 4, h - 1, h):         # the first em_len from R_MID_FROM bits with this r, with and without a leading byte
        em_len = next(e for e in range(R_MID_FROM // 8, R_MID_FROM // 8 + h + 1) if (e - h - 2) % h + 1 == r)
        out |= {8 * em_len, 8 * em_len + 1}
    return sorted(out)


def _check_sizes(digest):
    h = model.HASH[digest]().digest_size
    small = smallest(digest)
    s = sizes(digest)
    ms = {b: metrics(digest, b) for b in s}
    assert not metrics(digest, small - 1)["valid"] and ms[small]["valid"] and ms[small]["em_len"] == 2 * h + 2
    assert [b for b in s if not ms[b]["valid"]] == list(range(small - 8, small))
    for lo, hi in ((small, small + 32), (2041, 2073), (4081, 4113)):
        pairs = {(ms[b]["em_len"] & 3, ms[b]["em_bits"] & 7) for b in s if lo <= b < hi}
        assert len(pairs) == 32, (digest, lo, len(pairs))
    valid = [ms[b] for b in s if ms[b]["valid"]]
    assert {m["ps_len"] for m in valid} >= set(range(12))
    assert {m["top"] for m in valid if m["ps_len"] == 0} == {0xff >> i for i in range(8)}
    assert {m["r"] for m in valid} >= {1, 2, 3, 4, h - 1, h}
    assert {m["r"] for m in valid if m["em_len"] >= R_MID_FROM // 8 and m["em_len"] < 4081 // 8} == {1, 2, 3, 4, h - 1, h}
    nblk = {m["nblk"] for m in valid}
    assert len(nblk) >= 5 and 2 in nblk
    assert max(s) == model.GPU_MAX_BITS


for _d in DIGESTS:
    _check_sizes(_d)


def _bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def records(digest, sizes, rng):
    """[(bits, em, mhash, want, tag)] for every size: em the bytes of a message value m for a modulus of `bits`
    bits (any length: a record whose length is not k is a mismatch), mhash = H(msg), want = model.em_ok."""
    H = model.HASH[digest]
    h = H().digest_size
    out = []

    def add(bits, em, msg, tag):
        mh = H(msg).digest()
        out.append((bits, em, mh, model.em_ok(digest, mh, em, bits), tag))

    tail = model.encode(digest, b"tail", bytes(h), smallest(digest))
    for bits in sizes:
        m = metrics(digest, bits)
        k = m["k"]
        n0 = len(out)
        if not m["valid"]:
            add(bits, _bytes(rng, k - 1) + b"\xbc", _bytes(rng, 8), SMALL_TAGS[0])
            add(bits, bytes(k), b"", SMALL_TAGS[1])
            add(bits, tail[-k:], b"tail", SMALL_TAGS[2])      # the end of the smallest valid encoding
            add(bits, b"", b"", "empty")
            assert not any(r[3] for r in out[n0:]), bits
            continue
        # three valid encodings, each with a fresh message and salt
        msg = _bytes(rng, rng.randrange(1, 64))
        em = model.encode(digest, msg, _bytes(rng, h), bits)
        add(bits, em, msg, VALID_TAGS[0])
        add(bits, model.encode(digest, b"", _bytes(rng, h), bits), b"", VALID_TAGS[2])
        assert len(em) == k
        # one bit of every byte of the first
        for p in range(k):
            em2 = bytearray(em)
            em2[p] ^= 1 << rng.randrange(8)
            add(bits, bytes(em2), msg, "flip:%d" % p)
            assert out[-1][3] is False, (bits, p)
        # the edge fixture's crafted cases ("valid" is the third valid encoding).  Where ps_len == 0 there is no
        # padding byte: ps_first would set a bit of the separator and ps_last one of the salt, neither is the case
        for case in EM_CASES + ((LEAD,) if m["em_len"] < k else ()):
            if m["ps_len"] == 0 and case in ("ps_first", "ps_last"):
                continue
            cmsg = _bytes(rng, rng.randrange(1, 48))
            vmsg = bytes([cmsg[0] ^ 1]) + cmsg[1:] if case == "msg_changed" else cmsg
            for _ in range(64):      # a changed byte whose changed bits the top mask clears again is no failure: draw again
                cem = craft(digest, cmsg, bits, rng, case)
                if case == "valid" or not model.em_ok(digest, H(vmsg).digest(), cem, bits):
                    break
            assert len(cem) == k, (bits, case)
            add(bits, cem, vmsg, case)
        add(bits, em[1:], msg, LEN_TAGS[0])
        add(bits, b"\x00" + em, msg, LEN_TAGS[1])
        add(bits, b"", msg, LEN_TAGS[2])
        ok = [r[4] for r in out[n0:] if r[3]]
        assert sorted(ok) == sorted(VALID_TAGS), (digest, bits, ok)
    return out


def kind(tag):
    return tag.partition(":")[0]


def where(rec):
    """(bits, tag, byte position or None) of a record, for a failure report"""
    t, _, p = rec[4].partition(":")
    return rec[0], t, int(p) if p else None


@functools.lru_cache(maxsize=None)
def sweep(digest):
    """the records of every size of sizes(digest), generated once per process and shared by the tests"""
    recs = tuple(records(digest, sizes(digest), random.Random(SEED + model.DIGEST_ID[digest])))
    assert {kind(r[4]) for r in recs} == TAGS, TAGS ^ {kind(r[4]) for r in recs}
    return recs


@functools.lru_cache(maxsize=None)
def subset(digest, bits):
    """the same kind of records for a few sizes alone (seeded on its own: not a slice of sweep())"""
    return tuple(records(digest, list(bits), random.Random(SEED ^ 0x5a5a)))
