"""RSASSA-PKCS1-v1_5 with SHA-256, hashed on the GPU (include/cess_rsa.h hashed
mode; the signature check of verify_miner_cert, enclave-verify/src/lib.rs:165-169:
webpki::RSA_PKCS1_2048_8192_SHA256 = ring's key policy).

CPU: a plain-Python model (hashlib, pow, strict DER) reproduces ring's own 52
SHA-256 vectors (tests/golden/ring_rsa_pkcs1_sha256.json, from the reference's
utils/ring/tests/rsa_pkcs1_verify_tests.txt) and the fixture's expectation
fields; the library's key policy agrees with them; the digest kernel's padding
and word assembly (cess_amd/csrc/rsa_digest.hpp) built for the host equal
hashlib at every length 0..200 and start offset 0..3, and the padding function
alone is right where the bit length crosses 32 bits.

GPU: digests against hashlib; ring's rows through the host-buffer,
device-resident and single-record entries; generated records at the SHA block
and padding edges against the model and against the raw path over T computed
in Python; the key-uniform path; a two-device context; the profiling stage."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import rsa_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = bytes.fromhex("3031300d060960864801650304020105000420")
OK, SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH, KEY = range(6)


# --- the plain-Python model ---------------------------------------------------
class BadKey(ValueError):
    pass


def _tlv(b, pos):
    if pos + 2 > len(b):
        raise BadKey
    tag, ln = b[pos], b[pos + 1]
    pos += 2
    if ln & 0x80:
        nb = ln & 0x7F
        if nb == 0 or nb > 4 or pos + nb > len(b) or b[pos] == 0:
            raise BadKey
        ln = int.from_bytes(b[pos:pos + nb], "big")
        if ln < 0x80:
            raise BadKey
        pos += nb
    if pos + ln > len(b):
        raise BadKey
    return tag, b[pos:pos + ln], pos + ln


def _uint(tag, v):
    if tag != 0x02 or not v or v[0] & 0x80 or (len(v) > 1 and v[0] == 0 and not v[1] & 0x80):
        raise BadKey
    return int.from_bytes(v, "big")


def ring_key(der):
    """(n, e) of a PKCS#1 RSAPublicKey DER under ring's RSA_PKCS1_2048_8192_SHA256 key checks."""
    tag, body, end = _tlv(der, 0)
    if tag != 0x30 or end != len(der):
        raise BadKey
    t1, vn, p = _tlv(body, 0)
    t2, ve, p = _tlv(body, p)
    if p != len(body):
        raise BadKey
    n, e = _uint(t1, vn), _uint(t2, ve)
    if 8 * ((n.bit_length() + 7) // 8) < 2048 or n.bit_length() > 8192:
        raise BadKey
    if not n & 1 or not e & 1 or not 3 <= e <= (1 << 33) - 1:
        raise BadKey
    return n, e


def t_of(msg):
    return PREFIX + hashlib.sha256(msg).digest()


def model_code(n, e, msg, sig):
    """Hashed-mode code: k = the modulus length in bytes (RsaKeyDev.k_bytes)."""
    return o.verify_code(n, e, t_of(msg), sig)


def model_status(der):
    try:
        n, _ = ring_key(der)
    except BadKey:
        return "bad_key"
    return "ok" if n.bit_length() <= 4096 else "unsupported"


@pytest.fixture(scope="module")
def ring():
    with open(os.path.join(ROOT, "tests", "golden", "ring_rsa_pkcs1_sha256.json")) as f:
        rows = json.load(f)["rows"]
    for r in rows:
        for k in ("key", "msg", "sig"):
            r[k] = bytes.fromhex(r[k])
    return rows


def _status_value(bls, name):
    return {"ok": 0, "bad_key": bls.E_BAD_KEY, "unsupported": bls.RSA_E_UNSUPPORTED}[name]


# --- CPU ------------------------------------------------------------------------
def test_fixture_model(ring):
    assert len(ring) == 52
    assert sum(r["result"] == "P" for r in ring) == 12
    causes = {"mismatch": 0, "sig_len": 0, "range": 0, "bad_key": 0}
    for r in ring:
        st = model_status(r["key"])
        assert st == r["key_status"], r["comment"]
        if st == "bad_key":
            assert r["result"] == "F" and r["code"] is None
            causes["bad_key"] += 1
            continue
        n, e = ring_key(r["key"])
        code = model_code(n, e, r["msg"], r["sig"])
        assert (code == OK) == (r["result"] == "P"), r["comment"]
        assert r["code"] == (code if st == "ok" else None), r["comment"]
        causes["mismatch"] += code == MISMATCH
        causes["sig_len"] += code == SIG_LEN
        causes["range"] += code == SIG_RANGE
    assert causes == {"mismatch": 30, "sig_len": 5, "range": 1, "bad_key": 4}
    bits = {ring_key(r["key"])[0].bit_length() for r in ring if r["key_status"] != "bad_key"}
    assert {2048, 3072, 4096, 8192} <= bits
    assert {len(r["msg"]) for r in ring} == {0, 128}


def test_key_policy(ring):
    from cess_amd import bls
    seen = {}
    for r in ring:
        seen.setdefault(r["key"], r)
    assert len(seen) == 22
    parsed = rejected = 0
    for der, r in seen.items():
        if r["key_status"] == "bad_key":
            with pytest.raises(bls.BlsInfraError) as ei:
                bls.rsa_parse_key(der, bls.RSA_KEY_PKCS1, policy=bls.RSA_POLICY_RING_2048_8192)
            assert ei.value.status == bls.E_BAD_KEY, r["comment"]
            rejected += 1
        else:       # "ok" and "unsupported" (the 8192-bit key): the policy accepts the key
            mod, e = bls.rsa_parse_key(der, bls.RSA_KEY_PKCS1, policy=bls.RSA_POLICY_RING_2048_8192)
            assert (int.from_bytes(mod, "big"), e) == ring_key(der), r["comment"]
            parsed += 1
    assert rejected == 4 and parsed == 18          # 2040 bits, 8193 bits, e = 1, e = 2^33 + 1
    assert any(len(bls.rsa_parse_key(d, bls.RSA_KEY_PKCS1, policy=1)[0]) == 1024 for d, r in seen.items()
               if r["key_status"] == "unsupported")
    # ring rounds the modulus length up to bytes for the 2048-bit floor; an even modulus or exponent is rejected
    n2041, n2047 = (1 << 2040) | 1, (1 << 2046) | 1
    for n, e, good in ((n2041, 65537, True), (n2047, 3, True), ((1 << 2039) | 1, 65537, False),
                       ((1 << 2047) | 2, 65537, False), ((1 << 2047) | 1, 65536, False), ((1 << 2047) | 1, 1, False),
                       ((1 << 2047) | 1, (1 << 33) - 1, True), ((1 << 2047) | 1, (1 << 33) + 1, False)):
        der = o.encode_pkcs1(n, e)
        assert (model_status(der) == "ok") == good
        if good:
            assert bls.rsa_parse_key(der, bls.RSA_KEY_PKCS1, policy=1) == (n.to_bytes((n.bit_length() + 7) // 8, "big"), e)
            assert bls.rsa_parse_key(o.encode_spki(n, e), bls.RSA_KEY_SPKI, policy=1)[1] == e
        else:
            with pytest.raises(bls.BlsInfraError) as ei:
                bls.rsa_parse_key(der, bls.RSA_KEY_PKCS1, policy=1)
            assert ei.value.status == bls.E_BAD_KEY
    # policy 0 is cess_rsa_parse_key
    with open(os.path.join(ROOT, "tests", "golden", "rsa_vectors.json")) as f:
        rv = json.load(f)
    lib = bls.load_library()

    def old(der, fmt):
        out = (ctypes.c_uint8 * 512)()
        ln, e = ctypes.c_size_t(), ctypes.c_uint64()
        st = lib.cess_rsa_parse_key(ctypes.cast(ctypes.c_char_p(der), ctypes.POINTER(ctypes.c_uint8)), len(der), fmt,
                                    out, 512, ctypes.byref(ln), ctypes.byref(e))
        return (st, bytes(out)[: ln.value], e.value) if st == 0 else (st,)

    def new(der, fmt):
        try:
            return (0,) + bls.rsa_parse_key(der, fmt, policy=bls.RSA_POLICY_RSA_CRATE)
        except bls.BlsInfraError as ex:
            return (ex.status,)

    checked = 0
    for k in rv["keys"]:
        for name, fmt in (("spki", bls.RSA_KEY_SPKI), ("pkcs1", bls.RSA_KEY_PKCS1)):
            der = bytes.fromhex(k[name])
            assert new(der, fmt) == old(der, fmt) and old(der, fmt)[0] == 0
            checked += 1
    for b in rv["bad_keys"] + rv["unsupported_keys"]:
        der = bytes.fromhex(b["der"])
        assert new(der, bls.RSA_KEY_SPKI) == old(der, bls.RSA_KEY_SPKI), b["name"]
        checked += 1
    assert checked > 10


def _emu():
    src = os.path.join(ROOT, "tests", "hostemu", "rsa_digest_emu.cpp")
    lib = os.path.join(ROOT, "tests", "hostemu", "librsa_digest_emu.so")
    hdrs = [os.path.join(ROOT, "cess_amd", "csrc", "rsa_digest.hpp"), os.path.join(ROOT, "cess_amd", "csrc", "bls", "h2c.hpp"),
            os.path.join(ROOT, "tests", "hostemu", "rsa_digest_emu.hpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", src, "-o", lib])
    emu = ctypes.CDLL(lib)
    emu.emu_rsa_digest.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p]
    emu.emu_rsa_digest_pad_block.argtypes = [ctypes.c_uint64, ctypes.c_char_p]
    emu.emu_rsa_digest_pad_word_check.argtypes = [ctypes.c_uint64]
    emu.emu_rsa_digest_padded_len.argtypes = [ctypes.c_uint64]
    emu.emu_rsa_digest_padded_len.restype = ctypes.c_uint64
    return emu


def test_digest_header_on_host():
    """rsa_digest.hpp compiled for the host (no sanitizer, no preload): digests
    of every length 0..200 at start offsets 0..3 inside a larger buffer equal
    hashlib's and no fetched dword lies outside the buffer's dwords; the padding
    function alone gives the final block for lengths around 2^32 bits."""
    emu = _emu()
    rng = random.Random(0x5348)
    total = 64 + 208
    data = bytes(rng.randrange(256) for _ in range(total))
    buf = ctypes.create_string_buffer(data, total)           # 16-byte aligned
    assert ctypes.addressof(buf) % 4 == 0
    out = ctypes.create_string_buffer(32)
    for base in (0, 61):                                     # the buffer's start and its middle
        for off in range(4):
            for ln in range(201):
                start = base + off
                assert emu.emu_rsa_digest(ctypes.addressof(buf), total, start, ln, out) == 0, (start, ln)
                assert out.raw == hashlib.sha256(data[start:start + ln]).digest(), (start, ln)
    # a message that ends at the buffer's last byte, buffer lengths of every residue mod 4
    for total2 in range(197, 205):
        b2 = ctypes.create_string_buffer(data[:total2], total2)
        for start in range(4):
            assert emu.emu_rsa_digest(ctypes.addressof(b2), total2, start, total2 - start, out) == 0
            assert out.raw == hashlib.sha256(data[start:total2]).digest()
    blk = ctypes.create_string_buffer(64)
    for ln in ((1 << 29) - 1, 1 << 29, (1 << 32) + 5, 0, 55, 56, 64, (1 << 61) - 1):
        padded = (ln + 9 + 63) // 64 * 64
        assert emu.emu_rsa_digest_padded_len(ln) == padded
        # the stream after the message (whose own bytes the padding function leaves zero)
        want = (bytes(64) + b"\x80" + bytes(padded - ln - 9) + (8 * ln).to_bytes(8, "big"))[-64:]
        emu.emu_rsa_digest_pad_block(ln, blk)
        assert blk.raw == want, ln
        assert emu.emu_rsa_digest_pad_word_check(ln) == 0, ln        # the kernel's word form of the same function
    for ln in range(260):
        assert emu.emu_rsa_digest_pad_word_check(ln) == 0, ln


# --- GPU ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gen():
    """Generated keys (1024 and 2048 bits) and records at the SHA block and
    padding edges, with the model's codes; computed once."""
    rng = random.Random(0x52534132)
    keys = [o.gen_key(1024, 65537, rng), o.gen_key(2048, 65537, rng)]
    recs = []      # (key index, msg, sig)
    for ki, (n, e, d) in enumerate(keys):
        for ln in (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 129, 183, 1000):
            msg = bytes(rng.randrange(256) for _ in range(ln))
            sig = o.sign_raw(n, d, t_of(msg))
            recs.append((ki, msg, sig))
            if ln:
                recs.append((ki, bytes([msg[0] ^ 1]) + msg[1:], sig))
                recs.append((ki, msg[:-1] + bytes([msg[-1] ^ 0x80]), sig))
            recs.append((ki, msg + b"\x00", sig))
            recs.append((ki, msg, sig[:-1] + bytes([sig[-1] ^ 1])))
        short = bytes(rng.randrange(256) for _ in range(40))
        recs.append((ki, short, o.sign_raw(n, d, short)))       # signed over the message itself, not T
        recs.append((ki, short, o.sign_raw(n, d, t_of(short))))
    recs.append((len(keys), b"no such key", bytes(256)))           # key_idx >= k
    codes = [KEY if ki >= len(keys) else model_code(keys[ki][0], keys[ki][1], m, s) for ki, m, s in recs]
    return {"keys": keys, "recs": recs, "codes": codes}


def _device_codes(c, fn, recs):
    S = b"".join(r[2] for r in recs)
    M = b"\xa5" + b"".join(r[1] for r in recs)          # messages start at an odd device address
    so = np.cumsum([0] + [len(r[2]) for r in recs]).astype(np.uint64)
    mo = np.cumsum([0] + [len(r[1]) for r in recs]).astype(np.uint64)
    d = [c.to_device(np.array([r[0] for r in recs], dtype=np.uint32)), c.to_device(S), c.to_device(so),
         c.to_device(M), c.to_device(mo)]
    dc = c.device_alloc(len(recs))
    try:
        fn(len(recs), d[0], d[1], d[2], d[3] + 1, d[4], dc)
        c.synchronize()
        return c.from_device(dc, len(recs))
    finally:
        for p in d + [dc]:
            c.device_free(p)


@pytest.mark.gpu
def test_gpu_sha256_batch(ctx):
    rng = random.Random(4)
    msgs = [bytes(rng.randrange(256) for _ in range(ln)) for ln in range(300)]
    assert ctx.sha256_batch(msgs) == [hashlib.sha256(m).digest() for m in msgs]
    # one long message among 63 short ones of the same wave
    wave = [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 200))) for _ in range(64)]
    wave[17] = bytes(rng.randrange(256) for _ in range(70001))
    assert ctx.sha256_batch(wave) == [hashlib.sha256(m).digest() for m in wave]
    assert ctx.sha256_batch([]) == []
    assert ctx.sha256_batch([b""]) == [hashlib.sha256(b"").digest()]
    assert ctx.sha256_batch([b""] * 65) == [hashlib.sha256(b"").digest()] * 65


@pytest.mark.gpu
def test_gpu_ring_rows(ctx, ring):
    from cess_amd import bls
    ders = list(dict.fromkeys(r["key"] for r in ring))
    status = {d: next(r["key_status"] for r in ring if r["key"] == d) for d in ders}
    st = ctx.rsa_keys_load(ders, bls.RSA_KEY_PKCS1, policy=bls.RSA_POLICY_RING_2048_8192)
    assert st == [_status_value(bls, status[d]) for d in ders]
    recs = [(ders.index(r["key"]), r["msg"], r["sig"]) for r in ring]
    want = bytes(KEY if r["code"] is None else r["code"] for r in ring)      # a key that did not load: KEY
    assert ctx.rsa_verify_sha256_batch([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]) == want
    assert _device_codes(ctx, ctx.rsa_verify_sha256_batch_device, recs) == want
    classes = set()
    for r in ring:
        if r["code"] is None:
            with pytest.raises(bls.BlsInfraError) as ei:
                ctx.verify_rsa_sha256(r["key"], r["msg"], r["sig"], bls.RSA_KEY_PKCS1)
            assert ei.value.status == _status_value(bls, r["key_status"]), r["comment"]
        else:
            assert ctx.verify_rsa_sha256(r["key"], r["msg"], r["sig"], bls.RSA_KEY_PKCS1) == (r["code"] == 0), r["comment"]
            if r["code"] == 0:
                n, e = ring_key(r["key"])
                classes.add((n.bit_length(), e))
    assert {b for b, _ in classes} >= {2048, 3072, 4096}          # the 2048-bit and the loop-form classes
    assert max(e for _, e in classes) == (1 << 33) - 1 and min(e for _, e in classes) == 3


@pytest.mark.gpu
def test_gpu_generated_records(ctx, gen):
    from cess_amd import bls
    keys, recs, want = gen["keys"], gen["recs"], gen["codes"]
    assert {OK, MISMATCH, KEY} <= set(want)
    ders = [o.encode_spki(n, e) for n, e, _ in keys]
    assert ctx.rsa_keys_load(ders) == [0, 0]                       # policy 0: the 1024-bit key loads
    idx, msgs, sigs = [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]
    got = ctx.rsa_verify_sha256_batch(idx, msgs, sigs)
    assert list(got) == want
    assert list(_device_codes(ctx, ctx.rsa_verify_sha256_batch_device, recs)) == want
    # the unchanged raw path over T computed here gives the same codes
    assert ctx.rsa_verify_batch(idx, [t_of(m) for m in msgs], sigs) == got
    # under ring's policy the 1024-bit key does not load: its records are KEY, the others unchanged
    assert ctx.rsa_keys_load(ders, policy=bls.RSA_POLICY_RING_2048_8192) == [bls.E_BAD_KEY, 0]
    assert list(ctx.rsa_verify_sha256_batch(idx, msgs, sigs)) == [KEY if k == 0 else c for k, c in zip(idx, want)]


@pytest.mark.gpu
def test_gpu_key_uniform_path(ctx, gen):
    """One 2048-bit key, 512 records (>= 256 per key: the key-sorted lists and
    k_rsa_verify_2048u), message lengths cycling 0..127, bad records at the
    ends of the first wave, the start of the second and the end of the batch."""
    from cess_amd import bls
    n, e, d = gen["keys"][1]
    rng = random.Random(77)
    base = []
    for ln in range(128):
        m = bytes(rng.randrange(256) for _ in range(ln))
        base.append((m, o.sign_raw(n, d, t_of(m))))
    recs = [base[i % 128] for i in range(512)]
    bad = (0, 63, 64, 511)
    recs[0] = (recs[0][0] + b"x", recs[0][1])                                # another message
    recs[63] = (recs[63][0], recs[63][1][:-1] + bytes([recs[63][1][-1] ^ 1]))   # signature bit
    recs[64] = (recs[64][0][:-1] + bytes([recs[64][0][-1] ^ 4]), recs[64][1])   # message bit
    recs[511] = (recs[511][0], recs[511][1][1:])                             # SIG_LEN
    want = [model_code(n, e, m, s) for m, s in recs]
    assert [i for i, c in enumerate(want) if c] == list(bad) and want[511] == SIG_LEN
    assert ctx.rsa_keys_load([o.encode_spki(n, e)], policy=bls.RSA_POLICY_RING_2048_8192) == [0]
    codes, words = ctx.rsa_verify_sha256_batch([0] * 512, [r[0] for r in recs], [r[1] for r in recs], with_bitmap=True)
    assert list(codes) == want
    full = (1 << 64) - 1
    assert words == [full & ~1 & ~(1 << 63), full & ~1] + [full] * 5 + [full & ~(1 << 63)]


@pytest.mark.gpu
def test_gpu_multi_device_context(gen):
    from cess_amd import bls
    keys, recs, want = gen["keys"], gen["recs"], gen["codes"]
    m = bls.Context(max_batch=1024, devices=[0, 0])
    try:
        assert m.rsa_keys_load([o.encode_spki(n, e) for n, e, _ in keys]) == [0, 0]
        got = m.rsa_verify_sha256_batch([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
        assert want[-2] == OK and want[-3] == MISMATCH
        assert m.verify_rsa_sha256(o.encode_spki(*keys[1][:2]), recs[-2][1], recs[-2][2]) is True
        assert m.verify_rsa_sha256(o.encode_spki(*keys[1][:2]), recs[-3][1], recs[-3][2]) is False
    finally:
        m.close()
    assert len(recs) > 128                    # both shards hold records
    assert list(got) == want


@pytest.mark.gpu
def test_gpu_digest_stage(gen):
    from cess_amd import bls
    keys, recs = gen["keys"], gen["recs"][:40]
    c = bls.Context(max_batch=4096, profile=True)
    try:
        c.rsa_keys_load([o.encode_spki(n, e) for n, e, _ in keys])
        c.stage_stats(reset=True)
        idx, msgs, sigs = [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]
        c.rsa_verify_sha256_batch(idx, msgs, sigs)
        st = c.stage_stats(reset=True)
        assert st["k_rsa_digest"][1] == 1 and st["k_rsa_digest"][0] > 0 and st["k_rsa_verify"][1] == 1
        c.rsa_verify_batch(idx, [t_of(m) for m in msgs], sigs)
        st = c.stage_stats(reset=True)
        assert st["k_rsa_digest"] == (0.0, 0) and st["k_rsa_verify"][1] == 1
        assert "k_rsa_digest" not in {k for k, v in st.items() if v[1] > 0}      # the filtered view omits it
        names = list(st)
        assert names.index("k_rsa_digest") == len(names) - 1 and names[:3] == ["k_decode_sig", "k_decode_pk", "k_hash"]
    finally:
        c.close()
