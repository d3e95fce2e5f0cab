"""RSASSA-PKCS1-v1_5 with SHA-384 and SHA-512, hashed on the GPU (include/cess_rsa.h:
cess_rsa_verify_digest_batch*, cess_rsa_verify_alg, cess_sha2_batch, key policy 2):
with SHA-256 the four webpki algorithms that verify_miner_cert admits
(enclave-verify/src/lib.rs:87-93).

CPU: a plain-Python model (hashlib, pow, strict DER) reproduces ring's own 75
SHA-384 / SHA-512 vectors (tests/golden/ring_rsa_pkcs1_sha384_sha512.json, from the
reference's utils/ring/tests/rsa_pkcs1_verify_tests.txt) and the fixture's
expectation fields; the 3072-bit-floor key policy; the digest kernel's padding, word
assembly and compression (cess_amd/csrc/rsa_digest512.hpp) built for the host equal
hashlib at every length 0..300 and start offset 0..3; the kernel's code object has
no scratch.

GPU: digests against hashlib; ring's rows through the host-buffer, device-resident
and single-record entries; generated records at the SHA-512 block and padding edges
against the model and against the raw path over T computed in Python; MSG_LEN; the
key-uniform path; a two-device context; the profiling stage; SHA-256 through the new
entries equals the existing ones."""
import ctypes
import glob
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import rsa_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA256, SHA384, SHA512 = 0, 1, 2                                   # CESS_RSA_DIGEST_*
PREFIX = {SHA256: bytes.fromhex("3031300d060960864801650304020105000420"),
          SHA384: bytes.fromhex("3041300d060960864801650304020205000430"),
          SHA512: bytes.fromhex("3051300d060960864801650304020305000440")}
HASH = {SHA256: hashlib.sha256, SHA384: hashlib.sha384, SHA512: hashlib.sha512}
DIGEST_OF = {"SHA384": SHA384, "SHA512": SHA512}
OK, SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH, KEY = range(6)
LENGTHS = (0, 1, 110, 111, 112, 113, 119, 120, 127, 128, 129, 239, 240, 255, 256, 257, 1000)


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


def ring_key(der, floor=2048):
    """(n, e) of a PKCS#1 RSAPublicKey DER under ring's key checks with a floor of 2048 or 3072 bits."""
    tag, body, end = _tlv(der, 0)
    if tag != 0x30 or end != len(der):
        raise BadKey
    t1, vn, p = _tlv(body, 0)
    t2, ve, p = _tlv(body, p)
    if p != len(body):
        raise BadKey
    n, e = _uint(t1, vn), _uint(t2, ve)
    if 8 * ((n.bit_length() + 7) // 8) < floor or n.bit_length() > 8192:
        raise BadKey
    if not n & 1 or not e & 1 or not 3 <= e <= (1 << 33) - 1:
        raise BadKey
    return n, e


def t_of(digest, msg):
    return PREFIX[digest] + HASH[digest](msg).digest()


def model_code(digest, n, e, msg, sig):
    """Hashed-mode code: k = the modulus length in bytes (RsaKeyDev.k_bytes)."""
    return o.verify_code(n, e, t_of(digest, msg), sig)


def model_status(der, floor=2048):
    try:
        n, _ = ring_key(der, floor)
    except BadKey:
        return "bad_key"
    return "ok" if n.bit_length() <= 4096 else "unsupported"


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ring():
    rows = _load("ring_rsa_pkcs1_sha384_sha512.json")["rows"]
    for r in rows:
        for k in ("key", "msg", "sig"):
            r[k] = bytes.fromhex(r[k])
    return rows


@pytest.fixture(scope="module")
def ring_digests():
    return [(DIGEST_OF[r["hash"]], bytes.fromhex(r["input"]) * r["repeat"], bytes.fromhex(r["output"]))
            for r in _load("ring_digest_sha384_sha512.json")["rows"]]


# --- CPU ------------------------------------------------------------------------
def test_fixture_model(ring, ring_digests):
    assert len(ring) == 75
    want = {"SHA384": (38, 7, {MISMATCH: 30, SIG_RANGE: 1}, {2048, 3072}, {0, 128}),
            "SHA512": (37, 7, {MISMATCH: 29, SIG_LEN: 1}, {2048, 3072, 4096}, {127, 128})}
    for name, (rows_n, passes, causes, bits, lens) in want.items():
        rows = [r for r in ring if r["digest"] == name]
        assert len(rows) == rows_n and sum(r["result"] == "P" for r in rows) == passes
        got = {}
        for r in rows:
            assert model_status(r["key"]) == r["key_status"] == "ok", r["comment"]
            n, e = ring_key(r["key"])
            code = model_code(DIGEST_OF[name], n, e, r["msg"], r["sig"])
            assert (code == OK) == (r["result"] == "P"), r["comment"]
            assert r["code"] == code, r["comment"]
            if code:
                got[code] = got.get(code, 0) + 1
        assert got == causes
        assert {ring_key(r["key"])[0].bit_length() for r in rows} == bits
        assert {len(r["msg"]) for r in rows} == lens
    # ring's digest_tests.txt has two rows for each of the two digests (its SHA512_256 rows are another algorithm)
    assert sorted(d for d, _, _ in ring_digests) == [SHA384, SHA384, SHA512, SHA512]
    for d, data, out in ring_digests:
        assert HASH[d](data).digest() == out


def _parse_status(bls, der, fmt, policy):
    try:
        return (0,) + bls.rsa_parse_key(der, fmt, policy=policy)
    except bls.BlsInfraError as ex:
        return (ex.status,)


def test_key_policy_3072(ring):
    from cess_amd import bls
    assert bls.RSA_POLICY_RING_3072_8192 == 2
    P2 = bls.RSA_POLICY_RING_3072_8192
    # the floor is compared against the length rounded up to whole bytes: 3065 bits pass, 3064 do not
    for n, e, good in (((1 << 3064) | 1, 65537, True), ((1 << 3063) | 1, 65537, False), ((1 << 3071) | 1, 3, True),
                       ((1 << 3071) | 2, 65537, False), ((1 << 3071) | 1, 65536, False), ((1 << 3071) | 1, 1, False),
                       ((1 << 3071) | 1, (1 << 33) - 1, True), ((1 << 3071) | 1, (1 << 33) + 1, False),
                       ((1 << 8191) | 1, 65537, True), ((1 << 8192) | 1, 65537, False)):
        der = o.encode_pkcs1(n, e)
        assert (model_status(der, 3072) != "bad_key") == good
        if good:
            assert _parse_status(bls, der, bls.RSA_KEY_PKCS1, P2) == (0, n.to_bytes((n.bit_length() + 7) // 8, "big"), e)
            assert _parse_status(bls, o.encode_spki(n, e), bls.RSA_KEY_SPKI, P2)[0] == 0
        else:
            assert _parse_status(bls, der, bls.RSA_KEY_PKCS1, P2) == (bls.E_BAD_KEY,)
            assert _parse_status(bls, o.encode_spki(n, e), bls.RSA_KEY_SPKI, P2) == (bls.E_BAD_KEY,)
    # the fixture's keys: 3072 and 4096 bits pass, 2048 bits do not
    seen = {2048: 0, 3072: 0, 4096: 0}
    for der in dict.fromkeys(r["key"] for r in ring):
        n, e = ring_key(der)
        seen[n.bit_length()] += 1
        if n.bit_length() >= 3072:
            assert _parse_status(bls, der, bls.RSA_KEY_PKCS1, P2) == (0, n.to_bytes((n.bit_length() + 7) // 8, "big"), e)
        else:
            assert _parse_status(bls, der, bls.RSA_KEY_PKCS1, P2) == (bls.E_BAD_KEY,)
        assert _parse_status(bls, der, bls.RSA_KEY_PKCS1, 1)[0] == 0
    assert all(seen.values())
    with pytest.raises(bls.BlsInfraError) as ei:
        bls.rsa_parse_key(o.encode_pkcs1((1 << 3071) | 1, 65537), bls.RSA_KEY_PKCS1, policy=3)
    assert ei.value.status == bls.E_INVALID_ARG


def test_key_policies_0_and_1_unchanged():
    """Policy 0 is cess_rsa_parse_key, policy 1 the SHA-256 fixture's recorded status, on every key of the
    two older fixtures."""
    from cess_amd import bls
    lib = bls.load_library()

    def old(der, fmt):
        out = (ctypes.c_uint8 * 512)()
        ln, e = ctypes.c_size_t(), ctypes.c_uint64()
        st = lib.cess_rsa_parse_key(ctypes.cast(ctypes.c_char_p(der), ctypes.POINTER(ctypes.c_uint8)), len(der), fmt,
                                    out, 512, ctypes.byref(ln), ctypes.byref(e))
        return (st, bytes(out)[: ln.value], e.value) if st == 0 else (st,)

    rv = _load("rsa_vectors.json")
    ders = [(bytes.fromhex(k[name]), fmt) for k in rv["keys"]
            for name, fmt in (("spki", bls.RSA_KEY_SPKI), ("pkcs1", bls.RSA_KEY_PKCS1))]
    ders += [(bytes.fromhex(b["der"]), bls.RSA_KEY_SPKI) for b in rv["bad_keys"] + rv["unsupported_keys"]]
    rows256 = _load("ring_rsa_pkcs1_sha256.json")["rows"]
    ring256 = {bytes.fromhex(r["key"]): r["key_status"] for r in rows256}
    ders += [(d, bls.RSA_KEY_PKCS1) for d in ring256]
    assert len(ders) > 30
    for der, fmt in ders:
        assert _parse_status(bls, der, fmt, 0) == old(der, fmt)
    for der, status in ring256.items():
        got = _parse_status(bls, der, bls.RSA_KEY_PKCS1, 1)
        assert (got[0] == bls.E_BAD_KEY) == (status == "bad_key")
        if status != "bad_key":
            n, e = ring_key(der)
            assert got[1:] == (n.to_bytes((n.bit_length() + 7) // 8, "big"), e)
        # the 3072-bit floor differs from the 2048-bit one only between the floors
        assert (_parse_status(bls, der, bls.RSA_KEY_PKCS1, 2)[0] == 0) == (model_status(der, 3072) != "bad_key")


def _emu():
    src = os.path.join(ROOT, "tests", "hostemu", "rsa_digest512_emu.cpp")
    lib = os.path.join(ROOT, "tests", "hostemu", "librsa_digest512_emu.so")
    hdrs = [os.path.join(ROOT, "cess_amd", "csrc", h) for h in ("rsa_digest512.hpp", "rsa_digest.hpp", "bls/h2c.hpp")]
    hdrs.append(os.path.join(ROOT, "tests", "hostemu", "rsa_digest_emu.hpp"))
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", src, "-o", lib])
    emu = ctypes.CDLL(lib)
    emu.emu_rsa_digest512.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                      ctypes.c_char_p]
    emu.emu_rsa_digest512_pad_block.argtypes = [ctypes.c_uint64, ctypes.c_char_p]
    emu.emu_rsa_digest512_pad_word_check.argtypes = [ctypes.c_uint64]
    emu.emu_rsa_digest512_padded_len.argtypes = [ctypes.c_uint64]
    emu.emu_rsa_digest512_padded_len.restype = ctypes.c_uint64
    emu.emu_rsa_digest512_prefix.argtypes = [ctypes.c_int, ctypes.c_char_p]
    return emu


def test_digest512_header_on_host():
    """rsa_digest512.hpp compiled for the host (no sanitizer, no preload): both digests of every length
    0..300 at start offsets 0..3, at the buffer's start and in its middle, equal hashlib's and no fetched
    dword lies outside the buffer's dwords; messages that end at the buffer's last byte; the word form of
    the padding equals the byte form, also where the bit length crosses 32 bits."""
    emu = _emu()
    rng = random.Random(0x5348)
    total = 64 + 308
    data = bytes(rng.randrange(256) for _ in range(total))
    buf = ctypes.create_string_buffer(data, total)
    assert ctypes.addressof(buf) % 4 == 0
    out = ctypes.create_string_buffer(64)
    for d in (SHA384, SHA512):
        w = HASH[d]().digest_size
        for base in (0, 61):
            for off in range(4):
                for ln in range(301):
                    start = base + off
                    assert emu.emu_rsa_digest512(d, ctypes.addressof(buf), total, start, ln, out) == 0, (start, ln)
                    assert out.raw[:w] == HASH[d](data[start:start + ln]).digest(), (d, start, ln)
        for total2 in range(261, 269):           # every residue mod 4, twice
            b2 = ctypes.create_string_buffer(data[:total2], total2)
            for start in range(4):
                assert emu.emu_rsa_digest512(d, ctypes.addressof(b2), total2, start, total2 - start, out) == 0
                assert out.raw[:w] == HASH[d](data[start:total2]).digest()
        pre = ctypes.create_string_buffer(19)
        emu.emu_rsa_digest512_prefix(d, pre)
        assert pre.raw == PREFIX[d]
    blk = ctypes.create_string_buffer(128)
    for ln in ((1 << 29) - 1, 1 << 29, (1 << 32) + 5, (1 << 61) - 1, 0, 111, 112, 127, 128):
        padded = (ln + 17 + 127) // 128 * 128
        assert emu.emu_rsa_digest512_padded_len(ln) == padded
        want = (bytes(128) + b"\x80" + bytes(padded - ln - 17) + (8 * ln).to_bytes(16, "big"))[-128:]
        emu.emu_rsa_digest512_pad_block(ln, blk)
        assert blk.raw == want, ln
        assert emu.emu_rsa_digest512_pad_word_check(ln) == 0, ln
    assert [emu.emu_rsa_digest512_padded_len(x) for x in (111, 112, 127, 128)] == [128, 256, 256, 256]
    for ln in range(521):
        assert emu.emu_rsa_digest512_pad_word_check(ln) == 0, ln


OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NOTE_KEYS = (".group_segment_fixed_size", ".max_flat_workgroup_size", ".private_segment_fixed_size", ".vgpr_count",
             ".vgpr_spill_count")


def _kernel_note(tmp_path, lib, kernel):
    """The metadata-note fields NOTE_KEYS of one kernel of the library's gfx950 code objects (the notes are
    read as tests/test_isa_guard.py reads them).  An entry's keys are sorted: the first two precede the
    kernel's own .name (the .name lines before it are its arguments'), the others follow it; .wavefront_size is
    an entry's last key."""
    copy = str(tmp_path / "libcess_bls.so")
    shutil.copy(lib, copy)
    subprocess.check_call([OBJDUMP, "--offloading", copy], cwd=tmp_path, stdout=subprocess.DEVNULL)
    for obj in glob.glob(str(tmp_path / "libcess_bls.so.*gfx950")):
        notes = subprocess.run([READELF, "--notes", obj], capture_output=True, text=True, check=True).stdout
        before, found = {}, None
        for line in notes.splitlines():
            key, _, val = line.strip().lstrip("- ").strip().partition(":")
            val = val.strip()
            if key == ".name" and found is None and val == kernel:
                found = dict(before)
            elif key == ".wavefront_size":
                if found is not None:
                    return found
                before = {}
            elif key in NOTE_KEYS:
                (before if found is None else found)[key] = int(val)
    return None


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="llvm tools not in this image")
def test_code_object_no_scratch(tmp_path):
    lib = os.path.join(ROOT, "cess_amd", "lib", "libcess_bls.so")
    if not os.path.exists(lib):
        pytest.skip("library not built (run __graft_entry__.build())")
    note = _kernel_note(tmp_path, lib, "_Z15k_rsa_digest512mPKhPKmPhjPmi")
    assert note is not None, "k_rsa_digest512 is not in the library"
    assert note[".private_segment_fixed_size"] == 0 and note[".vgpr_spill_count"] == 0
    assert note[".max_flat_workgroup_size"] == 64                       # __launch_bounds__(64)
    assert note[".vgpr_count"] <= 256
    assert 8 * note[".group_segment_fixed_size"] <= 160 * 1024          # at least 8 workgroups share a CU's LDS


# --- GPU ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gen():
    """Generated keys (1024 and 2048 bits) and, per digest, records at the SHA-512 block and padding edges
    with the model's codes; computed once."""
    rng = random.Random(0x52534133)
    keys = [o.gen_key(1024, 65537, rng), o.gen_key(2048, 65537, rng)]
    per = {}
    for dg, other in ((SHA384, SHA512), (SHA512, SHA384)):
        recs = []      # (key index, msg, sig)
        for ki, (n, e, d) in enumerate(keys):
            for ln in LENGTHS:
                msg = bytes(rng.randrange(256) for _ in range(ln))
                sig = o.sign_raw(n, d, t_of(dg, msg))
                recs.append((ki, msg, sig))                                          # valid
                if ln:
                    recs.append((ki, bytes([msg[0] ^ 1]) + msg[1:], sig))            # first message byte
                    recs.append((ki, msg[:-1] + bytes([msg[-1] ^ 0x80]), sig))       # last message bit
                recs.append((ki, msg + b"\x00", sig))                                # a byte appended
                recs.append((ki, msg, sig[:-1] + bytes([sig[-1] ^ 1])))              # a signature bit
                if ln + 11 <= (n.bit_length() + 7) // 8:                             # (where the raw mode has room)
                    recs.append((ki, msg, o.sign_raw(n, d, msg)))                    # signed over the bare message
                recs.append((ki, msg, o.sign_raw(n, d, t_of(other, msg))))           # made for the other digest's T
        recs.append((len(keys), b"no such key", bytes(256)))                         # key_idx >= k
        codes = [KEY if ki >= len(keys) else model_code(dg, keys[ki][0], keys[ki][1], m, s) for ki, m, s in recs]
        per[dg] = (recs, codes)
    return {"keys": keys, "per": per}


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


def _cols(recs):
    return [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [SHA384, SHA512])
def test_gpu_sha2_batch(ctx, ring_digests, dg):
    h = HASH[dg]
    rng = random.Random(4)
    msgs = [bytes(rng.randrange(256) for _ in range(ln)) for ln in range(300)]
    assert ctx.sha2_batch(dg, msgs) == [h(m).digest() for m in msgs]
    # one long message among 63 short ones of the same wave
    wave = [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 200))) for _ in range(64)]
    wave[17] = bytes(rng.randrange(256) for _ in range(70001))
    assert ctx.sha2_batch(dg, wave) == [h(m).digest() for m in wave]
    assert ctx.sha2_batch(dg, []) == []
    assert ctx.sha2_batch(dg, [b""]) == [h(b"").digest()]
    assert ctx.sha2_batch(dg, [b""] * 65) == [h(b"").digest()] * 65
    # ring's digest rows, and the 1,000,000-byte message of its long-input rows (FIPS 180: "a" x 10^6)
    rows = [(m, out) for d, m, out in ring_digests if d == dg]
    assert len(rows) == 2 and ctx.sha2_batch(dg, [m for m, _ in rows]) == [out for _, out in rows]
    million = b"a" * 1000000
    assert ctx.sha2_batch(dg, [b"abc", million]) == [h(b"abc").digest(), h(million).digest()]


# the padding edges of both block sizes, and the lengths around the 256-byte staging rounds' boundaries,
# where the carry dword and the round's last word are used
EDGE_LENGTHS = (0, 1, 55, 56, 63, 64, 111, 112, 119, 120, 127, 128) + tuple(range(247, 266)) + tuple(range(503, 522))


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [SHA256, SHA384, SHA512])
def test_gpu_sha2_batch_round_edges(ctx, dg):
    """What the three digests share, the message stream: every edge length at every start alignment (a
    leading filler of 0..3 bytes shifts the whole list), in one batch of more than a wave."""
    h = HASH[dg]
    rng = random.Random(6)
    msgs = []
    for filler in range(4):
        msgs.append(bytes(rng.randrange(256) for _ in range(filler)))
        msgs += [bytes(rng.randrange(256) for _ in range(ln)) for ln in EDGE_LENGTHS]
    starts = np.cumsum([0] + [len(m) for m in msgs])[:-1]
    for ln in EDGE_LENGTHS:                          # (the test's own premise)
        assert {int(s) % 4 for s, m in zip(starts, msgs) if len(m) == ln} >= {0, 1, 2, 3}, ln
    assert len(msgs) >= 65
    assert ctx.sha2_batch(dg, msgs) == [h(m).digest() for m in msgs]


@pytest.mark.gpu
def test_gpu_sha2_batch_sha256_and_bad_selector(ctx):
    from cess_amd import bls
    rng = random.Random(5)
    msgs = [bytes(rng.randrange(256) for _ in range(ln)) for ln in (0, 1, 55, 56, 64, 200, 257)]
    assert ctx.sha2_batch(SHA256, msgs) == ctx.sha256_batch(msgs) == [hashlib.sha256(m).digest() for m in msgs]
    lib = bls.load_library()
    out = (ctypes.c_uint8 * 64)()
    offs = (ctypes.c_uint64 * 2)(0, 0)
    assert lib.cess_sha2_batch(ctx._h, 3, 1, out, offs, out) == bls.E_INVALID_ARG
    with pytest.raises(bls.BlsInfraError) as ei:
        ctx.rsa_verify_digest_batch(3, [0], [b"m"], [bytes(256)])
    assert ei.value.status == bls.E_INVALID_ARG
    with pytest.raises(bls.BlsInfraError) as ei:
        ctx.verify_rsa_alg(4, o.encode_spki((1 << 2047) | 1, 65537), b"m", bytes(256))
    assert ei.value.status == bls.E_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["SHA384", "SHA512"])
def test_gpu_ring_rows(ctx, ring, name):
    from cess_amd import bls
    dg, alg = DIGEST_OF[name], {"SHA384": bls.RSA_ALG_2048_8192_SHA384, "SHA512": bls.RSA_ALG_2048_8192_SHA512}[name]
    rows = [r for r in ring if r["digest"] == name]
    ders = list(dict.fromkeys(r["key"] for r in rows))
    assert ctx.rsa_keys_load(ders, bls.RSA_KEY_PKCS1, policy=bls.RSA_POLICY_RING_2048_8192) == [0] * len(ders)
    recs = [(ders.index(r["key"]), r["msg"], r["sig"]) for r in rows]
    want = bytes(r["code"] for r in rows)
    assert ctx.rsa_verify_digest_batch(dg, *_cols(recs)) == want
    assert _device_codes(ctx, lambda *a: ctx.rsa_verify_digest_batch_device(dg, *a), recs) == want
    passed_bits = set()
    for r in rows:
        assert ctx.verify_rsa_alg(alg, r["key"], r["msg"], r["sig"], bls.RSA_KEY_PKCS1) == (r["code"] == 0), r["comment"]
        if r["code"] == 0:
            passed_bits.add(ring_key(r["key"])[0].bit_length())
    assert passed_bits >= {2048, 3072}
    # RSA_PKCS1_3072_8192_SHA384: the 3072- and 4096-bit passing rows pass, a 2048-bit key is rejected
    if name == "SHA384":
        seen = set()
        for r in rows:
            bits = ring_key(r["key"])[0].bit_length()
            if r["code"] != 0 or bits in seen:
                continue
            seen.add(bits)
            if bits >= 3072:
                assert ctx.verify_rsa_alg(bls.RSA_ALG_3072_8192_SHA384, r["key"], r["msg"], r["sig"], bls.RSA_KEY_PKCS1)
            else:
                with pytest.raises(bls.BlsInfraError) as ei:
                    ctx.verify_rsa_alg(bls.RSA_ALG_3072_8192_SHA384, r["key"], r["msg"], r["sig"], bls.RSA_KEY_PKCS1)
                assert ei.value.status == bls.E_BAD_KEY
        assert seen >= {2048, 3072}
        # under policy 2 the table drops the 2048-bit keys: their records are KEY, the others unchanged
        st = ctx.rsa_keys_load(ders, bls.RSA_KEY_PKCS1, policy=bls.RSA_POLICY_RING_3072_8192)
        small = [ring_key(d)[0].bit_length() < 3072 for d in ders]
        assert st == [bls.E_BAD_KEY if s else 0 for s in small] and any(small) and not all(small)
        assert ctx.rsa_verify_digest_batch(dg, *_cols(recs)) == bytes(KEY if small[k] else c for (k, _, _), c in zip(recs, want))


@pytest.mark.gpu
@pytest.mark.parametrize("dg", [SHA384, SHA512])
def test_gpu_generated_records(ctx, gen, dg):
    keys = gen["keys"]
    recs, want = gen["per"][dg]
    assert {OK, MISMATCH, KEY} <= set(want) and want.count(OK) == 2 * len(LENGTHS)
    assert ctx.rsa_keys_load([o.encode_spki(n, e) for n, e, _ in keys]) == [0, 0]      # policy 0: the 1024-bit key loads
    idx, msgs, sigs = _cols(recs)
    got = ctx.rsa_verify_digest_batch(dg, idx, msgs, sigs)
    assert list(got) == want
    assert list(_device_codes(ctx, lambda *a: ctx.rsa_verify_digest_batch_device(dg, *a), recs)) == want
    # the unchanged raw path over T computed here gives the same codes
    assert ctx.rsa_verify_batch(idx, [t_of(dg, m) for m in msgs], sigs) == got


@pytest.mark.gpu
def test_gpu_msg_len_small_key(ctx):
    """k = 64 < len(T) + 11 = 78 / 94: MSG_LEN for both digests (k >= 62: SHA-256 still fits)."""
    rng = random.Random(9)
    n, e, d = o.gen_key(512, 65537, rng)
    assert ctx.rsa_keys_load([o.encode_spki(n, e)]) == [0]
    msg = b"a report"
    sig = o.sign_raw(n, d, msg)
    for dg in (SHA384, SHA512):
        assert model_code(dg, n, e, msg, sig) == MSG_LEN
        assert list(ctx.rsa_verify_digest_batch(dg, [0, 0], [msg, b""], [sig, sig])) == [MSG_LEN, MSG_LEN]
    sig256 = o.sign_raw(n, d, t_of(SHA256, msg))
    assert list(ctx.rsa_verify_digest_batch(SHA256, [0, 0], [msg, b""], [sig256, sig256])) == [OK, MISMATCH]


@pytest.mark.gpu
def test_gpu_key_uniform_path(ctx, gen):
    """One 2048-bit key, 512 records (>= 256 per key: the key-sorted lists and k_rsa_verify_2048u), SHA-512,
    message lengths cycling 0..127, bad records at the ends of the first wave, the start of the second and
    the end of the batch."""
    from cess_amd import bls
    n, e, d = gen["keys"][1]
    rng = random.Random(77)
    base = []
    for ln in range(128):
        m = bytes(rng.randrange(256) for _ in range(ln))
        base.append((m, o.sign_raw(n, d, t_of(SHA512, m))))
    recs = [base[i % 128] for i in range(512)]
    bad = (0, 63, 64, 511)
    recs[0] = (recs[0][0] + b"x", recs[0][1])                                # another message
    recs[63] = (recs[63][0], recs[63][1][:-1] + bytes([recs[63][1][-1] ^ 1]))   # signature bit
    recs[64] = (recs[64][0][:-1] + bytes([recs[64][0][-1] ^ 4]), recs[64][1])   # message bit
    recs[511] = (recs[511][0], recs[511][1][1:])                             # SIG_LEN
    want = [model_code(SHA512, n, e, m, s) for m, s in recs]
    assert [i for i, c in enumerate(want) if c] == list(bad) and want[511] == SIG_LEN
    assert ctx.rsa_keys_load([o.encode_spki(n, e)], policy=bls.RSA_POLICY_RING_2048_8192) == [0]
    codes, words = ctx.rsa_verify_digest_batch(SHA512, [0] * 512, [r[0] for r in recs], [r[1] for r in recs],
                                               with_bitmap=True)
    assert list(codes) == want
    full = (1 << 64) - 1
    assert words == [full & ~1 & ~(1 << 63), full & ~1] + [full] * 5 + [full & ~(1 << 63)]


@pytest.mark.gpu
def test_gpu_multi_device_context(gen):
    from cess_amd import bls
    keys = gen["keys"]
    m = bls.Context(max_batch=1024, devices=[0, 0])
    try:
        assert m.rsa_keys_load([o.encode_spki(n, e) for n, e, _ in keys]) == [0, 0]
        got = {dg: m.rsa_verify_digest_batch(dg, *_cols(gen["per"][dg][0])) for dg in (SHA384, SHA512)}
        recs, want = gen["per"][SHA512]
        i_ok = max(i for i, (r, c) in enumerate(zip(recs, want)) if c == OK and r[0] == 1)
        i_bad = max(i for i, (r, c) in enumerate(zip(recs, want)) if c == MISMATCH and r[0] == 1)
        spki = o.encode_spki(*keys[1][:2])
        assert m.verify_rsa_alg(bls.RSA_ALG_2048_8192_SHA512, spki, recs[i_ok][1], recs[i_ok][2]) is True
        assert m.verify_rsa_alg(bls.RSA_ALG_2048_8192_SHA512, spki, recs[i_bad][1], recs[i_bad][2]) is False
        assert m.sha2_batch(SHA384, [b"abc"]) == [hashlib.sha384(b"abc").digest()]
    finally:
        m.close()
    for dg in (SHA384, SHA512):
        assert len(gen["per"][dg][0]) > 128                    # both shards hold records
        assert list(got[dg]) == gen["per"][dg][1]


@pytest.mark.gpu
def test_gpu_digest_stage(gen):
    from cess_amd import bls
    keys, recs = gen["keys"], gen["per"][SHA384][0][:40]
    c = bls.Context(max_batch=4096, profile=True)
    try:
        c.rsa_keys_load([o.encode_spki(n, e) for n, e, _ in keys])
        before = list(c.stage_stats(reset=True))
        c.rsa_verify_digest_batch(SHA384, *_cols(recs))
        st = c.stage_stats(reset=True)
        assert st["k_rsa_digest"][1] == 1 and st["k_rsa_digest"][0] > 0 and st["k_rsa_verify"][1] == 1
        names = list(st)
        assert names == before and names.index("k_rsa_digest") == len(names) - 1
        assert names == ["k_decode_sig", "k_decode_pk", "k_hash", "k_prepare", "k_miller", "k_final", "k_rsa_classify",
                         "k_rsa_verify", "k_group", "k_sign", "k_rsa_digest"]
    finally:
        c.close()


@pytest.mark.gpu
def test_gpu_sha256_entries_unchanged(ctx, gen):
    """rsa_verify_digest_batch(SHA256, ...) is rsa_verify_sha256_batch: same codes and bitmap on the
    generated records (signed for other digests: the codes are mostly MISMATCH, with KEY, and OK where a
    SHA-256 signature is added)."""
    n, e, d = gen["keys"][1]
    recs = list(gen["per"][SHA384][0])
    for ln in (0, 55, 56, 64, 300):
        m = bytes(range(256)) * 2
        recs.append((1, m[:ln], o.sign_raw(n, d, t_of(SHA256, m[:ln]))))
    assert ctx.rsa_keys_load([o.encode_spki(n_, e_) for n_, e_, _ in gen["keys"]]) == [0, 0]
    idx, msgs, sigs = _cols(recs)
    new = ctx.rsa_verify_digest_batch(SHA256, idx, msgs, sigs, with_bitmap=True)
    old = ctx.rsa_verify_sha256_batch(idx, msgs, sigs, with_bitmap=True)
    assert new == old
    assert list(new[0][-5:]) == [OK] * 5 and new[0][-6] == KEY and MISMATCH in new[0]
    assert _device_codes(ctx, lambda *a: ctx.rsa_verify_digest_batch_device(SHA256, *a), recs) == \
        _device_codes(ctx, ctx.rsa_verify_sha256_batch_device, recs) == new[0]
    from cess_amd import bls
    spki = o.encode_spki(n, e)
    assert ctx.verify_rsa_alg(bls.RSA_ALG_2048_8192_SHA256, spki, recs[-1][1], recs[-1][2]) is True
    assert ctx.verify_rsa_sha256(spki, recs[-1][1], recs[-1][2]) is True
