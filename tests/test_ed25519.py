"""Batch Ed25519 under ring's ED25519 rules (include/cess_ed25519.h).

CPU: the plain-Python model (tests/ed25519_model.py) against the two fixtures;
cess_amd/csrc/ed25519.hpp built for the host (tests/hostemu/ed25519_emu.cpp,
-DCESS_HOSTEMU, no sanitizer preload) against Python integers and the model; the
same code as a stand-alone program under the address and undefined-behaviour
sanitizers (its record file also takes the crafted rows of
tests/golden/ring_ed25519_crafted.json, whose codes are ring's own); the
code-object notes of the new kernels; the Rust declarations and the Python
constants against the header.
GPU: the fixtures and generated batches through every entry point.
"""
import ctypes
import json
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ed25519_model as model
from test_rsa_sha2 import OBJDUMP, READELF, _kernel_note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = model.P, model.L
OK, SIG_LEN, SIG_RANGE, KEY, MISMATCH = range(5)
KERNELS = {"k_ed25519_keys": "_Z14k_ed25519_keysmPKhPKmPjPhS4_",
           "k_ed25519_pack": "_Z14k_ed25519_packmPKjjPKhS2_PKmS2_S4_PhPm",
           "k_ed25519_verify": "_Z16k_ed25519_verifymPKjjPKhS0_S0_S2_PKmS2_Ph"}
VERIFY_BLOCK = 256                      # k_ed25519_verify's workgroup (CESS_LB)
# mul / sqr input bound of ed25519.hpp: even limbs < 13 * 2^24, odd limbs < 13 * 2^23
MAX_EVEN, MAX_ODD = 13 * 2**24 - 1, 13 * 2**23 - 1
BITS = [26, 25] * 5
WEIGHT = [sum(BITS[:k]) for k in range(10)]


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ring():
    """(key, msg, sig) of the 323 reference rows"""
    rows = _load("ring_ed25519.json")["rows"]
    assert len(rows) == 323
    return [tuple(bytes.fromhex(r[k]) for k in ("pub", "msg", "sig")) for r in rows]


@pytest.fixture(scope="module")
def edges():
    e = _load("ed25519_edges.json")
    rows = [(r["name"], r["group"], bytes.fromhex(r["key"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"])
            for r in e["rows"]]
    keys = [(k["name"], bytes.fromhex(k["key"]), k["loads"]) for k in e["keys"]]
    return {"rows": rows, "keys": keys}


def tamper(sig):
    return bytes([sig[0] ^ 1]) + sig[1:]


# --- CPU: the model and the fixtures ------------------------------------------
def test_model_on_fixtures(ring, edges):
    for key, msg, sig in ring:
        assert model.verify_code(key, msg, sig) == OK
        assert model.verify_code(key, msg, tamper(sig)) == MISMATCH
    for name, _, key, msg, sig, code in edges["rows"]:
        assert model.verify_code(key, msg, sig) == code, name
    for name, key, loads in edges["keys"]:
        assert model.key_loads(key) == loads, name
    by_name = {r[0]: r[5] for r in edges["rows"]}
    assert by_name["S + L"] == by_name["S = L"] == by_name["S = 2^256 - 1"] == SIG_RANGE
    assert by_name["S = L - 1"] == MISMATCH
    assert by_name["identity key, S = 0, R = the p + 1 encoding (never matches)"] == MISMATCH
    assert by_name["identity key encoded as p + 1"] == by_name["identity key with the sign bit set (x = 0 stays 0)"] == OK
    assert {len(r[3]) for r in edges["rows"] if r[1] == "sha512"} == {0, 47, 48, 63, 64, 65, 175, 176, 191, 192, 193, 1000}
    starts = np.cumsum([0] + [len(r[3]) for r in edges["rows"] if r[1] == "align"])[:-1]
    assert sorted(int(s) % 4 for s in starts) == [0, 1, 2, 3]


# --- CPU: ed25519.hpp on the host ----------------------------------------------
def _emu():
    src = os.path.join(ROOT, "tests", "hostemu", "ed25519_emu.cpp")
    lib = os.path.join(ROOT, "tests", "hostemu", "libed25519_emu.so")
    hdrs = [os.path.join(ROOT, "cess_amd", "csrc", h) for h in ("ed25519.hpp", "rsa_digest512.hpp", "rsa_digest.hpp",
                                                                "bls/h2c.hpp", "bls/field.hpp", "kernels.hpp")]
    hdrs.append(os.path.join(ROOT, "tests", "probe", "ed25519_probe.hip"))      # its lane functions (emu_edp)
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", src, "-o", lib])
    emu = ctypes.CDLL(lib)
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    emu.emu_ed_fe_op.argtypes = [ctypes.c_int, u32p, u32p, u32p]
    emu.emu_ed_fe_frombytes.argtypes = [ctypes.c_char_p, u32p]
    emu.emu_ed_fe_tobytes.argtypes = [u32p, ctypes.c_char_p]
    emu.emu_ed_col_max.argtypes = [u64p, u64p, ctypes.c_int]
    emu.emu_ed_sc_lt_l.argtypes = [ctypes.c_char_p]
    emu.emu_ed_sc_reduce.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    emu.emu_ed_sc_digits.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int8)]
    emu.emu_ed_key_table.argtypes = [ctypes.c_char_p, ctypes.c_uint64, u32p]
    emu.emu_ed_verify.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p,
                                  ctypes.c_uint64]
    return emu


@pytest.fixture(scope="module")
def emu():
    return _emu()


def limbs_of(v):
    out = []
    for b in BITS:
        out.append(v & ((1 << b) - 1))
        v >>= b
    assert v == 0
    return out


def value_of(limbs):
    return sum(int(x) << w for x, w in zip(limbs, WEIGHT))


def _arr(limbs):
    return (ctypes.c_uint32 * 10)(*limbs)


def _op(emu, op, a, b=None):
    out = (ctypes.c_uint32 * 10)()
    emu.emu_ed_fe_op(op, _arr(a), _arr(b if b is not None else a), out)
    return list(out)


MUL, SQR, ADD, SUB, NEG, CARRY, INVERT, POW22523, NEG_TIGHT = range(9)
TIGHT_EVEN, TIGHT_ODD = 2**26 + 2**12, 2**25 + 2**16


def _is_tight(limbs):
    return all(x <= (TIGHT_ODD if k & 1 else TIGHT_EVEN) for k, x in enumerate(limbs))


def test_field_on_host(emu):
    rng = random.Random(0x25519)
    structured = [0, 1, 2, 19, P - 1, P, P + 18, 2**255 - 1]
    vals = structured + [rng.randrange(2**255) for _ in range(3000)]
    # from-bytes (top bit masked, no canonical check) and the canonical encoding, zero and sign tests
    for v in vals:
        out = (ctypes.c_uint32 * 10)()
        emu.emu_ed_fe_frombytes((v | rng.randrange(2) << 255).to_bytes(32, "little"), out)
        assert value_of(out) == v and list(out) == limbs_of(v)
        enc = ctypes.create_string_buffer(32)
        flags = emu.emu_ed_fe_tobytes(out, enc)
        assert int.from_bytes(enc.raw, "little") == v % P
        assert flags == (1 if v % P == 0 else 0) | ((v % P) & 1) << 1
    hi, lo = ctypes.c_uint64(), ctypes.c_uint64()
    emu.emu_ed_col_max(hi, lo, 1)
    top = [MAX_ODD if k & 1 else MAX_EVEN for k in range(10)]
    loose = lambda: [rng.randrange((MAX_ODD if k & 1 else MAX_EVEN) + 1) for k in range(10)]   # noqa: E731
    pairs = [(limbs_of(a), limbs_of(b)) for a in structured for b in structured]
    pairs += [(limbs_of(rng.randrange(2**255)), limbs_of(rng.randrange(2**255))) for _ in range(2000)]
    pairs += [(loose(), loose()) for _ in range(2000)]
    pairs += [(top, top), (top, limbs_of(P - 1)), (limbs_of(1), top)]
    for a, b in pairs:
        va, vb = value_of(a), value_of(b)
        r = _op(emu, MUL, a, b)
        assert value_of(r) % P == va * vb % P and _is_tight(r)
        r = _op(emu, SQR, a)
        assert value_of(r) % P == va * va % P and _is_tight(r)
        r = _op(emu, SUB, a, b)
        assert value_of(r) % P == (va - vb) % P and _is_tight(r)
        r = _op(emu, NEG, a)
        assert value_of(r) % P == -va % P and _is_tight(r)
        r = _op(emu, CARRY, a)
        assert value_of(r) % P == va % P and _is_tight(r)
        enc = ctypes.create_string_buffer(32)
        emu.emu_ed_fe_tobytes(_arr(a), enc)
        assert int.from_bytes(enc.raw, "little") == va % P
    # add of two tight values is loose; neg_tight of a tight value is within the input bound
    for _ in range(500):
        a, b = _op(emu, CARRY, loose()), _op(emu, CARRY, loose())
        s = _op(emu, ADD, a, b)
        assert value_of(s) == value_of(a) + value_of(b) and all(x <= 2 * (TIGHT_ODD if k & 1 else TIGHT_EVEN)
                                                                for k, x in enumerate(s))
        n = _op(emu, NEG_TIGHT, a)
        assert value_of(n) % P == -value_of(a) % P and all(x <= t for x, t in zip(n, top))
    # the 128-bit shadow of every column sum so far, the maximal inputs included
    emu.emu_ed_col_max(hi, lo, 0)
    assert hi.value == 0 and 2**61 < lo.value < 2**63
    for v in structured + [rng.randrange(2**255) for _ in range(40)]:
        a = limbs_of(v)
        assert value_of(_op(emu, INVERT, a)) % P == pow(v, P - 2, P)
        assert value_of(_op(emu, POW22523, a)) % P == pow(v, (P - 5) // 8, P)
    assert value_of(_op(emu, INVERT, top)) % P == pow(value_of(top), P - 2, P)
    emu.emu_ed_col_max(hi, lo, 0)
    assert hi.value == 0


def test_scalars_on_host(emu):
    rng = random.Random(0x5ca1a5)
    xs = [0, L - 1, L, L + 1, 2**512 - 1, 2**252, 2**252 - 1, 2**256, 2**504]
    xs += [k * L + d for k in (2, 3, 2**128, 2**259, (2**512 - 1) // L) for d in (-1, 0, 1) if k * L + d < 2**512]
    xs += [rng.randrange(2**512) for _ in range(3000)] + [rng.randrange(2**256) for _ in range(300)]
    out = ctypes.create_string_buffer(32)
    for x in xs:
        emu.emu_ed_sc_reduce(x.to_bytes(64, "little"), out)
        assert int.from_bytes(out.raw, "little") == x % L, hex(x)
    for s, want in ((L - 1, 1), (L, 0), (L + 1, 0), (2**256 - 1, 0), (0, 1), (2**252, 1), (2**253, 0)):
        assert emu.emu_ed_sc_lt_l(s.to_bytes(32, "little")) == want
    for _ in range(300):
        s = rng.randrange(2**256)
        assert emu.emu_ed_sc_lt_l(s.to_bytes(32, "little")) == (1 if s < L else 0)
    digits = (ctypes.c_int8 * 64)()
    for s in [0, 1, 7, 8, 15, 16, L - 1, 2**252, 2**253 - 1] + [rng.randrange(L) for _ in range(500)]:
        emu.emu_ed_sc_digits(s.to_bytes(32, "little"), digits)
        d = list(digits)
        assert all(-8 <= x <= 7 for x in d)
        assert sum(x * 16**(63 - i) for i, x in enumerate(d)) == s


def test_key_tables_on_host(emu, ring, edges):
    keys = list(dict.fromkeys([r[0] for r in ring] + [k for _, k, _ in edges["keys"]] + [r[2] for r in edges["rows"]]))
    tab = (ctypes.c_uint32 * 240)()
    seen = set()
    for key in keys:
        st = emu.emu_ed_key_table(key, len(key), tab)
        want = 1 if len(key) != 32 else 0 if model.key_loads(key) else 2
        assert st == want, key.hex()
        seen.add(st)
        if st == 0:
            got = [tuple(value_of(tab[30 * i + 10 * j:30 * i + 10 * j + 10]) for j in range(3)) for i in range(8)]
            assert all(_is_tight(tab[10 * q:10 * q + 10]) for q in range(24))
            assert [tuple(v % P for v in e) for e in got] == model.neg_multiples(key), key.hex()
    assert seen == {0, 1, 2}


def test_verify_on_host(emu, ring, edges):
    for key, msg, sig in ring:
        assert emu.emu_ed_verify(key, 32, msg, len(msg), sig, 64) == OK
        t = tamper(sig)
        assert emu.emu_ed_verify(key, 32, msg, len(msg), t, 64) == MISMATCH
    for name, _, key, msg, sig, code in edges["rows"]:
        assert emu.emu_ed_verify(key, len(key), msg, len(msg), sig, len(sig)) == code, name
    hi, lo = ctypes.c_uint64(), ctypes.c_uint64()
    emu.emu_ed_col_max(hi, lo, 0)
    assert hi.value == 0


_san = []
SAN_ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def san_exe():
    """The emulator as a stand-alone program (its own main, run as a child process) built with the address
    and undefined-behaviour sanitizers; built once per test run, in a temporary directory."""
    if not _san:
        exe = os.path.join(tempfile.mkdtemp(prefix="ed25519_san_"), "ed25519_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-DCESS_HOSTEMU",
                               "-DED25519_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "hostemu", "ed25519_emu.cpp"), "-o", exe])
        _san.append(exe)
    return _san[0]


def test_verify_under_sanitizers(tmp_path, ring, edges):
    """The emulator's verify over the three fixtures as a stand-alone program under the sanitizers."""
    exe = san_exe()
    crafted = [tuple(bytes.fromhex(r[k]) for k in ("key", "msg", "sig")) + (r["code"],)
               for r in _load("ring_ed25519_crafted.json")["rows"]]
    assert len(crafted) > 300
    hx = lambda b: b.hex() if b else "-"   # noqa: E731
    recs = str(tmp_path / "records.txt")
    with open(recs, "w") as f:
        for key, msg, sig in ring:
            f.write("%s %s %s %d\n" % (hx(key), hx(msg), hx(sig), OK))
            f.write("%s %s %s %d\n" % (hx(key), hx(msg), hx(tamper(sig)), MISMATCH))
        for _, _, key, msg, sig, code in edges["rows"]:
            f.write("%s %s %s %d\n" % (hx(key), hx(msg), hx(sig), code))
        for key, msg, sig, code in crafted:
            f.write("%s %s %s %d\n" % (hx(key), hx(msg), hx(sig), code))
    env = dict(os.environ, **SAN_ENV)
    r = subprocess.run([exe, recs], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d records, 0 wrong" % (2 * len(ring) + len(edges["rows"]) + len(crafted)) in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# --- CPU: the library's code objects, the bindings --------------------------------
@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="llvm tools not in this image")
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_code_object_notes(tmp_path, kernel):
    lib = os.path.join(ROOT, "cess_amd", "lib", "libcess_bls.so")
    if not os.path.exists(lib):
        pytest.skip("library not built (run __graft_entry__.build())")
    note = _kernel_note(tmp_path, lib, KERNELS[kernel])
    assert note is not None, kernel + " is not in the library"
    assert note[".private_segment_fixed_size"] == 0 and note[".vgpr_spill_count"] == 0
    if kernel == "k_ed25519_verify":
        assert note[".vgpr_count"] <= 256 and note[".max_flat_workgroup_size"] == VERIFY_BLOCK


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_rust_declares_every_header_function():
    text = _strip(open(os.path.join(ROOT, "include", "cess_ed25519.h")).read())
    h = {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
         for m in re.finditer(r"\b(cess_ed25519_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text)}
    assert {"cess_ed25519_keys_load", "cess_ed25519_verify_batch", "cess_ed25519_verify_batch_device",
            "cess_ed25519_verify"} <= set(h)
    rust = open(os.path.join(ROOT, "utils", "verify-bls-signatures-gpu", "src", "ffi.rs")).read()
    r = {}
    for m in re.finditer(r"pub fn (cess_ed25519_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->[^;]*)?;", rust, flags=re.S):
        args = m.group(2).strip().rstrip(",")
        r[m.group(1)] = 0 if not args else args.count(",") + 1
    assert r == h
    from cess_amd import bls
    assert sorted(bls.EXPORTS_ED25519) == sorted(h)


def test_python_constants_and_policy():
    import cess_amd
    from cess_amd import bls
    text = _strip(open(os.path.join(ROOT, "include", "cess_ed25519.h")).read())
    enum = dict((k, int(v)) for k, v in re.findall(r"CESS_ED25519_([A-Z_]+)\s*=\s*(\d+)", text))
    assert enum == {"OK": bls.ED25519_OK, "SIG_LEN": bls.ED25519_SIG_LEN, "SIG_RANGE": bls.ED25519_SIG_RANGE,
                    "KEY": bls.ED25519_KEY, "MISMATCH": bls.ED25519_MISMATCH} == {v: k for k, v in bls.ED25519_CODE_NAMES.items()}
    assert (OK, SIG_LEN, SIG_RANGE, KEY, MISMATCH) == (bls.ED25519_OK, bls.ED25519_SIG_LEN, bls.ED25519_SIG_RANGE,
                                                       bls.ED25519_KEY, bls.ED25519_MISMATCH)
    assert int(re.search(r"#define CESS_ED25519_POLICY_RING (\d+)", text).group(1)) == bls.ED25519_POLICY_RING == 0
    assert cess_amd.verify_ed25519 is bls.verify_ed25519 and cess_amd.ED25519_MISMATCH == 4
    # an unknown policy is refused before anything else is looked at (no device needed)
    lib = bls.load_library()
    for s in bls.EXPORTS_ED25519:
        assert hasattr(lib, s), s
    ok = ctypes.c_int(7)
    assert lib.cess_ed25519_keys_load(None, 0, None, None, 1, None) == bls.E_INVALID_ARG
    assert lib.cess_ed25519_verify(None, None, 0, None, 0, None, 0, -1, ctypes.byref(ok)) == bls.E_INVALID_ARG
    assert ok.value == 7


# --- GPU ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from cess_amd import bls
    c = bls.Context(max_batch=1024)
    yield c
    c.close()


def bitmap_of(codes):
    words = [0] * ((len(codes) + 63) // 64)
    for i, c in enumerate(codes):
        if c == OK:
            words[i >> 6] |= 1 << (i & 63)
    return words


def table_of(recs):
    """distinct keys of (key, msg, sig) records and the records as (index, msg, sig) columns"""
    keys = list(dict.fromkeys(r[0] for r in recs))
    pos = {k: i for i, k in enumerate(keys)}
    return keys, [pos[r[0]] for r in recs], [r[1] for r in recs], [r[2] for r in recs]


def device_codes(c, idx, msgs, sigs):
    S = b"".join(sigs)
    M = b"\xa5" + b"".join(msgs)          # messages start at an odd device address
    so = np.cumsum([0] + [len(s) for s in sigs]).astype(np.uint64)
    mo = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    d = [c.to_device(np.array(idx, dtype=np.uint32)), c.to_device(S), c.to_device(so), c.to_device(M), c.to_device(mo)]
    dc = c.device_alloc(len(idx))
    try:
        c.ed25519_verify_batch_device(len(idx), d[0], d[1], d[2], d[3] + 1, d[4], dc)
        c.synchronize()
        return c.from_device(dc, len(idx))
    finally:
        for p in d + [dc]:
            c.device_free(p)


def cycled(ring, n):
    """n records cycled from the reference rows, every fifth tampered, and their codes"""
    recs = [ring[i % len(ring)] for i in range(n)]
    recs = [(k, m, tamper(s)) if i % 5 == 4 else (k, m, s) for i, (k, m, s) in enumerate(recs)]
    return recs, [MISMATCH if i % 5 == 4 else OK for i in range(n)]


@pytest.mark.gpu
def test_gpu_reference_rows(ctx, ring):
    from cess_amd import bls
    recs = [r for k, m, s in ring for r in ((k, m, s), (k, m, tamper(s)))]
    want = [OK, MISMATCH] * len(ring)
    keys, idx, msgs, sigs = table_of(recs)
    assert ctx.ed25519_keys_load(keys) == [0] * len(keys)
    codes, words = ctx.ed25519_verify_batch(idx, msgs, sigs, with_bitmap=True)
    assert list(codes) == want
    assert words == bitmap_of(want) and len(words) == 11
    assert list(device_codes(ctx, idx, msgs, sigs)) == want
    for i in range(0, 24, 2):
        k, m, s = ring[13 * i % len(ring)]
        assert ctx.verify_ed25519(k, m, s) is True and ctx.verify_ed25519(k, m, tamper(s)) is False
        assert bls.verify_ed25519(s, m, k, ctx=ctx) is True
    # the single-record entry used a table of its own: the loaded one is still in place
    assert list(ctx.ed25519_verify_batch(idx[:10], msgs[:10], sigs[:10])) == want[:10]


@pytest.mark.gpu
def test_gpu_edges(ctx, edges):
    from cess_amd import bls
    names = [k[0] for k in edges["keys"]]
    st = ctx.ed25519_keys_load([k[1] for k in edges["keys"]])
    assert st == [0 if k[2] else bls.E_BAD_KEY for k in edges["keys"]], [n for n, s, k in zip(names, st, edges["keys"])
                                                                       if (s == 0) != k[2]]
    rows = edges["rows"]
    keys, idx, msgs, sigs = table_of([r[2:5] for r in rows])
    assert ctx.ed25519_keys_load(keys) == [0 if model.key_loads(k) else bls.E_BAD_KEY for k in keys]
    want = [r[5] for r in rows]
    codes, words = ctx.ed25519_verify_batch(idx, msgs, sigs, with_bitmap=True)
    assert list(codes) == want, [r[0] for r, c in zip(rows, codes) if c != r[5]]
    assert words == bitmap_of(want) and set(want) == {OK, SIG_LEN, SIG_RANGE, KEY, MISMATCH}
    assert list(device_codes(ctx, idx, msgs, sigs)) == want
    al = [i for i, r in enumerate(rows) if r[1] == "align"]
    assert list(ctx.ed25519_verify_batch([idx[i] for i in al], [msgs[i] for i in al], [sigs[i] for i in al])) == [OK] * 4
    for name, _, key, msg, sig, code in rows:
        if model.key_loads(key):
            assert ctx.verify_ed25519(key, msg, sig) == (code == OK), name
        else:
            with pytest.raises(bls.BlsInfraError) as ei:
                ctx.verify_ed25519(key, msg, sig)
            assert ei.value.status == bls.E_BAD_KEY
            assert bls.verify_ed25519(sig, msg, key, ctx=ctx) is False


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, VERIFY_BLOCK - 1, VERIFY_BLOCK, VERIFY_BLOCK + 1])
def test_gpu_batch_sizes(ctx, ring, n):
    recs, want = cycled(ring, n)
    keys, idx, msgs, sigs = table_of(recs)
    assert ctx.ed25519_keys_load(keys) == [0] * len(keys)
    codes, words = ctx.ed25519_verify_batch(idx, msgs, sigs, with_bitmap=True)
    assert list(codes) == want
    assert words == bitmap_of(want) and words[-1] >> ((n - 1) % 64 + 1) == 0


@pytest.mark.gpu
def test_gpu_null_outputs_and_empty_batch(ctx, ring):
    from cess_amd import bls
    lib = bls.load_library()
    n = 65
    recs, want = cycled(ring, n)
    keys, idx, msgs, sigs = table_of(recs)
    assert ctx.ed25519_keys_load(keys) == [0] * len(keys)
    a_idx = (ctypes.c_uint32 * n)(*idx)
    S, M = bls._buf(b"".join(sigs)), bls._buf(b"".join(msgs))
    so, mo = bls._offsets([len(s) for s in sigs]), bls._offsets([len(m) for m in msgs])
    codes = (ctypes.c_uint8 * n)(*([0xEE] * n))
    words = (ctypes.c_uint64 * 2)(2**64 - 1, 2**64 - 1)
    assert lib.cess_ed25519_verify_batch(ctx.handle, n, a_idx, S, so, M, mo, codes, None) == 0
    assert list(codes) == want
    assert lib.cess_ed25519_verify_batch(ctx.handle, n, a_idx, S, so, M, mo, None, words) == 0
    assert list(words) == bitmap_of(want)
    assert lib.cess_ed25519_verify_batch(ctx.handle, n, a_idx, S, so, M, mo, None, None) == 0
    # n = 0: OK, nothing touched, whatever the pointers
    codes[0], words[0] = 0xEE, 0x1234
    assert lib.cess_ed25519_verify_batch(ctx.handle, 0, None, None, None, None, None, codes, words) == 0
    assert codes[0] == 0xEE and words[0] == 0x1234
    assert lib.cess_ed25519_verify_batch_device(ctx.handle, 0, None, None, None, None, None, None, None) == 0
    assert ctx.ed25519_verify_batch([], [], []) == b""
    with pytest.raises(bls.BlsInfraError) as ei:
        ctx.ed25519_keys_load(keys, policy=1)
    assert ei.value.status == bls.E_INVALID_ARG
    with pytest.raises(bls.BlsInfraError) as ei:
        ctx.verify_ed25519(*ring[0], policy=2)
    assert ei.value.status == bls.E_INVALID_ARG


@pytest.mark.gpu
def test_gpu_codes_in_neighbouring_lanes(ctx, ring, edges):
    """64 records whose lanes carry OK, SIG_LEN, SIG_RANGE, KEY (index outside the table), KEY (a key that
    did not load) and MISMATCH in rotation."""
    from cess_amd import bls
    bad_key = next(k for _, k, loads in edges["keys"] if not loads and len(k) == 32)
    good = [r[0] for r in ring[:8]]
    assert ctx.ed25519_keys_load(good + [bad_key]) == [0] * 8 + [bls.E_BAD_KEY]
    idx, msgs, sigs, want = [], [], [], []
    for i in range(64):
        k, m, s = ring[i % 8]
        kind = i % 6
        over = (L + 5).to_bytes(32, "little")
        idx.append(9 + i if kind == 3 else 8 if kind == 4 else i % 8)
        msgs.append(m)
        sigs.append(s[:63] if kind == 1 else s[:32] + over if kind == 2 else tamper(s) if kind == 5 else s)
        want.append((OK, SIG_LEN, SIG_RANGE, KEY, KEY, MISMATCH)[kind])
    codes, words = ctx.ed25519_verify_batch(idx, msgs, sigs, with_bitmap=True)
    assert list(codes) == want and words == bitmap_of(want)
    # precedence: a missing key before the signature's length, the length before an undecodable key
    assert list(ctx.ed25519_verify_batch([99, 8, 8], [b"", b"", b""], [b"short", b"short", bytes(32) + over])) == \
        [KEY, SIG_LEN, SIG_RANGE]


@pytest.mark.gpu
def test_gpu_key_table(ctx, ring, edges):
    from cess_amd import bls
    # one key for all records: 40 messages signed by the model's signer
    seed = bytes(range(32))
    pub = model.public_key(seed)
    msgs = [bytes([i]) * (i % 7) for i in range(40)]
    sigs = [model.sign(seed, m) for m in msgs]
    sigs[17] = tamper(sigs[17])
    assert ctx.ed25519_keys_load([pub]) == [0]
    want = [MISMATCH if i == 17 else OK for i in range(40)]
    assert list(ctx.ed25519_verify_batch([0] * 40, msgs, sigs)) == want
    # 300 distinct keys, and indices at and past the table's end
    recs = ring[:300]
    keys, idx, m2, s2 = table_of(recs)
    assert len(keys) == 300 and ctx.ed25519_keys_load(keys) == [0] * 300
    got = ctx.ed25519_verify_batch(idx + [300, 0xFFFFFFFF], m2 + [b"x", b"y"], s2 + [s2[0], s2[1]])
    assert list(got) == [OK] * 300 + [KEY, KEY]
    # bad keys between good ones; the second load replaced the first
    bad = [k for _, k, loads in edges["keys"] if not loads]
    mixed = [keys[0], bad[0], keys[1], bad[-1], keys[2]]
    assert ctx.ed25519_keys_load(mixed) == [0, bls.E_BAD_KEY, 0, bls.E_BAD_KEY, 0]
    got = ctx.ed25519_verify_batch([0, 1, 2, 3, 4, 5], m2[:5] + [m2[0]], s2[:5] + [s2[0]])
    assert list(got) == [OK, KEY, MISMATCH, KEY, MISMATCH, KEY]
    assert list(ctx.ed25519_verify_batch([0, 2, 4], m2[:3], s2[:3])) == [OK, OK, OK]
    # the BLS and RSA sides of the same context still work
    v = _load("vectors.json")["cases"]
    case = next(c for c in v if c["code"] == 0 and len(c["sig"]) == 96)
    assert list(ctx.verify_codes([tuple(bytes.fromhex(case[k]) for k in ("sig", "msg", "pk"))])) == [0]
    row = next(r for r in _load("ring_rsa_pkcs1_sha256.json")["rows"] if r["code"] == 0 and r["key_status"] == "ok")
    assert ctx.verify_rsa_sha256(bytes.fromhex(row["key"]), bytes.fromhex(row["msg"]), bytes.fromhex(row["sig"]),
                                 bls.RSA_KEY_PKCS1) is True
    assert list(ctx.ed25519_verify_batch([0, 2, 4], m2[:3], s2[:3])) == [OK, OK, OK]


@pytest.mark.gpu
def test_gpu_two_device_context(ctx, ring, edges):
    from cess_amd import bls
    recs, want = cycled(ring, 192)
    recs += [r[2:5] for r in edges["rows"] if r[1] in ("range", "length")]      # 5 + 3 rows: codes 0, 1, 2, 4
    want += [r[5] for r in edges["rows"] if r[1] in ("range", "length")]
    assert len(recs) == 200 and {OK, SIG_LEN, SIG_RANGE, MISMATCH} <= set(want)
    keys, idx, msgs, sigs = table_of(recs)
    assert ctx.ed25519_keys_load(keys) == [0] * len(keys)
    one = ctx.ed25519_verify_batch(idx, msgs, sigs, with_bitmap=True)
    m = bls.Context(max_batch=1024, devices=[0, 0])
    try:
        assert m.ed25519_keys_load(keys) == [0] * len(keys)
        two = m.ed25519_verify_batch(idx, msgs, sigs, with_bitmap=True)
        assert m.verify_ed25519(*ring[0]) is True
    finally:
        m.close()
    assert list(one[0]) == want and one[1] == bitmap_of(want)
    assert two == one


@pytest.mark.gpu
def test_gpu_profile_stages(ring):
    from cess_amd import bls
    recs, want = cycled(ring, 70)
    keys, idx, msgs, sigs = table_of(recs)
    c = bls.Context(max_batch=1024, profile=True)
    try:
        before = c.stage_stats(reset=True)
        c.ed25519_stage_stats(reset=True)
        c.ed25519_keys_load(keys)
        st = c.ed25519_stage_stats(reset=True)
        assert list(st) == ["k_ed25519_keys", "k_ed25519_pack", "k_ed25519_verify"]
        assert st["k_ed25519_keys"][1] == 2 and st["k_ed25519_keys"][0] > 0        # the base point's table and the keys'
        assert st["k_ed25519_verify"][1] == 0
        assert list(c.ed25519_verify_batch(idx, msgs, sigs)) == want
        st = c.ed25519_stage_stats(reset=True)
        assert [st[k][1] for k in st] == [0, 1, 1] and st["k_ed25519_pack"][0] > 0 and st["k_ed25519_verify"][0] > 0
        legacy = c.stage_stats(reset=True)
        assert list(legacy) == list(before) and legacy["k_rsa_digest"][1] == 1
        assert c.ed25519_stage_stats(reset=True)["k_ed25519_verify"] == (0.0, 0)
    finally:
        c.close()
