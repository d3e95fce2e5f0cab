"""The Ed25519 signer (include/cess_ed25519_sign.h) on the CPU.

cess_amd/csrc/ed25519_sign.hpp built for the host (tests/hostemu/ed25519_sign_emu.cpp, -DCESS_HOSTEMU, no
sanitizer preload) against ring's own vectors (tests/golden/ring_ed25519.json: seed -> pub, (seed, msg) ->
sig, byte for byte), the edge fixture (tests/golden/ed25519_sign_edges.json, generated from
tests/ed25519_model.py) and Python integers; the same code as a stand-alone program under the address and
undefined-behaviour sanitizers; the code-object notes of the new kernels; the Python and Rust declarations
against the header.
"""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import tempfile

import pytest

import ed25519_model as model
from test_rsa_sha2 import OBJDUMP, READELF, _kernel_note

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = model.P, model.L
LOADED, BAD_LEN, INCONSISTENT = range(3)            # ed25519::SIGNER_*
KERNELS = {"k_ed25519_comb": "_Z14k_ed25519_combPjPh",
           "k_ed25519_signers": "_Z17k_ed25519_signersmPKjPKmPKhS4_PjS5_S5_Ph",
           "k_ed25519_sign_pack": "_Z19k_ed25519_sign_packmPKjjPKhS2_S2_S2_PKmPhPm",
           "k_ed25519_sign_r": "_Z16k_ed25519_sign_rmPKjjPKhS0_S2_PjPh",
           "k_ed25519_sign_s": "_Z16k_ed25519_sign_smPKjjPKhS0_S2_S0_PhS3_"}
BITS = [26, 25] * 5
WEIGHT = [sum(BITS[:k]) for k in range(10)]
HEADER = os.path.join(ROOT, "include", "cess_ed25519_sign.h")


def _load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ring():
    """(seed, pub, msg, sig) of the 323 reference rows"""
    rows = _load("ring_ed25519.json")["rows"]
    assert len(rows) == 323
    return [tuple(bytes.fromhex(r[k]) for k in ("seed", "pub", "msg", "sig")) for r in rows]


@pytest.fixture(scope="module")
def edges():
    e = _load("ed25519_sign_edges.json")
    return {"rows": [(r["name"],) + tuple(bytes.fromhex(r[k]) for k in ("seed", "pub", "msg", "sig")) for r in e["rows"]],
            "scalars": [(int(s["k"], 16), bytes.fromhex(s["enc"])) for s in e["scalars"]],
            "muladd": [tuple(int(t[k], 16) for k in "kars") for t in e["muladd"]],
            "overflow_seed": bytes.fromhex(e["overflow_seed"])}


def clamped(seed):
    return model._clamp(hashlib.sha512(seed).digest()[:32])


def words(v, n=8):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def unwords(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def _emu():
    src = os.path.join(ROOT, "tests", "hostemu", "ed25519_sign_emu.cpp")
    lib = os.path.join(ROOT, "tests", "hostemu", "libed25519_sign_emu.so")
    deps = [os.path.join(ROOT, "cess_amd", "csrc", h) for h in ("ed25519_sign.hpp", "ed25519.hpp", "rsa_digest512.hpp",
                                                                "rsa_digest.hpp", "bls/field.hpp", "kernels.hpp")]
    deps.append(os.path.join(ROOT, "tests", "probe", "ed25519_sign_probe.hip"))   # its lane functions (emu_edsp)
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in [src] + deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", src, "-o", lib])
    emu = ctypes.CDLL(lib)
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    emu.emu_eds_comb.argtypes = [u32p]
    emu.emu_eds_comb.restype = None
    emu.emu_eds_signer.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    emu.emu_eds_sign.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    emu.emu_eds_col_max.argtypes = [u64p, u64p, ctypes.c_int]
    emu.emu_eds_col_max.restype = None
    emu.emu_edsp.argtypes = [ctypes.c_char_p, ctypes.c_uint32, u32p, u32p]
    return emu


@pytest.fixture(scope="module")
def emu():
    return _emu()


def signer(emu, seed, expected=None):
    pub, a = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    st = emu.emu_eds_signer(seed, len(seed), expected, pub, a)
    return st, pub.raw, int.from_bytes(a.raw, "little")


def sign(emu, seed, msg):
    sig = ctypes.create_string_buffer(64)
    return emu.emu_eds_sign(seed, len(seed), msg, len(msg), sig), sig.raw


def probe(emu, name, rows, n_out=8):
    flat = [w for r in rows for w in r]
    out = (ctypes.c_uint32 * (n_out * len(rows)))()
    assert emu.emu_edsp(name.encode(), len(rows), (ctypes.c_uint32 * len(flat))(*flat), out) == 0
    return [list(out[n_out * i:n_out * (i + 1)]) for i in range(len(rows))]


# --- the fixtures themselves ----------------------------------------------------
def test_fixture_shape(ring, edges):
    """The edge fixture holds what the tests rely on: the recode-overflow seed, both block edges of both hash
    inputs, the scalar and muladd tables; 45 of ring's seeds exceed the recode bound."""
    bound = 2**256 * 7 // 15
    assert sum(clamped(r[0]) >= bound for r in ring) == 45
    ov = edges["overflow_seed"]
    assert ov == (5775).to_bytes(32, "little") and clamped(ov) >> 240 == 0x7fff and clamped(ov) >= bound
    seeds = list(dict.fromkeys(r[1] for r in edges["rows"]))
    assert len(seeds) == 4 and ov in seeds and bytes(range(32)) in seeds and bytes(32) in seeds
    assert any(clamped(s) >> 240 == 0x4000 for s in seeds)
    lens = [0, 1, 47, 48, 63, 64, 65, 79, 80, 95, 96, 97, 111, 112, 127, 128, 129, 1023]
    for s in seeds:
        assert [len(r[3]) for r in edges["rows"] if r[1] == s] == lens
    ks = [k for k, _ in edges["scalars"]]
    assert {0, 1, 2, 7, 8, 9, 15, 16, int("7" * 63, 16), int("8" * 63, 16), int("f" * 62, 16), 2**252 - 1, 2**252,
            L - 2, L - 1} <= set(ks) and all(k < L for k in ks)
    assert all(2**(4 * i) in ks and 2**(4 * i) - 1 in ks for i in (1, 31, 32, 62))
    tr = edges["muladd"]
    assert (L - 1, 2**255 - 8, L - 1) in [t[:3] for t in tr]
    assert any(t[0] == 0 and t[2] for t in tr) and any(t[2] == 0 and t[0] for t in tr)
    assert any(t[1] == clamped(ov) % L for t in tr)
    assert all((k * a + r) % L == s for k, a, r, s in tr)
    for name, seed, pub, msg, sig in edges["rows"][::7]:
        assert model.public_key(seed) == pub and model.sign(seed, msg) == sig, name
        assert model.verify_code(pub, msg, sig) == model.OK


# --- ed25519_sign.hpp on the host ------------------------------------------------
def test_ring_rows_on_host(emu, ring):
    """ring's vectors: pub from seed and sig from (seed, msg), byte for byte; the stored scalar is a mod L."""
    for seed, pub, msg, sig in ring:
        st, got_pub, a = signer(emu, seed)
        assert st == LOADED and got_pub == pub, seed.hex()
        assert a == clamped(seed) % L
        assert sign(emu, seed, msg) == (0, sig), seed.hex()
    hi, lo = ctypes.c_uint64(), ctypes.c_uint64()
    emu.emu_eds_col_max(hi, lo, 0)
    assert hi.value == 0 and lo.value < int(2**62.4)        # the column-sum bound of ed25519.hpp's header


def test_edges_on_host(emu, edges):
    for name, seed, pub, msg, sig in edges["rows"]:
        st, got_pub, _ = signer(emu, seed, pub)
        assert st == LOADED and got_pub == pub, name
        assert sign(emu, seed, msg) == (0, sig), name
    hi, lo = ctypes.c_uint64(), ctypes.c_uint64()
    emu.emu_eds_col_max(hi, lo, 0)
    assert hi.value == 0 and lo.value < int(2**62.4)


def test_expected_pubs_on_host(emu, ring):
    seed, pub = ring[0][0], ring[0][1]
    assert signer(emu, seed, pub)[:2] == (LOADED, pub)
    flipped = bytes([pub[0] ^ 1]) + pub[1:]
    st, got, a = signer(emu, seed, flipped)
    assert (st, got, a) == (INCONSISTENT, pub, 0)
    top = pub[:31] + bytes([pub[31] ^ 0x80])
    assert signer(emu, seed, top)[0] == INCONSISTENT
    st, got, a = signer(emu, seed[:31], pub)
    assert (st, got, a) == (BAD_LEN, bytes(32), 0)
    assert signer(emu, seed + b"\0")[0] == BAD_LEN and signer(emu, b"")[0] == BAD_LEN
    # a signer that did not load signs nothing: code 1 and 64 zero bytes
    assert sign(emu, seed[:31], b"msg") == (1, bytes(64))


def test_probe_tables_on_host(emu, edges):
    """The probe's lane functions (the GPU probe's own) on the fixture's tables against Python integers."""
    ks = [k for k, _ in edges["scalars"]]
    got = probe(emu, "ge_scalarmult_base", [words(k) for k in ks])
    assert [unwords(g).to_bytes(32, "little") for g in got] == [e for _, e in edges["scalars"]]
    assert got[0] == words(1)                                   # [0]B: the identity, y = 1
    tr = edges["muladd"]
    got = probe(emu, "sc_muladd", [words(k) + words(a) + words(r) for k, a, r, _ in tr])
    assert [unwords(g) for g in got] == [s for _, _, _, s in tr]
    hs = [int.from_bytes(hashlib.sha512(bytes([i])).digest()[:32], "little") for i in range(32)] + [0, 2**256 - 1]
    got = probe(emu, "clamp", [words(h) for h in hs])
    assert [unwords(g) for g in got] == [model._clamp(h.to_bytes(32, "little")) for h in hs]
    vals = hs + [L - 1, L, L + 1, 2**255 - 8, 2 * L, 15 * L + 3]
    got = probe(emu, "sc_reduce256", [words(v) for v in vals])
    assert [unwords(g) for g in got] == [v % L for v in vals]
    # a scalar that is not below L is refused, not recoded
    out = (ctypes.c_uint32 * 8)()
    assert emu.emu_edsp(b"ge_scalarmult_base", 1, (ctypes.c_uint32 * 8)(*words(L)), out) == 1
    assert emu.emu_edsp(b"nothing", 1, (ctypes.c_uint32 * 8)(), out) == 2


def value_of(limbs):
    return sum(int(x) << w for x, w in zip(limbs, WEIGHT))


def comb_rows_expected():
    """(y + x, y - x, 2 d x y) of j * 16^i * B, i = 0..63, j = 1..8"""
    out, base = [], model.B
    for _ in range(64):
        q, row = (0, 1), []
        for _ in range(8):
            q = model.add(q, base)
            row.append(((q[1] + q[0]) % P, (q[1] - q[0]) % P, 2 * model.D * q[0] * q[1] % P))
        out.append(row)
        for _ in range(4):
            base = model.add(base, base)
    return out


def check_comb(tab):
    want = comb_rows_expected()
    assert want[5][2][0] == sum(model.mul(3 * 16**5, model.B)) % P    # (the additions above are model.mul's points)
    for i in range(64):
        for j in range(8):
            e = [value_of(tab[240 * i + 30 * j + 10 * q:240 * i + 30 * j + 10 * q + 10]) % P for q in range(3)]
            assert tuple(e) == want[i][j], (i, j)
    tight = [2**26 + 2**12, 2**25 + 2**16] * 5
    assert all(tab[10 * q + k] <= tight[k] for q in range(64 * 24) for k in range(10))


def test_comb_table_on_host(emu):
    tab = (ctypes.c_uint32 * (64 * 240))()
    emu.emu_eds_comb(tab)
    check_comb(list(tab))


# --- the same code under the sanitizers ---------------------------------------------
SAN_ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def test_sign_under_sanitizers(tmp_path, ring, edges):
    """The emulator as a stand-alone program (its own main, run as a child process) built with the address and
    undefined-behaviour sanitizers, over ring's rows and the edges."""
    exe = os.path.join(tempfile.mkdtemp(prefix="ed25519_sign_san_"), "ed25519_sign_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-DCESS_HOSTEMU",
                           "-DED25519_SIGN_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostemu", "ed25519_sign_emu.cpp"), "-o", exe])
    hx = lambda b: b.hex() if b else "-"   # noqa: E731
    recs = str(tmp_path / "records.txt")
    rows = list(ring) + [r[1:] for r in edges["rows"]]
    with open(recs, "w") as f:
        for seed, pub, msg, sig in rows:
            f.write("%s %s %s %s\n" % (hx(seed), hx(msg), hx(pub), hx(sig)))
    r = subprocess.run([exe, recs], capture_output=True, text=True, timeout=900, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d records, 0 wrong" % len(rows) in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# --- the library's code objects, the bindings ------------------------------------------
@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="llvm tools not in this image")
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_code_object_notes(tmp_path, kernel):
    lib = os.path.join(ROOT, "cess_amd", "lib", "libcess_bls.so")
    if not os.path.exists(lib):
        pytest.skip("library not built (run __graft_entry__.build())")
    note = _kernel_note(tmp_path, lib, KERNELS[kernel])
    assert note is not None, kernel + " is not in the library"
    assert note[".private_segment_fixed_size"] == 0 and note[".vgpr_spill_count"] == 0
    if kernel == "k_ed25519_sign_r":
        assert note[".vgpr_count"] <= 256 and note[".max_flat_workgroup_size"] == 256


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _header_functions(path, prefix):
    text = _strip(open(path).read())
    return {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
            for m in re.finditer(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text)}


def _rust_functions(path, prefix):
    out = {}
    for m in re.finditer(r"pub fn (" + prefix + r"[a-z0-9_]+)\s*\((.*?)\)\s*(?:->[^;]*)?;", open(path).read(), flags=re.S):
        args = m.group(2).strip().rstrip(",")
        out[m.group(1)] = 0 if not args else args.count(",") + 1
    return out


def test_bindings_follow_the_header():
    from cess_amd import bls
    h = _header_functions(HEADER, "cess_ed25519_")
    assert h == {"cess_ed25519_signers_load": 7, "cess_ed25519_sign_batch": 7, "cess_ed25519_sign_batch_device": 8,
                 "cess_ed25519_sign": 7, "cess_ed25519_sign_stage_stats": 6}
    assert sorted(bls.EXPORTS_ED25519_SIGN) == sorted(h)
    lib = bls.load_library()
    for s in h:
        assert hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == h[s], s
    src = os.path.join(ROOT, "utils", "verify-bls-signatures-gpu", "src")
    assert _rust_functions(os.path.join(src, "ed25519_sign.rs"), "cess_ed25519_") == h
    assert "mod ed25519_sign;" in open(os.path.join(src, "lib.rs")).read()
    # the three existing lists are as they were: the verifier's header, its Rust declarations, its Python list
    v = _header_functions(os.path.join(ROOT, "include", "cess_ed25519.h"), "cess_ed25519_")
    assert sorted(v) == sorted(bls.EXPORTS_ED25519) == ["cess_ed25519_keys_load", "cess_ed25519_stage_stats",
                                                       "cess_ed25519_verify", "cess_ed25519_verify_batch",
                                                       "cess_ed25519_verify_batch_device"]
    assert _rust_functions(os.path.join(src, "ffi.rs"), "cess_ed25519_") == v
    assert not set(h) & set(bls.EXPORTS) and not set(h) & set(bls.EXPORTS_OTHER)


def test_constants_and_statuses():
    import cess_amd
    from cess_amd import bls
    text = _strip(open(HEADER).read())
    defs = dict((k, int(v)) for k, v in re.findall(r"#define (CESS_ED25519_[A-Z_]+) \(?(-?\d+)\)?", text))
    assert defs == {"CESS_ED25519_E_INCONSISTENT": bls.ED25519_E_INCONSISTENT, "CESS_ED25519_SIGN_OK": bls.ED25519_SIGN_OK,
                    "CESS_ED25519_SIGN_SIGNER": bls.ED25519_SIGN_SIGNER}
    # the next unused negative status: every other one is taken by cess_bls.h and cess_rsa.h
    used = set()
    for hname in ("cess_bls.h", "cess_rsa.h"):
        used |= {int(v) for v in re.findall(r"#define CESS_[A-Z]+_E_[A-Z_]+ \((-\d+)\)", open(os.path.join(ROOT, "include", hname)).read())}
    assert used == set(range(-11, 0)) and bls.ED25519_E_INCONSISTENT == -12
    lib = bls.load_library()
    assert b"inconsistent_components" in lib.cess_bls_status_string(-12)
    assert lib.cess_bls_status_string(-13) == b"unknown status"
    assert cess_amd.sign_ed25519 is bls.sign_ed25519 and cess_amd.Ed25519PrivateKey is bls.Ed25519PrivateKey
    assert cess_amd.ED25519_SIGN_SIGNER == 1
    with pytest.raises(bls.DeserializeError):
        bls.Ed25519PrivateKey.from_seed(bytes(31))
    assert repr(bls.Ed25519PrivateKey.from_seed(bytes(32))) == "Ed25519PrivateKey(REDACTED)"
    # no context: refused before anything else is looked at (no device needed)
    assert lib.cess_ed25519_signers_load(None, 0, None, None, None, None, None) == bls.E_INVALID_ARG
    assert lib.cess_ed25519_sign_batch(None, 0, None, None, None, None, None) == bls.E_INVALID_ARG
    assert lib.cess_ed25519_sign(None, None, 0, None, 0, None, None) == bls.E_INVALID_ARG
