"""ECDSA P-256 under ring's rules (include/cess_ecdsa.h), without a GPU.

The plain-Python model (tests/ecdsa_model.py) against the two fixtures;
cess_amd/csrc/p256.hpp and the kernels' lane steps built for the host
(tests/hostemu/ecdsa_emu.cpp, -DCESS_HOSTEMU, no sanitizer preload) over every
fixture row; the column bound of the header against the recorded maximum; the
same code as a stand-alone program under the address and undefined-behaviour
sanitizers (a child process; nothing is loaded into Python under a sanitizer);
the bindings.
"""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import tempfile

import pytest

import ecdsa_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def load_rows():
    ring = json.load(open(os.path.join(GOLDEN, "ring_ecdsa.json")))
    edges = json.load(open(os.path.join(GOLDEN, "ecdsa_edges.json")))
    rows = [("ring %d" % i, r["alg"], bytes.fromhex(r["key"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"])
            for i, r in enumerate(ring["verify"])]
    rows += [(r["name"], r["alg"], None if r["key"] is None else bytes.fromhex(r["key"]), bytes.fromhex(r["msg"]),
              bytes.fromhex(r["sig"]), r["code"]) for r in edges["rows"]]
    # valid records whose ladder doubles or cancels at a chosen addition (gen_ecdsa_ladder.py), and their twins
    ladder = json.load(open(os.path.join(GOLDEN, "ecdsa_ladder.json")))
    rows += [(r["name"], r["alg"], bytes.fromhex(r["key"]), bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"])
             for r in ladder["rows"]]
    return ring, edges, ladder, rows


RING, EDGES, LADDER, ROWS = load_rows()


def digest_of(alg, msg):
    return (hashlib.sha384 if alg == model.ALG_P256_SHA384_ASN1 else hashlib.sha256)(msg).digest()


def emu_lib():
    src = os.path.join(ROOT, "tests", "hostemu", "ecdsa_emu.cpp")
    lib = os.path.join(ROOT, "tests", "hostemu", "libecdsa_emu.so")
    deps = [src, os.path.join(ROOT, "cess_amd", "csrc", "p256.hpp"), os.path.join(ROOT, "cess_amd", "csrc", "bls", "field.hpp"),
            os.path.join(ROOT, "tests", "probe", "ecdsa_probe.hip")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", src, "-o", lib])
    emu = ctypes.CDLL(lib)
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    emu.emu_ecdsa_record.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64,
                                     ctypes.c_char_p]
    emu.emu_ecp.argtypes = [ctypes.c_char_p, ctypes.c_uint32, u8p, u32p, u32p, u32p, ctypes.c_uint32]
    emu.emu_ecdsa_col_max.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    emu.emu_ecdsa_col_bound.restype = ctypes.c_uint64
    return emu


@pytest.fixture(scope="module")
def emu():
    return emu_lib()


def col_max(emu, reset=False):
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    emu.emu_ecdsa_col_max(ctypes.byref(lo), ctypes.byref(hi), 1 if reset else 0)
    return (hi.value << 64) | lo.value


def test_fixture_shape():
    v = RING["verify"]
    assert [sum(1 for r in v if r["alg"] == a) for a in range(3)] == [13, 28, 17]
    assert {r["result"] for r in v} == {"P", "F"} and len(RING["keys"]) == 24 and len(RING["digest_scalar"]) == 8
    assert {r["code"] for r in EDGES["rows"]} == {0, 1, 2, 3, 4} and "model" in EDGES["judge"]
    for name in ("point_sum", "point_sum_mixed", "point_double", "point_mul"):
        assert RING[name]


def test_model_on_every_row():
    for name, alg, key, msg, sig, code in ROWS:
        assert model.verify_code(alg, key, msg, sig) == code, name
    for r in RING["verify"]:
        assert (r["code"] == model.OK) == (r["result"] == "P")
    for r in RING["keys"]:
        assert (model.key_point(bytes.fromhex(r["key"])) is not None) == (r["result"] == "P")
    for r in RING["digest_scalar"]:
        assert model.digest_to_scalar(bytes.fromhex(r["input"])) == int(r["output"], 16)


def test_hostemu_every_row_and_column_bound(emu):
    col_max(emu, reset=True)
    wrong = []
    for name, alg, key, msg, sig, code in ROWS:
        got = emu.emu_ecdsa_record(alg, key, 0 if key is None else len(key), sig, len(sig), digest_of(alg, msg))
        if got != code:
            wrong.append((name, got, code))
    assert not wrong, wrong[:10]
    # ring's key rows, through a record whose signature is well-formed
    for r in RING["keys"]:
        key = bytes.fromhex(r["key"])
        got = emu.emu_ecdsa_record(0, key, len(key), bytes(31) + b"\x01" + bytes(31) + b"\x01", 64, bytes(32))
        assert (got != model.KEY) == (r["result"] == "P")
    top = col_max(emu)
    assert 0 < top < emu.emu_ecdsa_col_bound() < 2 ** 64, (top, emu.emu_ecdsa_col_bound())


_san = []


def san_exe():
    if not _san:
        exe = os.path.join(tempfile.mkdtemp(prefix="ecdsa_san_"), "ecdsa_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-DCESS_HOSTEMU",
                               "-DECDSA_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "hostemu", "ecdsa_emu.cpp"), "-o", exe])
        _san.append(exe)
    return _san[0]


def test_under_sanitizers(tmp_path):
    """Every fixture row and the primitive tables through the stand-alone program under the sanitizers."""
    import ecdsa_probe_model as pm
    hx = lambda b: b.hex() if b else "-"   # noqa: E731
    recs, ops, outp = str(tmp_path / "records.txt"), str(tmp_path / "ops.txt"), str(tmp_path / "ops_out.txt")
    with open(recs, "w") as f:
        for name, alg, key, msg, sig, code in ROWS:
            f.write("%d %s %s %s %d\n" % (alg, "x" if key is None else hx(key), hx(sig), digest_of(alg, msg).hex(), code))
    tables = pm.tables()
    with open(ops, "w") as f:
        for op, rows in tables.items():
            if pm.OPS[op][2]:
                continue                      # (entries that read tables run in the record file above)
            for row in rows:
                f.write(op + " " + " ".join("%x" % w for w in row) + "\n")
        # the ladder on the program's two tables of G: u1 G + u2 G
        ladder = [(u, v) for u, v in zip(pm.RECODE_PATTERNS, reversed(pm.RECODE_PATTERNS))]
        for u, v in ladder:
            f.write("double_mul " + " ".join("%x" % w for w in [0, 1] + pm.words(u) + pm.words(v)) + "\n")
    r = subprocess.run([san_exe(), recs, ops, outp], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d records, 0 wrong" % len(ROWS) in r.stdout
    got = {}
    for line in open(outp):
        t = line.split()
        got.setdefault(t[0], []).append([int(x, 16) for x in t[1:]])
    for op, rows in tables.items():
        if not pm.OPS[op][2]:
            pm.check(op, rows, got[op])
    pm.check_mul([(0, u, v) for u, v in ladder], got["double_mul"], [model.mul((u + v) % model.N, model.G) for u, v in ladder])


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_ffi_and_python_agree():
    text = _strip(open(os.path.join(ROOT, "include", "cess_ecdsa.h")).read())
    h = {m.group(1): m.group(2).count(",") + 1
         for m in re.finditer(r"\b(cess_ecdsa_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text)}
    rust = open(os.path.join(ROOT, "utils", "verify-bls-signatures-gpu", "src", "ffi.rs")).read()
    r = {m.group(1): m.group(2).count(",") + 1
         for m in re.finditer(r"pub fn (cess_ecdsa_[a-z0-9_]+)\s*\(([^)]*)\)", rust)}
    assert r == h and len(h) == 5
    from cess_amd import bls
    assert sorted(bls.EXPORTS_ECDSA) == sorted(h)
    for name, val in (("ALG_P256_SHA256_FIXED", 0), ("ALG_P256_SHA256_ASN1", 1), ("ALG_P256_SHA384_ASN1", 2), ("OK", 0),
                      ("SIG_FORMAT", 1), ("SIG_RANGE", 2), ("KEY", 3), ("MISMATCH", 4)):
        assert re.search(r"CESS_ECDSA_%s\s*=?\s*%d\b" % (name, val), text), name
        assert getattr(bls, "ECDSA_" + name) == val
        assert re.search(r"CESS_ECDSA_%s: \w+ = %d;" % (name, val), rust), name


def test_library_exports_and_unknown_algorithm():
    import cess_amd
    from cess_amd import bls
    assert cess_amd.verify_ecdsa is bls.verify_ecdsa and cess_amd.ECDSA_MISMATCH == 4
    lib = bls.load_library()
    for s in bls.EXPORTS_ECDSA:
        assert hasattr(lib, s), s
    ok = ctypes.c_int(7)
    # an unknown algorithm id is refused before anything else is looked at (no device needed)
    for alg in (-1, 3, 99):
        assert lib.cess_ecdsa_verify_batch(None, alg, 0, None, None, None, None, None, None, None) == bls.E_INVALID_ARG
        assert lib.cess_ecdsa_verify_batch_device(None, alg, 0, None, None, None, None, None, None, None) == bls.E_INVALID_ARG
        assert lib.cess_ecdsa_verify(None, alg, None, 0, None, 0, None, 0, ctypes.byref(ok)) == bls.E_INVALID_ARG
