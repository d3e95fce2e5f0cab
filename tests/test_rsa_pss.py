"""CPU: RSASSA-PSS under ring's RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512.

The plain-Python model (tests/rsa_pss_model.py) against both sets of ring rows and the edge fixture's
recorded codes; cess_amd/csrc/rsa_pss.hpp built for the host (tests/hostemu/rsa_pss_emu.cpp) against the
model on ring's padding rows, on every edge row (m by pow) and on random m with one byte changed at every
position; the one-record path (the 2048-bit class's exponentiation in store mode, then the EM check) on the
host; the sweep of tests/rsa_pss_sweep.py (every byte phase, top mask, separator position and salt-mask
offset, one changed bit at every byte position) through the same host build; the phase-key fixture against
the model and its keys of the compile-time class through the one-record path; the same rows once more in a
stand-alone program under the address and undefined-behaviour sanitizers; the code-object notes of the new
and the old kernels; the bindings."""
import ctypes
import glob
import hashlib
import os
import random
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rsa_probe_model as pm  # noqa: E402
import rsa_pss_model as model  # noqa: E402
import rsa_pss_sweep as sweep  # noqa: E402

CSRC = os.path.join(ROOT, "cess_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "hostemu", "rsa_pss_emu.cpp")
HDRS = [os.path.join(CSRC, h) for h in ("rsa_pss.hpp", "k_rsa.hpp", "rsa.hpp", "rsa_digest.hpp", "rsa_digest512.hpp",
                                        "bls/h2c.hpp")]
OK, SIG_LEN, SIG_RANGE, MSG_LEN, MISMATCH, KEY = range(6)
DIGESTS = ("SHA256", "SHA384", "SHA512")
L2048 = 74


@pytest.fixture(scope="module")
def ring():
    return model.load_fixture("ring_rsa_pss.json.gz")


@pytest.fixture(scope="module")
def edges():
    fx = model.load_fixture("rsa_pss_edges.json.gz")
    for k in fx["keys"]:
        k["n"], k["e"] = int(k["n"], 16), int(k["e"], 16)
    return fx


@pytest.fixture(scope="module")
def phase():
    fx = model.load_fixture("rsa_pss_phase_keys.json.gz")
    for k in fx["keys"]:
        k["n"], k["e"] = int(k["n"], 16), int(k["e"], 16)
    return fx


_lib = []


def emu():
    if not _lib:
        lib = os.path.join(ROOT, "tests", "hostemu", "librsa_pss_emu.so")
        if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", SRC, "-o", lib])
        e = ctypes.CDLL(lib)
        vp = ctypes.c_void_p
        e.emu_rsa_pss_em.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
        e.emu_rsa_pss_verify.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, vp, vp,
                                         ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
        _lib.append(e)
    return _lib[0]


def emu_em(name, bits, em, msg):
    return emu().emu_rsa_pss_em(model.DIGEST_ID[name], bits, em, len(em), model.HASH[name](msg).digest())


# --- the model ------------------------------------------------------------------------------------------
def test_model_against_ring_rows(ring):
    assert len(ring["verify"]) == 54 and len(ring["padding"]) == 105
    for r in ring["verify"]:
        status, ne = model.key_status(bytes.fromhex(r["key"]))
        assert status == r["key_status"] == "ok" and ne[0].bit_length() == 2048
        code = model.verify_code(r["digest"], ne[0], ne[1], bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]))
        assert code == r["code"] and (code == OK) == (r["result"] == "P"), r["comment"]
    for name in DIGESTS:
        rows = [r for r in ring["verify"] if r["digest"] == name]
        assert len(rows) == 18 and {r["code"] for r in rows} == {OK, MISMATCH}
    for r in ring["padding"]:
        code = model.em_code(r["digest"], bytes.fromhex(r["msg"]), bytes.fromhex(r["em"]), r["bits"])
        assert code == r["code"] and (code == OK) == (r["result"] == "P"), (r["digest"], r["bits"], r["result"])
    assert {r["bits"] for r in ring["padding"]} == {256, 512, 2048, 2049, 2055, 2056, 2057, 4095, 4096, 4097, 8191, 8192}
    assert sum("Invalid length" in r["result"] for r in ring["padding"]) == 2


def test_model_against_edge_fixture(edges):
    keys, table = edges["keys"], edges["table"]
    assert [model.key_status(bytes.fromhex(t["der"]))[0] for t in table] == [t["status"] for t in table]
    assert [t["status"] for t in table] == ["ok"] * len(keys) + ["bad_key"] * 3 + ["unsupported"]
    assert [k["bits"] for k in keys] == [2048, 2048, 2041, 2049, 2056, 2312, 3072, 4095, 4096, 4104, 3073]
    for k, t in zip(keys, table):
        assert model.ring_key(bytes.fromhex(t["der"])) == (k["n"], k["e"]) and k["n"].bit_length() == k["bits"]
    cases = {}
    for r in edges["rows"]:
        if r["key"] < len(keys):
            k = keys[r["key"]]
            code = model.verify_code(r["digest"], k["n"], k["e"], bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]))
        else:
            code = KEY
        assert code == r["code"], (r["digest"], r["case"])
        cases.setdefault(r["digest"], set()).add(r["case"])
    assert cases["SHA256"] == cases["SHA384"] == cases["SHA512"] and len(cases["SHA256"]) == 39
    # the salt-length restriction: RFC 8017 accepts these encodings, ring's rule 7 does not
    for r in edges["rows"]:
        if r["case"].startswith("salt_len_"):
            assert r["code"] == MISMATCH
    # db_len is a whole number of MGF1 blocks where the fixture says so
    assert (257 - 32 - 1) % 32 == 0 and (257 - 64 - 1) % 64 == 0 and (289 - 48 - 1) % 48 == 0


def test_model_against_phase_key_fixture(phase, edges):
    """the keys for the phases and class edges that the edge fixture's keys do not reach: sizes, classes, the
    model's code of every row, the cases per key, and d (to sign with) for the compile-time class alone"""
    keys, table = phase["keys"], phase["table"]
    assert [(k["name"], k["bits"]) for k in keys] == [("p2058", 2058), ("p2065", 2065), ("p2070", 2070), ("p3090", 3090),
                                                      ("p4112", 4112)]
    assert [model.key_status(bytes.fromhex(t["der"]))[0] for t in table] == [t["status"] for t in table] == ["ok"] * 5
    for k, t in zip(keys, table):
        assert model.ring_key(bytes.fromhex(t["der"])) == (k["n"], k["e"]) and k["n"].bit_length() == k["bits"]
        L = pm.size_class_limbs(k["bits"], (k["bits"] + 7) // 8)
        assert (L == L2048) == (k["bits"] <= 2070) == ("d" in k) and L
        if "d" in k:
            assert pow(pow(12345, int(k["d"], 16), k["n"]), k["e"], k["n"]) == 12345
    assert [((k["bits"] + 7) // 8, (k["bits"] + 6) // 8 & 3) for k in keys] == [(258, 2), (259, 2), (259, 3), (387, 3), (514, 2)]
    assert pm.size_class_limbs(2071, 259) > L2048 and pm.size_class_limbs(4113, 515) == 0
    assert not {k["bits"] for k in keys} & {k["bits"] for k in edges["keys"]}
    cases = {}
    for r in phase["rows"]:
        k = keys[r["key"]]
        code = model.verify_code(r["digest"], k["n"], k["e"], bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]))
        assert code == r["code"] and (code == OK) == (r["case"] == "valid"), (r["digest"], k["name"], r["case"])
        cases.setdefault((r["digest"], k["name"]), []).append(r["case"])
    core = ["valid", "above_em_bits", "ps_first", "sep_02", "salt_changed", "hprime_changed"]
    assert cases == {(d, k["name"]): core + (["leading_byte"] if k["name"] == "p2065" else []) for d in DIGESTS for k in keys}


def test_code_lists_beside_the_fixtures(ring, edges):
    """NAME.codes.txt, the text that shows each row's recorded code in a diff, is what the gzipped fixture holds"""
    for name in ("ring_rsa_pss.json.gz", "rsa_pss_edges.json.gz", "rsa_pss_phase_keys.json.gz"):
        with open(model.codes_path(name)) as f:
            assert f.read().splitlines() == model.code_lines(model.load_fixture(name)), name


# --- rsa_pss.hpp on the host ----------------------------------------------------------------------------
def test_header_on_ring_padding_rows(ring):
    n = 0
    for r in ring["padding"]:
        if r["bits"] <= 4096:
            got = emu_em(r["digest"], r["bits"], bytes.fromhex(r["em"]), bytes.fromhex(r["msg"]))
            assert got == r["code"], (r["digest"], r["bits"], r["result"])
            n += 1
    assert n == 80


def test_header_on_edge_rows(edges, phase):
    for fx in (edges, phase):
        seen = set()
        for r in fx["rows"]:
            if r["code"] not in (OK, MISMATCH):
                continue
            k = fx["keys"][r["key"]]
            m = pow(int(r["sig"], 16), k["e"], k["n"]).to_bytes((k["bits"] + 7) // 8, "big")
            assert emu_em(r["digest"], k["bits"], m, bytes.fromhex(r["msg"])) == r["code"], (r["digest"], k["name"], r["case"])
            seen.add((k["name"], r["code"]))
        assert all((k["name"], c) in seen for k in fx["keys"] for c in (OK, MISMATCH))


@pytest.mark.parametrize("name", DIGESTS)
def test_header_on_changed_bytes(name):
    """a valid encoding with one byte changed, at every position of the smallest size and at each position
    class of the others (leading byte, first and last byte of PS, separator, salt, H', trailer), for sizes
    of every byte phase and on both sides of the word and MGF1 block boundaries; other salt lengths"""
    rng = random.Random(0x454d)
    h = model.HASH[name]().digest_size
    small = 8 * (2 * h + 2)
    sizes = [small, small + 1, small + 8, 1024, 1030] + list(range(2041, 2060)) + [2312, 3072, 4095, 4096]
    for bits in (b for b in sizes if b >= small):             # (SHA-512 has no valid 1024-bit encoding)
        msg = bytes(rng.randrange(256) for _ in range(rng.randrange(64)))
        em = model.encode(name, msg, bytes(rng.randrange(256) for _ in range(h)), bits)
        k, em_len = (bits + 7) // 8, (bits + 6) // 8
        assert len(em) == k and emu_em(name, bits, em, msg) == OK, bits
        db_len = em_len - h - 1
        ps_len = db_len - h - 1
        o = k - em_len
        pos = {0, o, o + 1, o + ps_len - 1, o + ps_len, o + ps_len + 1, o + db_len - 1, o + db_len, k - 2, k - 1}
        pos |= set(range(k)) if bits <= small + 1 or bits == 2049 else {rng.randrange(k) for _ in range(24)}
        for p in sorted(x for x in pos if 0 <= x < k):
            em2 = bytearray(em)
            em2[p] ^= 1 << rng.randrange(8)
            want = model.em_code(name, msg, bytes(em2), bits)
            assert emu_em(name, bits, bytes(em2), msg) == want, (bits, p)
            em2[p] = em[p] ^ 0x80
            assert emu_em(name, bits, bytes(em2), msg) == model.em_code(name, msg, bytes(em2), bits), (bits, p)
        for sl in (0, 20, h - 1, h + 1):
            em3 = model.encode(name, msg, bytes(sl), bits) if em_len >= h + sl + 2 else None
            if em3 is not None and len(em3) == k:
                assert emu_em(name, bits, em3, msg) == MISMATCH, (bits, sl)
        assert emu_em(name, bits, em[1:], msg) == MISMATCH and emu_em(name, bits, b"\x00" + em, msg) == MISMATCH
    # too short for two digests: ring's PSSMetrics::new fails
    assert emu_em(name, small - 8, bytes(2 * h + 1), b"") == MISMATCH == model.em_code(name, b"", bytes(2 * h + 1), small - 8)


@pytest.mark.parametrize("name", DIGESTS)
def test_header_on_the_sweep(name):
    """every record of tests/rsa_pss_sweep.py: all 32 pairs (em_len & 3, em_bits & 7) at the smallest sizes, at
    2041..2072 and at 4081..4112 bits, ps_len 0..11, r in {1, 2, 3, 4, h - 1, h}, the sizes with no valid encoding;
    per size three valid encodings, one changed bit at every byte position, the edge fixture's crafted cases and
    the wrong lengths.  The code of each is the model's."""
    e, dg = emu(), model.DIGEST_ID[name]
    recs = sweep.sweep(name)
    bad = [sweep.where(r) + (got,) for r in recs
           for got in [e.emu_rsa_pss_em(dg, r[0], r[1], len(r[1]), r[2])] if got != (OK if r[3] else MISMATCH)]
    assert not bad, (len(bad), bad[:20])
    assert len(recs) > 30000 and sum(r[3] for r in recs) == 3 * sum(sweep.metrics(name, b)["valid"] for b in sweep.sizes(name))


# --- the one-record path on the host --------------------------------------------------------------------
def key_row(n):
    L = pm.size_class_limbs(n.bit_length(), (n.bit_length() + 7) // 8)
    return L, pm.limbs(n, L), pm.limbs(pow(2, 2 * 28 * L, n), L), pm.ninv_of(n)


def one_record_rows(ring, edges, phase):
    """(digest, n, e, msg, sig, code) of every fixture row of the 2048-bit size class that reaches a kernel"""
    out = []
    for r in ring["verify"]:
        n, e = model.ring_key(bytes.fromhex(r["key"]))
        out.append((r["digest"], n, e, bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"]))
    for fx in (edges, phase):
        for r in fx["rows"]:
            if r["key"] < len(fx["keys"]) and r["code"] != SIG_LEN:
                k = fx["keys"][r["key"]]
                if key_row(k["n"])[0] == L2048:
                    out.append((r["digest"], k["n"], k["e"], bytes.fromhex(r["msg"]), bytes.fromhex(r["sig"]), r["code"]))
    return out


def test_one_record_path_on_host(ring, edges, phase):
    """(with the phase keys: m of 65 words, a leading zero byte in word 64, the largest key of the class)"""
    e = emu()
    arr = lambda v: np.array(v, dtype=np.uint32)   # noqa: E731
    rows = one_record_rows(ring, edges, phase)
    rowcache = {}
    for name, n, ex, msg, sig, code in rows:
        if n not in rowcache:
            L, n28, r2, ninv = key_row(n)
            assert L == L2048
            rowcache[n] = (arr(n28), arr(r2), ninv)
        n28, r2, ninv = rowcache[n]
        got = e.emu_rsa_pss_verify(model.DIGEST_ID[name], n.bit_length(), (n.bit_length() + 7) // 8, ex,
                                   n28.ctypes.data_as(ctypes.c_void_p), r2.ctypes.data_as(ctypes.c_void_p), ninv, sig,
                                   model.HASH[name](msg).digest())
        assert got == code, (name, n.bit_length(), code, got)
    assert {n.bit_length() for _, n, *_ in rows} == {2041, 2048, 2049, 2056, 2058, 2065, 2070}
    assert {c for *_, c in rows} == {OK, SIG_RANGE, MISMATCH} and len(rows) > 150 + 57


def test_rows_under_sanitizers(tmp_path, ring, edges, phase):
    """rsa_pss_emu.cpp as a stand-alone program (its own main, run as a child process; the test preloads nothing)
    built with the address and undefined-behaviour sanitizers: ring's padding rows, the edge rows' m, the
    one-record rows (the phase keys' among them) and the sweep's records of the smallest valid size, 2058, 2070
    and 4112 bits once more"""
    exe = str(tmp_path / "rsa_pss_emu_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-omit-frame-pointer", "-DCESS_HOSTEMU", "-DRSA_PSS_EMU_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])

    def padded(b):
        return b + bytes(-len(b) % 4)

    blob, want = [], []
    for r in ring["padding"]:
        if r["bits"] <= 4096:
            em = bytes.fromhex(r["em"])
            mh = model.HASH[r["digest"]](bytes.fromhex(r["msg"])).digest()
            blob.append(struct.pack("<4I", 0, model.DIGEST_ID[r["digest"]], r["bits"], len(em)) + mh + bytes(64 - len(mh)) +
                        padded(em))
            want.append(r["code"])
    for r in edges["rows"]:
        if r["code"] in (OK, MISMATCH):
            k = edges["keys"][r["key"]]
            m = pow(int(r["sig"], 16), k["e"], k["n"]).to_bytes((k["bits"] + 7) // 8, "big")
            mh = model.HASH[r["digest"]](bytes.fromhex(r["msg"])).digest()
            blob.append(struct.pack("<4I", 0, model.DIGEST_ID[r["digest"]], k["bits"], len(m)) + mh + bytes(64 - len(mh)) +
                        padded(m))
            want.append(r["code"])
    for name in DIGESTS:
        for bits, em, mh, ok, _ in sweep.subset(name, (sweep.smallest(name), 2058, 2070, 4112)):
            blob.append(struct.pack("<4I", 0, model.DIGEST_ID[name], bits, len(em)) + mh + bytes(64 - len(mh)) + padded(em))
            want.append(OK if ok else MISMATCH)
    assert len(want) > 3 * 1100 and want.count(OK) > 3 * 12
    for name, n, ex, msg, sig, code in one_record_rows(ring, edges, phase):
        L, n28, r2, ninv = key_row(n)
        mh = model.HASH[name](msg).digest()
        blob.append(struct.pack("<4I", 1, model.DIGEST_ID[name], n.bit_length(), len(sig)) +
                    struct.pack("<3I", ex & 0xffffffff, ex >> 32, ninv) + np.array(n28 + r2, dtype="<u4").tobytes() +
                    mh + bytes(64 - len(mh)) + padded(sig))
        want.append(code)
    inp, outp = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "%d rows" % len(want) in r.stdout
    assert list(np.fromfile(outp, dtype="<u4")) == want


# --- code objects ----------------------------------------------------------------------------------------
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NOTE_KEYS = (".group_segment_fixed_size", ".max_flat_workgroup_size", ".private_segment_fixed_size", ".sgpr_count",
             ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count")
# the metadata notes of the kernels that were there before RSASSA-PSS, as their build before it gave them
# (group segment, workgroup size, private segment, SGPRs, spilled SGPRs, VGPRs, spilled VGPRs)
BEFORE = {
    "_Z17k_rsa_verify_1024jPKjS0_S0_PK9RsaKeyDevPKhPKmS5_S7_PjPh": (0, 256, 0, 24, 0, 238, 0),
    "_Z17k_rsa_verify_2048jPKjS0_S0_PK9RsaKeyDevPKhPKmS5_S7_PjPh": (0, 256, 2220, 22, 0, 256, 1263),
    "_Z18k_rsa_verify_2048ujPKjS0_S0_PK9RsaKeyDevPKhPKmS5_S7_PjPh": (0, 256, 880, 106, 108, 256, 374),
    "_Z16k_rsa_verify_bigjPKjS0_S0_PK9RsaKeyDevPKhPKmS5_S7_Ph": (0, 256, 1872, 42, 0, 150, 0),
    "_Z14k_rsa_classifymPKjjPK9RsaKeyDevPKhPKmS7_PhPjS9_": (0, 256, 0, 29, 0, 12, 0),
    "_Z12k_rsa_digestmPKhPKmPhjPm": (16640, 64, 0, 106, 0, 115, 0),
    "_Z15k_rsa_digest512mPKhPKmPhjPmi": (16640, 64, 0, 97, 0, 138, 0),
}
STORE_OF = {"_Z18k_rsa_verify_2048mjPKjS0_S0_PK9RsaKeyDevPKhPKmPjPhS8_": "_Z17k_rsa_verify_2048jPKjS0_S0_PK9RsaKeyDevPKhPKmS5_S7_PjPh",
            "_Z19k_rsa_verify_2048umjPKjS0_S0_PK9RsaKeyDevPKhPKmPjPhS8_": "_Z18k_rsa_verify_2048ujPKjS0_S0_PK9RsaKeyDevPKhPKmS5_S7_PjPh",
            "_Z17k_rsa_verify_bigmjPKjS0_S0_PK9RsaKeyDevPKhPKmPhPj": "_Z16k_rsa_verify_bigjPKjS0_S0_PK9RsaKeyDevPKhPKmS5_S7_Ph"}
PSS_KERNELS = ["_Z16k_rsa_pss_%sjPKjS0_S0_PK9RsaKeyDevS0_S0_S0_Ph" % d for d in ("sha256", "sha384", "sha512")]


def kernel_notes(tmp_path, lib):
    """{kernel symbol: NOTE_KEYS values} of the library's gfx950 code objects (read as
    tests/test_rsa_sha2.py::_kernel_note reads them: an entry ends at its .wavefront_size)"""
    copy = str(tmp_path / "libcess_bls.so")
    shutil.copy(lib, copy)
    subprocess.check_call([OBJDUMP, "--offloading", copy], cwd=tmp_path, stdout=subprocess.DEVNULL)
    out = {}
    for obj in glob.glob(str(tmp_path / "libcess_bls.so.*gfx950")):
        notes = subprocess.run([READELF, "--notes", obj], capture_output=True, text=True, check=True).stdout
        cur, sym = {}, None
        for line in notes.splitlines():
            key, _, val = line.strip().lstrip("- ").strip().partition(":")
            val = val.strip()
            if key == ".symbol":
                sym = val[:-3] if val.endswith(".kd") else val
            elif key == ".wavefront_size":
                if sym:
                    out[sym] = tuple(cur.get(k) for k in NOTE_KEYS)
                cur, sym = {}, None
            elif key in NOTE_KEYS:
                cur[key] = int(val)
    return out


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="llvm tools not in this image")
def test_code_object_notes(tmp_path):
    lib = os.path.join(ROOT, "cess_amd", "lib", "libcess_bls.so")
    if not os.path.exists(lib):
        pytest.skip("library not built (run __graft_entry__.build())")
    notes = kernel_notes(tmp_path, lib)
    for k in PSS_KERNELS:                                   # no scratch, no spills
        assert k in notes, k
        lds, wg, priv, sgpr, sspill, vgpr, vspill = notes[k]
        assert (lds, wg, priv, sspill, vspill) == (0, 256, 0, 0, 0), (k, notes[k])
        assert vgpr <= 168                                  # three waves per SIMD at least
    assert notes[PSS_KERNELS[0]][5] <= 128                  # SHA-256: four
    for new, old in STORE_OF.items():                       # store mode: no more scratch than the original
        assert new in notes, new
        assert notes[new][2] <= notes[old][2] and notes[new][1] == notes[old][1], (new, notes[new], notes[old])
    for k, want in BEFORE.items():                          # the originals as they were
        assert notes.get(k) == want, (k, notes.get(k))


# --- bindings --------------------------------------------------------------------------------------------
def test_header_declares_and_bindings_list_the_entries():
    from cess_amd import bls
    with open(os.path.join(ROOT, "include", "cess_rsa.h")) as f:
        txt = f.read()
    for sym, nargs in (("cess_rsa_verify_pss_batch", 10), ("cess_rsa_verify_pss_batch_device", 10),
                       ("cess_rsa_verify_pss", 10), ("cess_rsa_pss_em_batch", 8), ("cess_rsa_pss_stage_stats", 6)):
        assert sym in bls.EXPORTS
        decl = txt[txt.index("int " + sym + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs, sym
    assert "CESS_RSA_ALG_3072_8192_SHA384 3" in txt and "CESS_RSA_DIGEST_SHA512 2" in txt
    assert hashlib.sha256(b"").digest_size == 32
    for name in ("rsa_verify_pss_batch", "rsa_verify_pss_batch_device", "verify_rsa_pss", "rsa_pss_em_batch"):
        assert callable(getattr(bls.Context, name))


def test_bindings_argument_counts_and_unknown_digest():
    from cess_amd import bls
    lib = bls.load_library()
    for sym, nargs in (("cess_rsa_verify_pss_batch", 10), ("cess_rsa_verify_pss_batch_device", 10),
                       ("cess_rsa_verify_pss", 10), ("cess_rsa_pss_em_batch", 8), ("cess_rsa_pss_stage_stats", 6)):
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    try:
        c = bls.Context(max_batch=64)
    except bls.DeviceUnavailable:
        pytest.skip("no device: the entries need a context")
    try:
        for dg in (3, -1):
            with pytest.raises(bls.BlsInfraError) as ei:
                c.rsa_verify_pss_batch(dg, [0], [b"m"], [bytes(256)])
            assert ei.value.status == bls.E_INVALID_ARG
    finally:
        c.close()
