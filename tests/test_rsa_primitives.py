"""CPU: the RSA kernels' Montgomery arithmetic alone, on the host build of
cess_amd/csrc/k_rsa.hpp, rsa_mont.hpp and k_rsa_big.hip
(tests/hostemu/rsa_emu.cpp and rsa_big_emu.cpp, -DCESS_HOSTEMU), against the
integer model of tests/rsa_probe_model.py.

The end-to-end RSA tests use products of two random primes and e = 3 / 65537:
after the first squaring every intermediate is a uniform residue.  Here
mont<37|74, false|true> (out aliasing a), canon, to_words and mont_rt at
L = 80, 88 and 152 run on all-ones, mostly-zero, single-limb and
every-top-fill moduli, with operands at the ends of [0, 2n), and the one-record
verifier of every class runs on keys made of Mersenne primes
(tests/rsa_structured_keys.py) with e = 2, 65537, 2^32 + 1 and 0x1fffffffd.

The host build shadows the 64-bit column accumulators in 128 bits and records
their maximum (see test_column_maxima)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import rsa_probe_model as pm
import rsa_structured_keys as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rsa_big_emu.cpp: k_rsa_big.hip itself, a translation unit of its own
SRCS = [os.path.join(ROOT, "tests", "hostemu", f) for f in ("rsa_emu.cpp", "rsa_big_emu.cpp")]
HDRS = [os.path.join(ROOT, "cess_amd", "csrc", h) for h in ("k_rsa.hpp", "rsa_mont.hpp", "rsa.hpp", "kernels.hpp",
                                                            "k_rsa_big.hip")]
OP_MUL, OP_SQR, OP_CANON, OP_WORDS, OP_MONT_RT, OP_VERIFY = range(6)
KIND_OP = {"mul": OP_MUL, "sqr": OP_SQR, "canon": OP_CANON, "words": OP_WORDS}

_lib = []


def emu():
    if not _lib:
        lib = os.path.join(ROOT, "tests", "hostemu", "librsa_emu.so")
        if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in SRCS + HDRS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC"] + SRCS + ["-o", lib])
        e = ctypes.CDLL(lib)
        vp = ctypes.c_void_p
        e.emu_rsa_rows.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp]
        e.emu_rsa_verify.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, vp, vp, ctypes.c_uint32,
                                     ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        e.emu_rsa_col_max.argtypes = [ctypes.c_int, u64p, u64p, ctypes.c_int]
        _lib.append(e)
    return _lib[0]


def col_max(which, reset=False):
    hi, lo = ctypes.c_uint64(), ctypes.c_uint64()
    emu().emu_rsa_col_max(which, ctypes.byref(hi), ctypes.byref(lo), int(reset))
    return hi.value << 64 | lo.value


def pack(c, rows):
    """(n, ninv, a, b) as uint32 arrays of the rows' limbs"""
    lim = lambda vs: np.array([pm.limbs(v, c.L) for v in vs], dtype=np.uint32).reshape(len(rows), c.L)   # noqa: E731
    return (lim([r.n for r in rows]), np.array([pm.ninv_of(r.n) for r in rows], dtype=np.uint32),
            lim([r.a for r in rows]), lim([r.b for r in rows]))


def units():
    """(class, kind, op of rsa_emu.cpp) of every table the host build runs:
    the loop form takes its products (a = b included) through mont_rt"""
    for c in pm.CLASSES:
        for kind in ("mul", "sqr") if c.loop else ("mul", "sqr", "canon", "words"):
            yield c, kind, OP_MONT_RT if c.loop else KIND_OP[kind]


def n_out(c, op):
    return (28 * c.L + 31) // 32 if op == OP_WORDS else c.L + 1 if op == OP_MONT_RT else c.L


def check_rows(c, kind, rows, out):
    for r, w in zip(rows, out):
        if kind in ("mul", "sqr"):
            pm.check_mont(c, r, w, kind)
        elif kind == "canon":
            pm.check_canon(c, r, w)
        else:
            pm.check_words(c, r, w)


def run_host(c, kind, op, rows):
    n, ninv, a, b = pack(c, rows)
    out = np.full((len(rows), n_out(c, op)), pm.POISON, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert emu().emu_rsa_rows(op, c.L, len(rows), p(n), p(ninv), p(a), p(b), p(out)) == 0
    return out


# --- the model's own checks ------------------------------------------------------
@pytest.mark.parametrize("c", pm.CLASSES, ids=lambda c: c.name)
def test_model_tables_hold_every_edge(c):
    """the tables cannot silently lose an edge: per class an all-ones modulus,
    a result >= n before canon, both extremes of ninv, an operand 2n - 1, every
    fill of the top limb and single-limb moduli; every modulus is one the host
    sends to the class (or a smaller one) and every operand is below 2n"""
    rows = pm.table(c, "mul")
    mods = dict(pm.moduli(c))
    assert mods["all_ones"] == (1 << c.max_bits) - 1 and c.holds(mods["all_ones"])
    assert not c.holds_bits(c.max_bits + 1) or c.max_bits == pm.MAX_BITS
    assert all(w == pm.M28 for w in pm.limbs(mods["all_ones"], c.L)[:c.max_bits // 28])
    assert {1, pm.M28} <= {pm.ninv_of(n) for n in mods.values()}
    assert pm.ninv_of(mods["all_ones"]) == 1 and pm.ninv_of(mods["top_and_one"]) == pm.M28
    assert {n.bit_length() % 28 for t, n in mods.items() if t.startswith("top_fill")} == set(range(28))
    assert {3, pm.M28, pm.M28 + 2} <= set(mods.values())
    assert any(pm.limbs(n, c.L)[1:c.L // 2] == [0] * (c.L // 2 - 1) for n in mods.values())      # a long run of zero limbs
    for n in mods.values():
        assert n & 1 and c.holds(n) and 4 * n <= c.R
        assert {r.a for r in rows if r.n == n} >= {0, 1, 2, n - 1, n, n + 1, 2 * n - 1, c.R % n, c.R * c.R % n}
        assert any(r.a == 2 * n - 1 and r.b == 2 * n - 1 for r in rows if r.n == n)
    for kind in ("mul", "sqr", "canon"):
        assert all(0 <= r.a < 2 * r.n and 0 <= r.b < 2 * r.n for r in pm.table(c, kind))
    assert all(r.a == r.b for r in pm.table(c, "sqr"))
    pairs = {(r.n, r.a, r.b) for r in rows}
    assert all((n, b, a) in pairs for n, a, b in pairs)                   # both operand orders
    assert any(r.a >= r.n for r in pm.table(c, "canon")) and any(r.a == 2 * r.n - 1 for r in pm.table(c, "canon"))
    # a Montgomery result that canon has to reduce exists in the model itself:
    # the least representative below 2n of a residue is not always below n
    assert any((r.a * r.b + (-r.a * r.b * pow(r.n, -1, c.R) % c.R) * r.n) // c.R >= r.n for r in rows)


def test_model_names_the_host_classes():
    assert [c.L for c in pm.CLASSES] == [37, 74, 80, 88, 152]
    assert pm.size_class_limbs(1032, 129) == 37 and pm.size_class_limbs(1033, 130) == 74
    assert pm.size_class_limbs(2070, 259) == 74 and pm.size_class_limbs(2071, 259) == 80      # the smallest loop-form size
    assert pm.size_class_limbs(2233, 280) == 88 and pm.size_class_limbs(4096, 512) == 152
    for c in pm.CLASSES:
        k = (c.max_bits + 7) // 8
        assert pm.size_class_limbs(c.max_bits, k) == c.L


# --- every table row through the host build -----------------------------------------
@pytest.mark.parametrize("unit", list(units()), ids=lambda u: "%s-%s" % (u[0].name, u[1]))
def test_rows_on_host(unit):
    """residue, range and limb bounds of every row; for the products also that
    some result came back in [n, 2n) (canon has work to do)"""
    c, kind, op = unit
    rows = pm.table(c, kind)
    out = run_host(c, kind, op, rows)
    check_rows(c, kind, rows, out)
    if kind == "mul":
        assert any(pm.from_limbs(w) >= r.n for r, w in zip(rows, out))


def expanded_bound(L):
    """2L products below (2^28 - 1)^2 and the carry of a column that large"""
    b = 2 * L * pm.M28 * pm.M28
    return b + (b >> 28) + 1


def test_column_maxima():
    """The 64-bit column values, shadowed in 128 bits by the host build, over
    every table row.

    Expanded form (k_rsa.hpp mont<L, SQR>): must stay below 2^64; the derived
    bound is 2L (2^28 - 1)^2 plus the carry, and the all-ones rows must come
    within a factor of 2 of it (else the table misses the edge it claims).
    Measured: L = 37: 0x2f45b655e0000000 (2^61.56, bound 2^62.21);
    L = 74: 0x5f94903c50000000 (2^62.58, bound 2^63.21).

    Loop form (rsa_mont.hpp mont_rt): k_rsa_big.hip promises u <= 2^58; one u
    is in + a_i b_j + m_i n_j + c <= (2^28 - 1) + 2 (2^28 - 1)^2 + c with
    c = u >> 28 < 2^30.  Measured: 0x1ffffffe0000001 (2^57.00) at L = 80 and 88,
    0x1ffffffdfffffff at L = 152."""
    for c in pm.CLASSES:
        col_max(int(c.loop), reset=True)
        ones = (1 << c.max_bits) - 1
        for kind in ("mul", "sqr"):
            rows = [r for r in pm.table(c, kind) if r.n == ones]
            run_host(c, kind, OP_MONT_RT if c.loop else KIND_OP[kind], rows)
        edge = col_max(int(c.loop), reset=True)
        for cc, kind, op in units():
            if cc is c:
                run_host(c, kind, op, pm.table(c, kind))
        top = max(edge, col_max(int(c.loop), reset=True))
        print("%s: column maximum %#x (2^%.3f), all-ones rows %#x" % (c.name, top, np.log2(float(top)), edge))
        if c.loop:
            assert top <= 1 << 58
            assert top <= pm.M28 + 2 * pm.M28 * pm.M28 + (1 << 30)
            assert 2 * edge >= pm.M28 + 2 * pm.M28 * pm.M28
        else:
            assert top < 1 << 64
            assert top <= expanded_bound(c.L) < 1 << 64
            assert 2 * edge >= expanded_bound(c.L)


# --- structured keys through the one-record verifier ---------------------------------
@pytest.fixture(scope="module")
def structured():
    return sk.structured()


def test_structured_oracle_against_pow(structured):
    """the oracle's codes for the generated rows, once against plain pow"""
    keys, rows = structured
    for r in rows:
        n, k = r.key.n, r.key.k
        s = int.from_bytes(r.sig, "big")
        if len(r.sig) != k:
            want = 1
        elif k < len(r.msg) + 11:
            want = 3
        elif s >= n:
            want = 2
        else:
            want = 0 if pow(s, r.e, n) == int.from_bytes(sk.em_of(k, r.msg), "big") else 4
        assert r.code == want, (r.key.name, r.e, r.what)
    for key in keys:
        codes = {r.code for r in rows if r.key is key}
        assert {0, 4} <= codes, key.name
        assert {r.e for r in rows if r.key is key and r.code == 0} == set(sk.EXPONENTS), key.name
    assert {r.code for r in rows} == {0, 2, 3, 4}
    assert {key.L for key in keys} == {37, 74, 80, 88, 120, 128, 152}
    assert pm.ninv_of(keys[0].n) == 1 and pm.ninv_of(keys[2].n) == pm.M28


def test_structured_rows_on_host(structured):
    """every row the kernels see (the host answers wrong lengths itself)
    through rsa_verify_lane<37|74> (t = 0, cnt = 1) and k_rsa_verify_big's
    own source built for the host, the key row computed in Python"""
    keys, rows = structured
    e = emu()
    arr = lambda v: np.array(v, dtype=np.uint32)   # noqa: E731
    seen = set()
    for key in keys:
        n28, r2, ninv = key.row28()
        n28, r2 = arr(n28), arr(r2)
        for r in rows:
            if r.key is not key or r.code in (1, 3):
                continue
            got = e.emu_rsa_verify(key.L, key.k, r.e, n28.ctypes.data_as(ctypes.c_void_p),
                                   r2.ctypes.data_as(ctypes.c_void_p), ninv, r.sig, r.msg, len(r.msg))
            assert got == r.code, (key.name, hex(r.e), r.what, got)
            seen.add((key.name, r.code))
    assert all((key.name, code) in seen for key in keys for code in (0, 2, 4))


# --- the same under the sanitizers -------------------------------------------------
def section(op, L, rows, *arrays):
    return struct.pack("<4I", op, L, rows, 0) + b"".join(np.ascontiguousarray(a, dtype="<u4").tobytes() for a in arrays)


def test_rows_under_sanitizers(tmp_path, structured):
    """rsa_emu.cpp as a stand-alone program (its own main, run as a child
    process) built with the address and undefined-behaviour sanitizers: every
    table row and every structured-key row once more, checked the same way"""
    exe = str(tmp_path / "rsa_emu_san")
    # no -g: the expanded L = 74 products take twice as long to compile with it
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-omit-frame-pointer", "-DCESS_HOSTEMU",
                           "-DRSA_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + SRCS + ["-o", exe])
    blob, plan = [], []
    for c, kind, op in units():
        rows = pm.table(c, kind)
        blob.append(section(op, c.L, len(rows), *pack(c, rows)))
        plan.append((c, kind, op, rows))
    keys, srows = structured
    pad = lambda b: b + bytes(-len(b) % 4)   # noqa: E731
    vrows = []
    for key in keys:
        n28, r2, ninv = key.row28()
        mine = [r for r in srows if r.key is key and r.code not in (1, 3)]
        body = b"".join(struct.pack("<5I", key.k, r.e & 0xffffffff, r.e >> 32, ninv, len(r.msg)) +
                        struct.pack("<%dI" % (2 * key.L), *(n28 + r2)) + pad(r.sig) + pad(r.msg) for r in mine)
        blob.append(struct.pack("<4I", OP_VERIFY, key.L, len(mine), 0) + body)
        vrows += mine
    inp, outp = str(tmp_path / "rows.bin"), str(tmp_path / "results.bin")
    with open(inp, "wb") as f:
        f.write(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    n_rows = sum(len(p[3]) for p in plan) + len(vrows)
    assert "%d sections, %d rows" % (len(plan) + len(keys), n_rows) in r.stdout
    res = np.fromfile(outp, dtype="<u4")
    pos = 0
    for c, kind, op, rows in plan:
        per = n_out(c, op)
        check_rows(c, kind, rows, res[pos:pos + per * len(rows)].reshape(len(rows), per))
        pos += per * len(rows)
    assert [int(x) for x in res[pos:pos + len(vrows)]] == [r.code for r in vrows]
    pos += len(vrows)
    assert len(res) == pos + 8
    word = lambda i: sum(int(res[pos + 4 * i + j]) << (32 * (3 - j)) for j in range(4))   # noqa: E731
    assert 0 < word(0) < 1 << 64 and 0 < word(1) <= 1 << 58
