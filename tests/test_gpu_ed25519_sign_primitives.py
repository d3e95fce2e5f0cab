"""GPU: the primitives of cess_amd/csrc/ed25519_sign.hpp, each alone, against
integer arithmetic.

The signer is otherwise checked end to end only, on scalars that are hashes
nobody can choose.  Here clamp, sc_reduce256, sc_muladd, the comb build and
ge_scalarmult_base run alone, through the test-only library
cess_amd/lib/libcess_ed25519_sign_probe.so (tests/probe/ed25519_sign_probe.hip:
the shipped header, one kernel per operation, the production blocks and launch
bounds, built with k_ed25519_sign's flags), on the tables of
tests/golden/ed25519_sign_edges.json: scalars with every digit 7, every digit
-8, carries through all 64 digits, single digits at the word boundaries, the
ends of the range, and the sc_muladd triples at the top of the 512-bit sum.
Every operation also runs with 1, 65 and 257 lanes, neighbouring lanes holding
different rows."""
import ctypes
import hashlib
import os

import pytest

import ed25519_model as model
from test_ed25519_sign import check_comb, edges, unwords, words  # noqa: F401  (edges: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cess_amd", "lib", "libcess_ed25519_sign_probe.so")
L = model.L
_lib = []


def probe():
    if not _lib:
        if not os.path.exists(LIB):
            pytest.fail("%s is missing: build it with `make -C cess_amd/csrc`" % LIB)
        lib = ctypes.CDLL(LIB)
        lib.ed25519_sign_probe_error.restype = ctypes.c_char_p
        _lib.append(lib)
    return _lib[0]


def run(name, rows, n_out=8):
    lib = probe()
    flat = [w for r in rows for w in r]
    out = (ctypes.c_uint32 * (n_out * len(rows)))(*([0xDEADBEEF] * (n_out * len(rows))))
    rc = getattr(lib, "edsp_" + name)(ctypes.c_uint32(len(rows)), (ctypes.c_uint32 * len(flat))(*flat), out)
    if rc != 0:     # a HIP error (a fault included): nothing more is launched on this device
        pytest.exit("edsp_%s: HIP status %d (%s)" % (name, rc, lib.ed25519_sign_probe_error(rc).decode()), returncode=3)
    return [list(out[n_out * i:n_out * (i + 1)]) for i in range(len(rows))]


def cycle(rows, n):
    return [rows[i % len(rows)] for i in range(n)]


@pytest.mark.parametrize("n", [None, 1, 65, 257])
def test_scalarmult_base(edges, n):
    tab = edges["scalars"] if n is None else cycle(edges["scalars"], n)
    got = run("ge_scalarmult_base", [words(k) for k, _ in tab])
    assert [unwords(g).to_bytes(32, "little") for g in got] == [e for _, e in tab]


@pytest.mark.parametrize("n", [None, 1, 65, 257])
def test_sc_muladd(edges, n):
    tab = edges["muladd"] if n is None else cycle(edges["muladd"], n)
    got = run("sc_muladd", [words(k) + words(a) + words(r) for k, a, r, _ in tab])
    assert [unwords(g) for g in got] == [s for _, _, _, s in tab]


def test_clamp_and_reduce(edges):
    hs = [int.from_bytes(hashlib.sha512(bytes([i])).digest()[:32], "little") for i in range(63)] + [0, 2**256 - 1]
    got = run("clamp", [words(h) for h in hs])
    want = [model._clamp(h.to_bytes(32, "little")) for h in hs]
    assert [unwords(g) for g in got] == want and all(2**254 <= w < 2**255 and w % 8 == 0 for w in want)
    vals = want + [L - 1, L, L + 1, 2**255 - 8, 2 * L, 15 * L + 3, 2**256 - 1]
    got = run("sc_reduce256", [words(v) for v in vals])
    assert [unwords(g) for g in got] == [v % L for v in vals]
    # the probe refuses what the lanes' bounds forbid, before anything is launched
    lib = probe()
    out = (ctypes.c_uint32 * 8)()
    assert lib.edsp_ge_scalarmult_base(ctypes.c_uint32(1), (ctypes.c_uint32 * 8)(*words(L)), out) != 0
    assert lib.edsp_clamp(ctypes.c_uint32(0), (ctypes.c_uint32 * 8)(), out) != 0


def test_comb_build():
    lib = probe()
    tab = (ctypes.c_uint32 * (64 * 240))()
    st = (ctypes.c_uint8 * 64)(*([0xEE] * 64))
    rc = lib.edsp_comb(tab, st)
    if rc != 0:
        pytest.exit("edsp_comb: HIP status %d (%s)" % (rc, lib.ed25519_sign_probe_error(rc).decode()), returncode=3)
    assert list(st) == [0] * 64
    check_comb(list(tab))
