"""GPU: the RSA kernels' Montgomery primitives alone (cess_amd/csrc/k_rsa.hpp
mont<37|74, false|true>, canon, to_words; rsa_mont.hpp mont_rt at L = 80, 88
and 152) against integer arithmetic.

k_rsa_verify_1024 / _2048 / _2048u / _big are otherwise checked end to end
only, on products of two random primes, where every intermediate is a uniform
residue.  Here each primitive runs alone, through the test-only library
cess_amd/lib/libcess_rsa_probe.so (tests/probe/rsa_probe.hip: the shipped
headers, one kernel per operation, 256-thread blocks, built with the flags of
the production unit that holds the form), on the operand tables of
tests/rsa_probe_model.py: all-ones, mostly-zero, single-limb and every-top-fill
moduli, both extremes of ninv, operands at the ends of [0, 2n) and with every
limb 0x0fffffff.  For every row the test asserts what the CPU test
(tests/test_rsa_primitives.py) asserts of the host build: the exact residue
with R = 2^(28 L) applied here, the range (< 2n; <= n for a multiply by one;
< n after canon) and every limb <= 0x0fffffff.

Placement: every operation runs on its whole table and with 1, 65 and 257
lanes (one lane; a wave and a lane; a block and a lane), and once more with
every lane i mod 4 in {1, 2} switched off, whose results must come back as the
poison they were filled with.  Neighbouring lanes hold different operands and,
in the kernels that keep the modulus in VGPRs, different moduli; the `u`
kernels read the key row through a wave-uniform index as k_rsa_verify_2048u
does, so their lanes are laid out one modulus per wave, the last wave of a
modulus padded with inactive lanes.  The probe's kernels are compiled apart
from the production kernels: this checks the headers' arithmetic at the edges,
the end-to-end tests keep checking those kernels' code generation."""
import ctypes
import os

import numpy as np
import pytest

import rsa_probe_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cess_amd", "lib", "libcess_rsa_probe.so")
MAKE_HINT = "make -C cess_amd/csrc ../lib/libcess_rsa_probe.so"
LMAX = 152                        # rsa.hpp RSA_LMAX
KEY_WORDS = 6 + 2 * LMAX          # RsaKeyDev: k_bytes, ninv, limbs, pad, e (2 words), n28, r2_28

_lib = []


def probe():
    if not _lib:
        if not os.path.exists(LIB):
            pytest.fail("%s is missing: build it with `%s` (or `make -C cess_amd/csrc`)" % (LIB, MAKE_HINT))
        lib = ctypes.CDLL(LIB)
        lib.rsa_probe_ops.restype = ctypes.c_char_p
        lib.rsa_probe_error.restype = ctypes.c_char_p
        _lib.append(lib)
    return _lib[0]


def key_table(c, mods):
    """RsaKeyDev rows of the moduli, as the host's key_row would fill them"""
    t = np.zeros((len(mods), KEY_WORDS), dtype=np.uint32)
    for j, n in enumerate(mods):
        t[j, 0] = (n.bit_length() + 7) // 8
        t[j, 1] = pm.ninv_of(n)
        t[j, 2] = c.L
        t[j, 4] = 65537
        t[j, 6:6 + c.L] = pm.limbs(n, c.L)
        t[j, 6 + LMAX:6 + LMAX + c.L] = pm.limbs(c.R * c.R % n, c.L)
    return t


def layout(op, rows):
    """(rows, live) in lane order: different moduli in neighbouring lanes, or,
    for the wave-uniform kernels, one modulus per wave (its last wave padded
    with dead copies of a row)"""
    if not op.uni:
        rows = pm.interleaved(rows)
        return rows, [1] * len(rows)
    out, live = [], []
    groups = {}
    for r in rows:
        groups.setdefault(r.n, []).append(r)
    for g in groups.values():
        padn = -len(g) % 64
        out += g + [g[0]] * padn
        live += [1] * len(g) + [0] * padn
    return out, live


def run(op, rows, active):
    """launch op's kernel, one lane per row; the (n, n_out) results, rows of
    inactive lanes still holding the poison"""
    lib, c, n = probe(), op.cls, len(rows)
    mods = sorted({r.n for r in rows})
    where = {m: j for j, m in enumerate(mods)}
    keys = key_table(c, mods)
    lim = lambda vs: np.array([pm.limbs(v, c.L) for v in vs], dtype=np.uint32).reshape(n, c.L)   # noqa: E731
    a, b = lim([r.a for r in rows]), lim([r.b for r in rows])
    ki = np.array([where[r.n] for r in rows], dtype=np.uint32)
    act = np.array(active, dtype=np.uint8)
    out = np.full((n, op.n_out), pm.POISON, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    rc = getattr(lib, "rp_" + op.entry)(ctypes.c_uint32(n), p(act), p(ki), p(keys), ctypes.c_uint32(len(mods)),
                                        p(a), p(b), p(out), ctypes.c_int(c.L))
    if rc != 0:     # a HIP error (a fault included): nothing more is launched on this device
        pytest.exit("rp_%s: HIP status %d (%s)" % (op.entry, rc, lib.rsa_probe_error(rc).decode()), returncode=3)
    return out


def check(op, rows, live, half):
    n = len(rows)
    active = [lv & m for lv, m in zip(live, pm.active_mask(n, half))]
    out = run(op, rows, active)
    for i in range(n):        # every lane is compared
        if not active[i]:
            assert (out[i] == pm.POISON).all(), (op.name, n, i, "an inactive lane's result was written")
            continue
        assert not (out[i] == pm.POISON).all(), (op.name, n, i, "no result")
        op.check(rows[i], out[i])
    return out


def test_probe_covers_the_model():
    """the library's entry points and the model's operations are the same set,
    with the same limb counts, in the production block size and key row"""
    lib = probe()
    listed = {}
    for item in lib.rsa_probe_ops().decode().strip(",").split(","):
        name, L, kind = item.split(":")
        listed[name] = (int(L), kind)
    assert lib.rsa_probe_threads() == 256 and lib.rsa_probe_key_words() == KEY_WORDS
    kinds = {"mul": "OP_MUL", "sqr": "OP_SQR", "canon": "OP_CANON", "words": "OP_WORDS"}
    used = set()
    for op in pm.ops():
        assert op.entry in listed and hasattr(lib, "rp_" + op.entry), op.entry
        assert listed[op.entry] == ((0 if op.cls.loop else op.cls.L), kinds[op.kind]), op.name
        used.add(op.entry)
    assert sorted(used) == sorted(listed)
    assert {op.cls.L for op in pm.ops() if op.cls.loop} == {80, 88, 152}


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
@pytest.mark.parametrize("name", pm.op_names())
def test_rsa_primitive(name, half):
    """one primitive at 1, 65 and 257 lanes and on its whole table, all lanes
    live or lanes i mod 4 in {1, 2} switched off"""
    op = pm.get_op(name)
    rows, live = layout(op, op.rows)
    assert sum(live) == len(op.rows)
    if not op.uni:
        assert all(rows[i].n != rows[i + 1].n for i in range(min(len(rows), 257) - 1))
    for n in pm.LANE_COUNTS + (len(rows),):
        out = check(op, rows[:n], live[:n], half)
    if op.kind == "mul" and not half:       # the whole table: canon has work to do
        assert any(pm.from_limbs(w) >= r.n for r, w, lv in zip(rows, out, live) if lv)
