"""CPU: the one-lane BLS primitives (bls/field.hpp Fp and Fp2, curve.hpp,
h2c.hpp, the line steps of pairing.hpp), each alone, in the host build
(tests/hostemu/lane_emu.cpp: the lane functions of tests/probe/lane_probe.hip
in a loop) against the integer references of tests/lane_probe_model.py, on the
tables the GPU probe takes (tests/test_gpu_lane_primitives.py).

hash_to_g1_parked and the LDS-parked g2_prepare exist on the device only; the
host list is the probe's list minus exactly those two.  The same tables go
through a stand-alone sanitizer program (address and undefined behaviour; its
own main, a child process).  The model is checked with no device at all: the
contracts, the inversion's iteration classes and their placement in the waves,
the isogeny's kernel points and the exceptional u of the SSWU map.
"""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lane_probe_model as pm
import oracle.bls_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HE = os.path.join(ROOT, "tests", "hostemu")
PROBE_SRC = os.path.join(ROOT, "tests", "probe", "lane_probe.hip")
EMU_SRC = os.path.join(HE, "lane_emu.cpp")
SAN_ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
P = pm.P


def _newest_source():
    hdr = os.path.join(ROOT, "cess_amd", "csrc", "bls")
    files = [EMU_SRC, PROBE_SRC, os.path.join(ROOT, "cess_amd", "csrc", "kernels.hpp")]
    files += [os.path.join(hdr, f) for f in os.listdir(hdr)]
    return max(os.path.getmtime(f) for f in files)


@pytest.fixture(scope="module")
def call():
    lib = os.path.join(HE, "liblane_emu.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < _newest_source():
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", EMU_SRC, "-o", lib])
    emu = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    emu.emu_lp.argtypes = [ctypes.c_char_p, ctypes.c_uint32, vp, vp, vp]
    emu.emu_lp_ops.restype = ctypes.c_char_p
    emu.emu_lp_soa_layout.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp, vp]

    def call(name, n, act, inp, out):
        return emu.emu_lp(name.encode(), n, act, inp, out)
    call.emu = emu
    return call


# --- the model alone ------------------------------------------------------------------
def test_probe_lists_the_models_operations(call):
    with open(PROBE_SRC) as f:
        text = f.read()
    listed, lds = pm.listed_in_source(text)
    ops = pm.ops()
    assert sorted(lds) == sorted(pm.DEVICE_ONLY)
    assert sorted(o_.name for o_ in ops) == sorted(listed) == sorted(pm.OP_NAMES)
    for op in ops:
        assert listed[op.name] == (op.n_in, op.n_out), op.name
    built = {it.split(":")[0]: tuple(int(v) for v in it.split(":")[1:])
             for it in call.emu.emu_lp_ops().decode().strip(",").split(",")}
    assert built.pop("soa_layout") == (pm.SOA_IN, pm.SOA_OUT)
    assert built == {k: v for k, v in listed.items() if k not in pm.DEVICE_ONLY}     # the probe's list minus exactly those
    assert sorted(built) == sorted(pm.HOST_OP_NAMES)
    # the production block and launch bounds, and nothing of the shipped headers edited for the probe
    assert text.count("__global__ CESS_LB void") == 4 and "dim3(256)" in text
    assert re.search(r"park\[48\]\[256\]", text) and re.search(r"QP\[12\]\[256\]", text)


def test_probe_parts_take_their_units_flags():
    """each part of the probe is compiled with the flags of the unit that ships its code, taken through the
    Makefile's variables: what CHAIN_UNITS adds to k_hash, k_decode and k_prepare reaches the probe"""
    csrc = os.path.join(ROOT, "cess_amd", "csrc")
    flags = lambda u, *v: subprocess.run(["make", "-s", "-C", csrc, "print-kflags-" + u, *v], capture_output=True,      # noqa: E731
                                         text=True, check=True).stdout.strip()
    units = {0: "k_hash", 1: "k_hash", 2: "k_hash", 3: "k_hash", 4: "k_decode", 5: "k_decode", 6: "k_prepare"}
    for part, unit in units.items():
        assert flags("lane_probe_%d" % part) == flags(unit), part
        assert flags("lane_probe_%d" % part, "CHAIN_FLAGS=-DX_CHAIN") == flags(unit, "CHAIN_FLAGS=-DX_CHAIN"), part
    assert "-DX_CHAIN" in flags("lane_probe_4", "CHAIN_FLAGS=-DX_CHAIN")
    with open(os.path.join(csrc, "Makefile")) as f:
        text = f.read()
    assert "LANE_PROBE_PARTS := 0 1 2 3 4 5 6" in text and "libcess_lane_probe.so" in text.split("clean:")[1]
    assert "$(OUT)/libcess_lane_probe.so" in text.split("all:")[1].split("\n\n")[0]


def test_tables_hold_their_contracts():
    for op in pm.ops():
        op.contract()           # every Fp operand inside the header's documented bound
        assert len(op.rows) >= pm.LANE_COUNTS[-1], (op.name, len(op.rows))
        assert all(op.rows[i] != op.rows[i + 1] for i in range(len(op.rows) - 1)), op.name
        assert op.n_unique >= 3


def test_inversion_classes_and_placement(tmp_path):
    rows, classes = pm.inv_rows()
    pm.assert_inv_placement(rows, classes)
    assert pm.get_op("fp_inv").rows[:128] == [pm.words(v) for v in rows[:128]]
    assert pm.INV_SEARCH >= 3000
    ints = [c for c in classes if isinstance(c, int)]
    print("inversion classes:", {c: classes.count(c) for c in sorted(set(classes), key=str)})
    assert min(ints) >= 20 and max(ints) <= 37
    # the two step counters agree (the big-integer rule of tools/divsteps_sim.c and the header's matrix form) ...
    for g in [1, 2, 3, 4, P - 1, (P - 1) // 2] + [v % P for v in rows[4:10] + rows[64:70]]:
        assert pm.divstep_iterations(g) == pm.divstep_iterations_matrix(g), hex(g)
    # ... and with the C tool itself on its four fixed inputs g = 1..4
    exe = str(tmp_path / "divsteps_sim")
    subprocess.check_call(["gcc", "-O2", os.path.join(ROOT, "tools", "divsteps_sim.c"), "-o", exe])
    text = subprocess.run([exe, "4"], capture_output=True, text=True, check=True, timeout=60).stdout
    line = next(ln for ln in text.splitlines() if ln.startswith("half-delta"))
    hist = {int(a): int(b) for a, b in re.findall(r" (\d+):(\d+)", line)}
    mine = {}
    for g in (1, 2, 3, 4):
        k = pm.divstep_iterations(g)
        mine[k] = mine.get(k, 0) + 1
    assert hist == mine


def test_kernel_points_and_exceptional_u():
    kern = pm.iso_kernel_points()
    assert len(kern) == 10 and len({x for x, _ in kern}) == 5
    for x, y in kern:
        assert o._poly_eval(o.ISO_XDEN, x) == 0 and o._poly_eval(o.ISO_YDEN, x) == 0
        assert y * y % P == pm.iso_rhs(x) and o.iso_map_g1((x, y)) is None
    us = pm.sswu_exceptional_u()
    assert o.ISO_Z == 11 and len(set(us)) == 3
    for u in us:
        assert (o.ISO_Z**2 * pow(u, 4, P) + o.ISO_Z * u * u) % P == 0
    sswu = pm.get_op("map_to_curve_sswu")
    assert sum(1 for t in sswu.tags[:sswu.n_unique] if t[0] == "exceptional") == 6
    iso = pm.get_op("iso_map_proj")
    assert sum(1 for t in iso.tags[:iso.n_unique] if t[0] == "kernel") >= 20
    nls = pm.get_op("normalize_lines")
    assert {t[1] for t in nls.tags if t[0] == "zero c2"} == {0, 33, 67}
    # the message rows: every length at every start offset, lengths mixed within a wave
    rows = pm.message_rows()
    assert {r[0] for r in rows} == set(pm.XMD_LENGTHS) and {r[1] for r in rows} == {0, 1, 2, 3}
    assert len({r[0] for r in rows[:14]}) > 8


# --- the host build ---------------------------------------------------------------------
@pytest.mark.parametrize("name", pm.HOST_OP_NAMES)
def test_primitive_on_host(call, name):
    op = pm.get_op(name)
    n = len(op.rows) if op.cheap else max(op.n_unique, 65)
    for half in (False, True):
        active = pm.active_mask(n, half)
        status, out = pm.run(call, op, n, active)
        assert status == 0
        pm.check_lanes(op, out, active)


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
def test_soa_layout_on_host(call, half):
    for n in pm.LANE_COUNTS:
        active = pm.active_mask(n, half)
        status, rows, tab, stride, out, slots = pm.soa_run(call.emu.emu_lp_soa_layout, n, active)
        assert status == 0 and stride > n
        pm.soa_check(rows, tab, stride, active, out, slots)
    p = ctypes.c_void_p(8)
    assert call.emu.emu_lp_soa_layout(5, 4, p, p, p, p, p) == 1       # a stride below the lane count is refused


def test_forbidden_arguments_are_refused(call):
    for name, bad in (("xmd", [4 * pm.MSG_WORDS + 1, 0]), ("hash_to_g1", [10, 4]), ("xmd_select", [4 * pm.MSG_WORDS - 2, 3])):
        op = pm.get_op(name)
        inp = np.array(op.rows[:2], dtype=np.uint32)
        inp[1, :2] = bad
        out = np.zeros((2, op.n_out), dtype=np.uint32)
        act = np.ones(2, dtype=np.uint8)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        assert call(name, 2, p(act), p(inp), p(out)) == 1
    op = pm.get_op("fp_pow_fixed")
    inp = np.array(op.rows[:1], dtype=np.uint32)
    inp[0, 0] = len(pm.EXPONENTS)
    out = np.zeros((1, 12), dtype=np.uint32)
    act = np.ones(1, dtype=np.uint8)
    assert call("fp_pow_fixed", 1, act.ctypes.data_as(ctypes.c_void_p), inp.ctypes.data_as(ctypes.c_void_p),
                out.ctypes.data_as(ctypes.c_void_p)) == 1
    assert call("no_such_operation", 1, None, None, None) == 2


def test_hash_forms_agree_on_host(call):
    """hash_to_g1 on the message rows equals expand -> two field elements -> the oracle, limb for limb canonical"""
    op = pm.get_op("hash_to_g1")
    n = op.n_unique
    _, out = pm.run(call, op, n, [1] * n)
    for i in range(n):
        want = o.hash_to_g1(pm.message_rows()[i][3])
        assert int(out[i][0]) == 0 and pm.res(pm.val(out[i][1:13])) == want[0] and pm.res(pm.val(out[i][13:25])) == want[1]


def test_primitives_under_sanitizers(tmp_path):
    exe = os.path.join(tempfile.mkdtemp(prefix="lane_san_"), "lane_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-DCESS_HOSTEMU", "-DLANE_EMU_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", EMU_SRC, "-o", exe])
    ops = [pm.get_op(n) for n in pm.HOST_OP_NAMES]
    src, dst = str(tmp_path / "ops.txt"), str(tmp_path / "results.txt")
    with open(src, "w") as f:
        for op in ops:
            n = op.n_unique
            f.write("%s %d %d %d\n" % (op.name, n, op.n_in, op.n_out))
            f.write("\n".join(" ".join(str(w) for w in r) for r in op.rows[:n]) + "\n")
        n_soa = 65
        rows, tab, stride = pm.soa_case(n_soa)
        f.write("soa_layout %d %d %d\n%d\n" % (n_soa, pm.SOA_IN, pm.SOA_OUT, stride))
        f.write("\n".join(" ".join(str(w) for w in r) for r in rows) + "\n" + " ".join(str(w) for w in tab) + "\n")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d operations" % (len(ops) + 1) in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    words = np.loadtxt(dst, dtype=np.uint64).astype(np.uint32)
    at = 0
    for op in ops:
        n = op.n_unique
        out = words[at:at + n * op.n_out].reshape(n, op.n_out)
        at += n * op.n_out
        pm.check_lanes(op, out, [1] * n)
    out = words[at:at + n_soa * pm.SOA_OUT].reshape(n_soa, pm.SOA_OUT)
    at += n_soa * pm.SOA_OUT
    pm.soa_check(rows, tab, stride, [1] * n_soa, out, words[at:at + pm.SOA_ROWS * stride])
    at += pm.SOA_ROWS * stride
    assert at == len(words)
