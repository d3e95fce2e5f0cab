"""CPU: the lane-group layer (bls/group.hpp: the half-products grp_mul_comp and
grp_sqr_comp, grp_operand's lazily reduced operands, the LIN and INV forms) in
the host build (tests/hostemu/group_probe_emu.cpp: the lane functions of
tests/probe/group_probe.hip and a round loop over group_eval_comp with
read-before-write semantics) against the integer model of
tests/group_probe_model.py, on the tables the GPU probe takes
(tests/test_gpu_group_primitives.py).

Beside the tables: the lazy-reduction bounds PROVED from NEG_K28, P28 and the
operand class maxima for every (kind, flag byte) the two programs hold; the
contracts of the generated programs that group.hpp only states in comments;
the committed program headers against what gen_group.py writes now; the
model's own sensitivity (one planted error at a time must fail on the tables);
and the same tables through a stand-alone sanitizer program (address and
undefined behaviour; its own main, a child process).

The device's round loop (group_rounds of k_group.hip, one function for k_group,
k_group_fe and the probe's `round` entry) has no host build: the host round
loop here is group_probe_emu.cpp's own, over the same group_eval_comp.
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import group_probe_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HE = os.path.join(ROOT, "tests", "hostemu")
CSRC = os.path.join(ROOT, "cess_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "probe", "group_probe.hip")
EMU_SRC = os.path.join(HE, "group_probe_emu.cpp")
SAN_ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
P = pm.P
MUTANTS = {"k28": "NEG_K28 off by one in one digit", "nosub": "the subtract flag ignored", "xisign": "LIN's xi sign flipped",
           "early": "writes landing before reads"}


def _newest_source():
    hdr = os.path.join(CSRC, "bls")
    files = [EMU_SRC, PROBE_SRC] + [os.path.join(hdr, f) for f in os.listdir(hdr)]
    return max(os.path.getmtime(f) for f in files)


@pytest.fixture(scope="module")
def emu():
    lib = os.path.join(HE, "libgroup_probe_emu.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < _newest_source():
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", EMU_SRC, "-o", lib])
    e = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    for f in (e.emu_gp_grp_mul_comp, e.emu_gp_grp_sqr_comp):
        f.argtypes = [ctypes.c_uint32, vp, vp, vp]
    e.emu_gp_round.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]
    e.emu_gp_ops.restype = ctypes.c_char_p
    e.comp = lambda name, lanes, act, inp, out: getattr(e, "emu_gp_" + name)(lanes, act, inp, out)
    return e


# --- the probe, the host build and the model name the same entries -------------------------
def test_probe_lists_the_models_operations(emu):
    built = {it.split(":")[0]: tuple(int(v) for v in it.split(":")[1:]) for it in emu.emu_gp_ops().decode().strip(",").split(",")}
    assert built == pm.OPS
    g, _, _, nslots, _, _ = pm.programs()["full"]
    assert emu.emu_gp_slots() == nslots and emu.emu_gp_consts() == len(g.consts)
    with open(PROBE_SRC) as f:
        text = f.read()
    # the kernel's block and launch bounds; the shipped unit and headers included as they are
    assert text.count("__global__ __launch_bounds__(64) void") == 3 and text.count("dim3(64)") == 4
    assert '#include "../../cess_amd/csrc/k_group.hip"' in text and "S[grp::N_SLOTS][6]" in text
    # one round loop for the two kernels and the probe
    with open(os.path.join(CSRC, "k_group.hip")) as f:
        unit = f.read()
    assert unit.count("group_rounds(R, ") == 2 and unit.count("group_eval_comp(") == 1 and text.count("group_rounds(R, ") == 1
    assert "group_eval_comp(" not in text.split("#if !defined(CESS_HOSTEMU)\n\n__global__")[1]


def test_probe_takes_k_groups_flags():
    flags = lambda u, *v: subprocess.run(["make", "-s", "-C", CSRC, "print-kflags-" + u, *v], capture_output=True,      # noqa: E731
                                         text=True, check=True).stdout.strip()
    assert flags("group_probe") == flags("k_group")
    assert flags("group_probe", "CHAIN_FLAGS=-DX_CHAIN") == flags("k_group", "CHAIN_FLAGS=-DX_CHAIN")
    assert "-DX_CHAIN" in flags("group_probe", "CHAIN_FLAGS=-DX_CHAIN")
    with open(os.path.join(CSRC, "Makefile")) as f:
        text = f.read()
    assert "$(OUT)/libcess_group_probe.so" in text.split("all:")[1].split("\n\n")[0]
    assert "libcess_group_probe.so" in text.split("clean:")[1]
    link = text.split("$(OUT)/libcess_bls.so:")[1].split("\n\n")[0]
    assert "group_probe" not in link                          # a library of its own


# --- the tables ----------------------------------------------------------------------------------
def test_tables_hold_their_contracts():
    """Every operand lies inside its class; neighbouring rows differ; each class pair of the programs has the
    product of its two maxima.  The double-width value grp_mul_comp / grp_sqr_comp reduce, computed from the
    digits with NEG_K28 - digit for a negation, is congruent to the plain formula on every row (NEG_K28 = 0 mod p),
    lies below p R and has every column below 2^64.

    A component is 12 words, so a digit is at most 0xfffffff (the top one 0xfffff), and every NEG_K28 digit is
    above that: no operand's digit can equal NEG_K28[i] or be one below it.  The nearest rows a register file can
    hold are in the tables: each digit alone at its maximum, and every digit at its maximum under each class's
    largest top digit."""
    assert all(k > pm.M28 for k in pm.NEG_K28[:13]) and pm.NEG_K28[13] > 0xFFFFF and pm.NEG_K28[13] == 0x1040AA
    assert pm.K_VALUE % P == 0 and pm.digits(P) == pm.P28
    assert all(v[0] < P and v[1] < P for v in pm.pool())
    for name in ("grp_mul_comp", "grp_sqr_comp"):
        rows, tags = pm.comp_table(name)
        assert len(rows) >= pm.PAIR_COUNTS[-1] and all(rows[i] != rows[i + 1] for i in range(len(rows) - 1))
        for row, tag in zip(rows, tags):
            comps = [c for v in row for c in v] if name == "grp_mul_comp" else list(row)
            assert all(0 <= c <= 4 * P - 2 for c in comps), tag
            for comp in (0, 1):
                t, col = pm.mul_comp_digits(row[0], row[1], comp) if name == "grp_mul_comp" else pm.sqr_comp_digits(row, comp)
                assert t * pm.RINV % P == pm.expect_comp(name, row)[comp], tag
                assert t < P * pm.R and col < 1 << 63, tag
    mtags = pm.comp_table("grp_mul_comp")[1]
    for ca, cb in pm._class_pairs():
        assert ("maxima", ca, cb) in mtags
    stags = pm.comp_table("grp_sqr_comp")[1]
    for cls in pm._class_singles():
        assert ("maximum", cls) in stags
    for cls, m in pm.CLASS_MAX.items():
        edges = pm.class_edges(cls)
        assert max(edges) == m and all(0 <= e <= m for e in edges)
        if cls in ("slot", "slot+slot"):
            assert {0, 1, pm.ONE, P - 1, P, P + 1, 2 * P - 1} <= set(edges)
            assert all(e + P in edges for e in edges if e < P)
            assert {1 << (28 * i) for i in range(14)} <= set(edges)
            assert (((m >> 364) << 364) | ((1 << 364) - 1)) in edges or ((((m >> 364) - 1) << 364) | ((1 << 364) - 1)) in edges
    assert 4 * P - 2 in pm.class_edges("slot+slot")


def test_round_table_covers_the_programs():
    """The coverage condition, with no exceptions: every MUL / SQR flag byte and every LIN shape of generate() and
    of build_fe is a row of the round table, under the kind it has in the program; so are the unused combinations
    of bits 1..32, 12 terms in each single class, a 3/3/3/3 split, INV with c1 = 0 and with c0 = 0, rounds of 1,
    31 and 32 operations, and a destination that the other 31 operations read."""
    flags, shapes, inv = pm.found_forms()
    cases = pm.round_cases()
    have_flags, have_shapes, cnts = set(), set(), set()
    for c in cases:
        cnts.add((c.kind, c.cnt))
        for e in c.ents[c.off:c.off + c.cnt]:
            if c.kind in (pm.OP_MUL, pm.OP_SQR):
                have_flags.add((c.kind, e[5]))
            elif c.kind == pm.OP_LIN:
                have_shapes.add((e[1] & 15, e[1] >> 4, e[2] & 15, e[2] >> 4))
    print("flag bytes found:", sorted(flags), "LIN shapes found:", len(shapes), "INV:", inv)
    assert flags <= have_flags and shapes <= have_shapes and inv == 2
    assert {(k, f) for k in (pm.OP_MUL, pm.OP_SQR) for f in range(64)} <= have_flags
    assert {(12, 0, 0, 0), (0, 12, 0, 0), (0, 0, 12, 0), (0, 0, 0, 12), (3, 3, 3, 3)} <= have_shapes
    for kind in (pm.OP_MUL, pm.OP_SQR, pm.OP_LIN):
        assert {(kind, 1), (kind, 31), (kind, 32)} <= cnts
    inv_vals = [c.image[c.ents[c.off][1]] for c in cases if c.kind == pm.OP_INV]
    assert any(v[1] % P == 0 and v[0] % P for v in inv_vals) and any(v[0] % P == 0 and v[1] % P for v in inv_vals)
    assert sum(1 for c in cases if c.tag[0] == "alias") == 6 and any(c.off for c in cases)
    assert all(len(c.image) == pm.ROUND_USED < pm.ROUND_SLOTS for c in cases)
    for c in [c for c in cases if c.tag[0] == "alias"]:     # operation 0 writes d; every other operation reads d
        d = c.ents[0][0]
        assert c.cnt == 32 and all(d in e[1:5] or (c.kind == pm.OP_LIN and d in e[3:15]) for e in c.ents[1:])


# --- the host build -----------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
@pytest.mark.parametrize("name", ["grp_mul_comp", "grp_sqr_comp"])
def test_half_product_on_host(emu, name, half):
    """the named component of A B / R (A^2 / R) mod p, below 2p, on every row; switched-off rows stay poison"""
    for n in pm.PAIR_COUNTS + (len(pm.comp_table(name)[0]),):
        active = pm.active_rows(n, half)
        status, out = pm.run_comp(emu.comp, name, n, active)
        assert status == 0
        pm.check_comp(name, out, active)


@pytest.mark.parametrize("half", [False, True], ids=["all", "halfquads"])
def test_round_on_host(emu, half):
    """every row of the round table, then the same rounds on their neighbours' images, then a full-size image"""
    cases = pm.round_cases()
    for table, n_slots in ((cases, pm.ROUND_SLOTS), (pm.rotate_images(cases), pm.ROUND_SLOTS), (cases[:1], pm.ROUND_SLOTS),
                           (pm.wide_cases(), pm.programs()["full"][3])):
        active = pm.active_rows(len(table), half)
        status, before, after = pm.run_round(emu.emu_gp_round, table, active, n_slots)
        assert status == 0
        pm.check_round(table, active, before, after)


def test_forbidden_arguments_are_refused(emu):
    cases = pm.round_cases()[:2]
    for bad in ("slot", "const", "count", "terms", "kind"):
        c = pm.Case(cases[0].kind, cases[0].ents[:cases[0].cnt], cases[0].image)
        if bad == "slot":
            c.ents[0][0] = pm.ROUND_SLOTS
        elif bad == "const":
            c.ents[0][1], c.ents[0][5] = len(pm.pool()), 16
        elif bad == "count":
            c.cnt, c.off = 32, 1
        elif bad == "terms":
            c.kind, c.ents[0][1], c.ents[0][2] = pm.OP_LIN, 0x66, 0x01
        else:
            c.kind = 4
        status, before, after = pm.run_round(emu.emu_gp_round, [c], [1])
        assert status == 1 and np.array_equal(before, after), bad
    assert pm.run_comp(emu.comp, "grp_mul_comp", 1, [1])[0] == 0
    p = ctypes.c_void_p(8)
    assert emu.emu_gp_grp_mul_comp(3, p, p, p) == 1 and emu.emu_gp_grp_sqr_comp(0, p, p, p) == 1


# --- the model notices each planted error -----------------------------------------------------
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_model_with_one_error_fails_on_the_tables(emu, mut):
    """the host build's results, right under the model, are wrong under the model with one deliberate error"""
    if mut == "k28":
        for name in ("grp_mul_comp", "grp_sqr_comp"):
            n = len(pm.comp_table(name)[0])
            _, out = pm.run_comp(emu.comp, name, n, [1] * n)
            pm.check_comp(name, out, [1] * n)
            with pytest.raises(AssertionError):
                pm.check_comp(name, out, [1] * n, mut)
        return
    cases = pm.round_cases()
    _, before, after = pm.run_round(emu.emu_gp_round, cases, [1] * len(cases))
    pm.check_round(cases, [1] * len(cases), before, after)
    with pytest.raises(AssertionError):
        pm.check_round(cases, [1] * len(cases), before, after, mut)


# --- the bounds, proved -------------------------------------------------------------------------
def _digit_max(m):
    """the largest digits of any value <= m < 2^384: 0xfffffff below the top digit, the top digit m >> 364"""
    return [pm.M28] * 13 + [m >> 364]


def _worst(kind, comp, ma, mb):
    """(worst double-width value, worst 64-bit accumulator, worst 32-bit operand digit) of a half-product whose
    operand components are at most ma (A) and mb (B)"""
    K, kv = pm.NEG_K28, pm.K_VALUE
    da, db = _digit_max(ma), _digit_max(mb)
    assert all(k >= d for k, d in zip(K, db)) and all(k >= d for k, d in zip(K, da))     # K[i] - digit never wraps
    if kind == pm.OP_MUL:
        # comp 0: a0 b0 + a1 (K - b1), K[j] - b1[j] <= K[j]; comp 1: a0 b1 + a1 b0
        pairs = [(da, db), (da, K)] if comp == 0 else [(da, db), (da, db)]
        value = ma * mb + ma * kv if comp == 0 else 2 * ma * mb
    elif comp == 0:
        # (a0 + a1)(a0 + K - a1)
        pairs, value = [([2 * d for d in da], [d + k for d, k in zip(da, K)])], 2 * ma * (ma + kv)
    else:
        # a0 (2 a1)
        pairs, value = [(da, [2 * d for d in da])], 2 * ma * ma
    word = max(max(max(u), max(v)) for u, v in pairs)
    acc, worst = 0, 0
    for k in range(27):                                    # mont28_d: column k, the reduction's m_i P28[k - i], the carry
        col = sum(u[i] * v[k - i] for u, v in pairs for i in range(14) if 0 <= k - i < 14)
        red = sum(pm.M28 * pm.P28[k - i] for i in range(14) if 0 <= k - i < 14 and (i < k or k < 14))
        acc = col + red + (acc >> 28)
        worst = max(worst, acc)
    return value, worst, word


def test_lazy_reduction_bounds_are_proved():
    """For every (kind, flag byte) of either program, from NEG_K28, P28 and the class maxima alone.

    An operand component of class c is at most CLASS_MAX[c]: a slot < 2p (the register-file contract), a pool
    constant < p, add_nr of two < 4p (of a constant and a slot < 3p), sub() and neg() < 2p.  Its 28-bit digits are
    at most 0xfffffff, the top one at most CLASS_MAX >> 364.  grp_mul_comp accumulates, in column k, the products
    x0_i y0_j + x1_i y1_j (i + j = k) with y1_j = NEG_K28_j - b1_j <= NEG_K28_j for component 0; grp_sqr_comp the
    products xs_i ys_j with xs = a0 + a1, ys = a0 + NEG_K28 - a1 (component 0) or xs = a0, ys = 2 a1.  mont28_d adds
    to each column at most 14 products m_i P28_j (m_i <= 0xfffffff) and the previous accumulator >> 28.  So
      (1) every digit-wise operand fits 32 bits and NEG_K28_j - digit never wraps,
      (2) the 64-bit accumulator stays below 2^64 in every column,
      (3) the double-width value T stays below p R,
    and since the reduction returns (T + m p) / R with m < R = 2^392, the result is below (p R + R p) / R = 2p."""
    flags = pm.found_forms()[0]
    seen = {}
    for kind, f in sorted(flags | {(pm.OP_MUL, 15), (pm.OP_SQR, 5)}):
        ca, cb = pm.flag_classes(kind, f)
        for comp in (0, 1):
            value, acc, word = _worst(kind, comp, pm.CLASS_MAX[ca], pm.CLASS_MAX[cb])
            assert word < 1 << 32, (kind, f, comp)
            assert acc < 1 << 64, (kind, f, comp, acc.bit_length())
            assert value < P * pm.R, (kind, f, comp, value.bit_length())
            seen[(kind, f, comp)] = (acc.bit_length(), value.bit_length())
    print("worst accumulator and value bits:", seen)
    # SQR of a sum: a column near 2^62.4, a value near 2^769
    assert seen[(pm.OP_SQR, 5, 0)][0] <= 63 and 768 <= seen[(pm.OP_SQR, 5, 0)][1] <= 770
    assert (P * pm.R).bit_length() == 773


# --- the programs' contracts ----------------------------------------------------------------
@pytest.mark.parametrize("which", ["full", "fe"])
def test_program_contracts(which):
    """what group.hpp states in comments, of generate() and of the FE build"""
    g, rounds, slot, nslots, heads, ents = pm.programs()[which]
    n_consts = len(pm.programs()["full"][0].consts)
    table_flags = {(k, f) for k in (pm.OP_MUL, pm.OP_SQR) for f in pm.table_flags()}
    table_shapes = set(pm.table_shapes())
    assert len(g.consts) == n_consts and nslots <= pm.programs()["full"][3] and nslots <= 256
    at = 0
    for kind, cnt, off in heads:
        assert kind in (pm.OP_MUL, pm.OP_SQR, pm.OP_LIN, pm.OP_INV) and 1 <= cnt <= 32 and off == at
        at += cnt
        dests = [e[0] for e in ents[off:off + cnt]]
        assert len(set(dests)) == cnt                       # no two operations of a round write the same slot
        for e in ents[off:off + cnt]:
            assert len(e) == 16 and all(0 <= b < 256 for b in e) and e[0] < nslots
            if kind in (pm.OP_MUL, pm.OP_SQR):
                d, a0, a1, b0, b1, f = e[:6]
                assert not (f & 64 and f & 1), e            # a conjugate only on a plain operand
                assert f < 128 and e[6:] == [0] * 10        # (no conjugate flag exists for B)
                assert not (f & 16 and f & 1) and not (f & 32 and f & 4), e     # a constant never has a second slot
                assert not (f & 2 and not f & 1) and not (f & 8 and not f & 4), e
                assert a0 < (n_consts if f & 16 else nslots) and b0 < (n_consts if f & 32 else nslots), e
                assert a1 < nslots and b1 < nslots, e
                assert (kind, f) in table_flags, e          # the coverage condition
            elif kind == pm.OP_LIN:
                n = (e[1] & 15, e[1] >> 4, e[2] & 15, e[2] >> 4)
                assert 1 <= sum(n) <= 12 and 3 + sum(n) <= 16 and all(s < nslots for s in e[3:3 + sum(n)]), e
                assert e[3 + sum(n):] == [0] * (13 - sum(n)) and n in table_shapes, e
            else:
                assert cnt == 1 and e[1] < nslots and e[2:] == [0] * 14
    assert at == len(ents) < 1 << 16
    assert sum(1 for k, _, _ in heads if k == pm.OP_INV) == 1


def test_generator_refuses_a_conjugate_on_a_sum():
    """encode() raises on flag 64 together with a second slot (conj(add_nr(..)) would wrap in the kernel), as it
    does on a conjugate on B; simulate() alone would conjugate after the sum and pass"""
    m = pm.gen()
    for bad in (0, 1):
        g = m.Graph()
        a, b, c = g.inp("a"), g.inp("b"), g.inp("c")
        plain, conj_sum = (c.n, None, False, False), (a.n, b.n, False, True)
        n = g._new("mul", (conj_sum, plain) if bad == 0 else (plain, (a.n, None, False, True)))
        g.out("x", m.H(n))
        with pytest.raises(ValueError):
            m.generate(g)
    g = m.Graph()
    a, c = g.inp("a"), g.inp("c")
    g.out("x", g.mul(("conj", a), c))
    heads, ents = m.generate(g)[4:6]
    assert ents[0][5] == 64


def test_committed_headers_are_current(tmp_path):
    """bls/group_prog.hpp and bls/group_fe_prog.hpp are, byte for byte, what gen_group.py writes now"""
    work = tmp_path / "csrc"
    (work / "bls").mkdir(parents=True)
    shutil.copy(os.path.join(CSRC, "gen_group.py"), work / "gen_group.py")
    subprocess.run([sys.executable, str(work / "gen_group.py")], check=True, capture_output=True, timeout=300)
    for name in ("group_prog.hpp", "group_fe_prog.hpp"):
        with open(work / "bls" / name, "rb") as f, open(os.path.join(CSRC, "bls", name), "rb") as h:
            assert f.read() == h.read(), name


# --- the whole-kernel rows (run on the GPU only): what the model asserts of them -----------------
def test_whole_kernel_rows():
    fe = pm.fe_rows()
    tags = {r[0] for r in fe}
    assert {"Fp", "Fp2", "Fp6", "golden Miller value", "coefficients 0, 1, p - 1"} <= tags
    assert {"sparse w^%d" % k for k in range(6)} <= tags and len(fe) == 2 * len(tags)
    for n in pm.BLOCK_COUNTS:
        rows = pm.pick(fe, n)
        assert all(rows[i] != rows[i + 1] for i in range(n - 1))
    assert {id(r) for r in pm.pick(fe, 65)} == {id(r) for r in fe}
    recs = pm.group_recs()                      # (asserts the single INV operand nonzero and the subgroup check failing)
    assert len(recs) <= 65 and {id(r) for r in pm.pick(recs, 65)} == {id(r) for r in recs}
    assert sum(1 for r in recs if r.want_code == 4 and r.want_gt is None and not r.code2) >= 12
    assert sum(1 for r in recs if r.tag.startswith("values") and r.inf == pm.INF_PK) >= 12


# --- sanitizers -------------------------------------------------------------------------------------
def test_tables_under_sanitizers(tmp_path):
    exe = os.path.join(tempfile.mkdtemp(prefix="group_san_"), "group_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-DCESS_HOSTEMU", "-DGROUP_EMU_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", EMU_SRC, "-o", exe])
    src, dst = str(tmp_path / "ops.txt"), str(tmp_path / "results.txt")
    line = lambda ws: " ".join(str(int(w)) for w in ws) + "\n"      # noqa: E731
    cases = pm.round_cases()
    holder = {}

    def grab(n, n_slots, act, heads, ents, img):
        holder["n"] = n
        return 0
    _, before, _ = pm.run_round(grab, cases, [1] * len(cases))
    with open(src, "w") as f:
        for name in ("grp_mul_comp", "grp_sqr_comp"):
            rows = pm.comp_table(name)[0]
            f.write("%s %d\n" % (name, 2 * len(rows)))
            for r in rows:
                f.write(line(pm.comp_words(name, r)))
        f.write("round %d %d\n" % (len(cases), pm.ROUND_SLOTS))
        f.write(line(c.head() for c in cases))
        for c in cases:
            f.write(line(c.ent_words()))
        f.write(line(before.reshape(-1)))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "3 operations" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = np.loadtxt(dst, dtype=np.uint64).astype(np.uint32)
    at = 0
    for name in ("grp_mul_comp", "grp_sqr_comp"):
        n = len(pm.comp_table(name)[0])
        pm.check_comp(name, got[at:at + 24 * n].reshape(2 * n, 12), [1] * n)
        at += 24 * n
    after = got[at:].reshape(before.shape)
    pm.check_round(cases, [1] * len(cases), before, after)
