"""CPU: the device-side algorithms (cess_amd/csrc/bls/*.hpp — the exact source the
gfx950 kernels are built from) compiled for the host by a TEST-ONLY harness
(tests/hostemu/emu.cpp, -DCESS_HOSTEMU) and checked against the golden vectors.
This is not a product path: the shipped library is gfx950-only."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostemu", "emu.cpp")
LIB = os.path.join(HERE, "hostemu", "libemu.so")


@pytest.fixture(scope="module")
def emu():
    hdr_dir = os.path.join(HERE, "..", "cess_amd", "csrc", "bls")
    newest = max(os.path.getmtime(os.path.join(hdr_dir, f)) for f in os.listdir(hdr_dir))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(newest, os.path.getmtime(SRC)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", SRC, "-o", LIB])
    return ctypes.CDLL(LIB)


def test_codes_and_gt(emu, vectors):
    for c in vectors["cases"]:
        s, m, k = bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"])
        gt = (ctypes.c_uint8 * 576)()
        code = emu.emu_verify(s, m, len(m), k, gt)
        assert code == c["code"], c["name"]
        if "gt" in c:
            assert bytes(gt).hex() == c["gt"], c["name"]


def test_normalized_key_lines_keep_gt(emu, vectors):
    """A distinct-key table's lines scaled to c2 = 1 by normalize_lines (one
    Fp2 inversion per key, k_norm_keys) and the Miller loop's norm1 path
    (pair 1 through the 9-product sparse multiply) give the golden codes and
    Gt bytes."""
    old = emu.emu_set_norm_pk(1)
    try:
        for c in vectors["cases"]:
            s, m, k = bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"])
            gt = (ctypes.c_uint8 * 576)()
            code = emu.emu_verify(s, m, len(m), k, gt)
            assert code == c["code"], c["name"]
            if "gt" in c:
                assert bytes(gt).hex() == c["gt"], c["name"]
    finally:
        emu.emu_set_norm_pk(old)


def test_hash_to_g1(emu, vectors):
    import oracle.bls_oracle as o
    for h in vectors["hash_to_g1"]:
        m = bytes.fromhex(h["msg"])
        out = (ctypes.c_uint32 * 24)()
        inf = ctypes.c_int()
        emu.emu_hash(m, len(m), out, ctypes.byref(inf))
        x = sum(out[i] << (32 * i) for i in range(12))
        y = sum(out[12 + i] << (32 * i) for i in range(12))
        assert o.g1_to_compressed((x, y)).hex() == h["h"]


def test_clear_cofactor_jacobian(emu):
    """h2c.hpp clear_cofactor_g1: the Jacobian [1 - x] ladder (incomplete
    formulas, complete recompute when it ends with Z = 0) equals the oracle's
    [h_eff]R on random points of E(Fp) and on the order-3 points (0, +-2),
    whose ladder hits T = -R and takes the complete recompute."""
    import random

    import oracle.bls_oracle as o
    rng = random.Random(29)
    limbs = lambda v: (ctypes.c_uint32 * 12)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)])
    pts = [(0, 2), (0, o.P - 2)]
    while len(pts) < 14:
        x = rng.randrange(o.P)
        rhs = (x * x * x + 4) % o.P
        if pow(rhs, (o.P - 1) // 2, o.P) == 1:
            pts.append((x, o.fp_sqrt(rhs)))
    for x, y in pts:
        out = (ctypes.c_uint32 * 24)()
        inf = ctypes.c_int()
        emu.emu_clear_cofactor(limbs(x), limbs(y), out, ctypes.byref(inf))
        want = o.ec_mul(o.FP, (x, y), o.H_EFF_G1)
        if want is None:
            assert inf.value == 1, (x, y)
        else:
            got = (sum(out[i] << (32 * i) for i in range(12)), sum(out[12 + i] << (32 * i) for i in range(12)))
            assert inf.value == 0 and got == want, (x, y)


def test_g1_mul_glv(emu):
    """curve.hpp g1_mul_glv (batch signing): the GLV split k mod r = k1 + k2 L
    (L = x^2 - 1) and the joint 2-bit windows equal the oracle's [k mod r]P at
    the split's edges, for keys >= r, and on random keys and points of G1."""
    import random

    import oracle.bls_oracle as o
    rng = random.Random(31)
    L = o.X * o.X - 1
    limbs = lambda v, n: (ctypes.c_uint32 * n)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)])
    ks = [0, 1, 2, 3, L - 1, L, L + 1, L * L, L * L + L, 1 << 128, o.R - 1, o.R, o.R + 1, (1 << 256) - 1]
    ks += [rng.randrange(1 << 256) for _ in range(6)] + [rng.randrange(o.R) for _ in range(6)]
    for j, k in enumerate(ks):
        pt = o.ec_mul(o.FP, o.G1_GEN, rng.randrange(1, o.R)) if j % 3 else o.G1_GEN
        out = (ctypes.c_uint32 * 24)()
        inf = ctypes.c_int()
        emu.emu_g1_mul_glv(limbs(pt[0], 12), limbs(pt[1], 12), limbs(k, 8), out, ctypes.byref(inf))
        want = o.ec_mul(o.FP, pt, k % o.R)
        if want is None:
            assert inf.value == 1, hex(k)
        else:
            got = (sum(out[i] << (32 * i) for i in range(12)), sum(out[12 + i] << (32 * i) for i in range(12)))
            assert inf.value == 0 and got == want, hex(k)


def test_g1_mul_glv32(emu):
    """curve.hpp g1_mul_glv32 (the distinct-key RLC's multiples r = a + b
    lambda, lambda = -x^2 the eigenvalue of phi(x, y) = (beta x, y)): Jacobian
    ladder with incomplete formulas over an affine table equals the oracle's
    [a - b x^2]P, at the digit edges (leading zero windows, a = 1, b = 0,
    all-ones digits) and on random 32-bit a (odd, as the mode draws them), b."""
    import random

    import oracle.bls_oracle as o
    rng = random.Random(37)
    limbs = lambda v: (ctypes.c_uint32 * 12)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)])
    ab = [(1, 0), (3, 0), (1, 1), (3, 3), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0xFFFFFFFF), (0xFFFFFFFF, 0),
          (0x80000001, 0x40000000), (5, 2)]
    ab += [(rng.getrandbits(32) | 1, rng.getrandbits(32)) for _ in range(10)]
    for j, (a, b) in enumerate(ab):
        pt = o.ec_mul(o.FP, o.G1_GEN, rng.randrange(1, o.R)) if j % 2 else o.G1_GEN
        out = (ctypes.c_uint32 * 24)()
        inf = ctypes.c_int()
        emu.emu_g1_mul_glv32(limbs(pt[0]), limbs(pt[1]), a, b, out, ctypes.byref(inf))
        want = o.ec_mul(o.FP, pt, (a - b * o.X * o.X) % o.R)
        got = (sum(out[i] << (32 * i) for i in range(12)), sum(out[12 + i] << (32 * i) for i in range(12)))
        assert inf.value == 0 and got == want, (hex(a), hex(b))


def test_miller_lane_of_records(emu, vectors):
    """staged.hpp miller_loopn_staged (k_miller_rr: four records per lane, one
    squaring per step for all, general lines for each) equals the product of
    the records' single-pair Miller loops, with every record taking part and
    with some left out (a record with a code or an identity point)."""
    import random
    rng = random.Random(41)
    keys = [bytes.fromhex(c["pk"]) for c in vectors["cases"] if c["code"] == 0]
    keys = list(dict.fromkeys(keys))[:4]
    assert len(keys) >= 2
    while len(keys) < 4:
        keys.append(keys[len(keys) % 2])
    msgs = b"".join(rng.randbytes(32) for _ in range(4))
    pks = b"".join(keys)
    for use in (0b1111, 0b0101, 0b1000, 0b0110):
        assert emu.emu_miller_rr_matches(msgs, pks, 4, use) == 1, bin(use)


def test_staged_matches_valuebased(emu, vectors):
    """The staged Fp12 code (LDS/HBM stores, final-exponentiation program) gives
    the same Gt as the value-based Fp12 code on every golden record."""
    for c in vectors["cases"][:12]:
        s, m, k = bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"])
        g1 = (ctypes.c_uint8 * 576)()
        g2 = (ctypes.c_uint8 * 576)()
        c1 = emu.emu_verify(s, m, len(m), k, g1)
        c2 = emu.emu_gt_valuebased(s, m, len(m), k, g2)
        assert c1 == c2 == c["code"], c["name"]
        if c1 in (0, 5):
            assert bytes(g1) == bytes(g2), c["name"]


def test_fp2_sqrt_against_oracle(emu):
    """The single-exponentiation Fp2 square root (field.hpp sqrt(fp2)) agrees
    with the oracle's square test on random squares and non-squares, including
    a0 + s non-square branches and real (a1 = 0) inputs."""
    import random

    import oracle.bls_oracle as o
    rng = random.Random(99)
    limbs = lambda v: (ctypes.c_uint32 * 12)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)])
    val = lambda arr: sum(arr[i] << (32 * i) for i in range(12))
    seen = {True: 0, False: 0}
    cases = [(rng.randrange(o.P), rng.randrange(o.P)) for _ in range(60)]
    cases += [o.f2_sqr((rng.randrange(o.P), rng.randrange(o.P))) for _ in range(60)]
    cases += [(rng.randrange(o.P), 0) for _ in range(10)]
    for a in cases:
        r0, r1 = (ctypes.c_uint32 * 12)(), (ctypes.c_uint32 * 12)()
        ok = bool(emu.emu_fp2_sqrt(limbs(a[0]), limbs(a[1]), r0, r1))
        assert ok == o.f2_is_square(a), a
        if ok:
            assert o.f2_sqr((val(r0), val(r1))) == tuple(x % o.P for x in a)
        seen[ok] += 1
    assert seen[True] > 50 and seen[False] > 20


def test_fp2_mul_lazy_bounds(emu):
    """The lazily reduced Fp2 product (field.hpp mul(fp2, fp2): one Montgomery
    reduction per component over combined column sums) and its digit-scaled
    form mul_scaled<3> at the extremes of its
    input contract -- components up to 2^384 - 1 (unreduced add_nr sums), 0,
    p, multiples of p -- and random values; output must be fully reduced."""
    import random

    import oracle.bls_oracle as o
    P, RINV = o.P, pow(2, -392, o.P)
    rng = random.Random(7)
    limbs = lambda v: (ctypes.c_uint32 * 12)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)])
    val = lambda arr: sum(arr[i] << (32 * i) for i in range(12))
    top = (1 << 384) - 1
    edge = [0, 1, P - 1, P, 2 * P - 1, 4 * P - 1, 8 * P - 1, top, top - 1, 1 << 383, (1 << 364) - 1]
    cases = [(rng.choice(edge), rng.choice(edge), rng.choice(edge), rng.choice(edge)) for _ in range(200)]
    cases += [(top, 0, top, top), (0, top, top, top), (top, top, top, top), (0, top, 0, top)]
    cases += [tuple(rng.randrange(1 << 384) for _ in range(4)) for _ in range(200)]
    for a0, a1, b0, b1 in cases:
        r0, r1 = (ctypes.c_uint32 * 12)(), (ctypes.c_uint32 * 12)()
        emu.emu_fp2_mul_mont(limbs(a0), limbs(a1), limbs(b0), limbs(b1), r0, r1)
        assert val(r0) == (a0 * b0 - a1 * b1) * RINV % P, (a0, a1, b0, b1)
        assert val(r1) == (a0 * b1 + a1 * b0) * RINV % P, (a0, a1, b0, b1)
        emu.emu_fp2_mul3_mont(limbs(a0), limbs(a1), limbs(b0), limbs(b1), r0, r1)   # mul_scaled<3>
        assert val(r0) == 3 * (a0 * b0 - a1 * b1) * RINV % P, (a0, a1, b0, b1)
        assert val(r1) == 3 * (a0 * b1 + a1 * b0) * RINV % P, (a0, a1, b0, b1)


def test_fp2_sqr_and_dot2_lazy_bounds(emu):
    """The lazily reduced Fp2 square (one unpack, digit-negated a1 = K - a1)
    and dot2 (a*b + c*d, one reduction per component) at the extremes of their
    input contract -- components up to 2^384 - 1, 0, p, multiples of p -- and
    random values; outputs must be the exact Montgomery products mod p."""
    import random

    import oracle.bls_oracle as o
    P, RINV = o.P, pow(2, -392, o.P)
    rng = random.Random(11)
    limbs = lambda v: (ctypes.c_uint32 * 12)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)])
    val = lambda arr: sum(arr[i] << (32 * i) for i in range(12))
    top = (1 << 384) - 1
    edge = [0, 1, P - 1, P, 2 * P - 1, 4 * P - 1, 8 * P - 1, top, top - 1, 1 << 383, (1 << 364) - 1]
    pick = lambda: rng.choice(edge) if rng.random() < 0.6 else rng.randrange(1 << 384)
    for _ in range(300):
        a0, a1 = pick(), pick()
        r0, r1 = (ctypes.c_uint32 * 12)(), (ctypes.c_uint32 * 12)()
        emu.emu_fp2_sqr_mont(limbs(a0), limbs(a1), r0, r1)
        assert val(r0) == (a0 * a0 - a1 * a1) * RINV % P, (a0, a1)
        assert val(r1) == (2 * a0 * a1) * RINV % P, (a0, a1)
    for _ in range(300):
        x = [pick() for _ in range(8)]
        buf = (ctypes.c_uint32 * 96)(*[(v >> (32 * i)) & 0xFFFFFFFF for v in x for i in range(12)])
        r0, r1 = (ctypes.c_uint32 * 12)(), (ctypes.c_uint32 * 12)()
        emu.emu_fp2_dot2_mont(buf, r0, r1)
        a0, a1, b0, b1, c0, c1, d0, d1 = x
        assert val(r0) == (a0 * b0 - a1 * b1 + c0 * d0 - c1 * d1) * RINV % P, x
        assert val(r1) == (a0 * b1 + a1 * b0 + c0 * d1 + c1 * d0) * RINV % P, x


def test_cpu_baseline_path_codes(vectors):
    """bench.py's cpu_baseline leg (tests/hostemu/cpu_verify.cpp, multi-threaded)
    gives the golden verdict codes for every fixed-size case."""
    src = os.path.join(HERE, "hostemu", "cpu_verify.cpp")
    lib = os.path.join(HERE, "hostemu", "libcpu_verify.so")
    hdr_dir = os.path.join(HERE, "..", "cess_amd", "csrc", "bls")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(hdr_dir, f)) for f in os.listdir(hdr_dir)])
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-DCESS_HOSTEMU", "-shared", "-fPIC", "-pthread", src,
                               "-o", lib])
    cpu = ctypes.CDLL(lib)
    cases = [c for c in vectors["cases"] if len(c["sig"]) == 96 and len(c["pk"]) == 192 and len(c["msg"]) == 64]
    assert len(cases) >= 4
    n = len(cases)
    sigs = b"".join(bytes.fromhex(c["sig"]) for c in cases)
    msgs = b"".join(bytes.fromhex(c["msg"]) for c in cases)
    pks = b"".join(bytes.fromhex(c["pk"]) for c in cases)
    codes = (ctypes.c_uint8 * n)()
    cpu.cpu_verify_batch(ctypes.c_uint64(n), sigs, msgs, ctypes.c_uint32(32), pks, codes, ctypes.c_int(4))
    assert list(codes) == [c["code"] for c in cases]


def test_fp_inv_safegcd(emu):
    """field.hpp inv(): Bernstein-Yang safegcd (37 x 30 divsteps) on Montgomery
    values anywhere in the redundant range [0, 2p) -- 0 and p (both zero) map
    to 0 -- against Python's modular inverse, including values with long runs
    of equal bits and the largest/smallest residues."""
    import random

    import oracle.bls_oracle as o
    P, RM = o.P, 1 << 392
    rng = random.Random(5)
    limbs = lambda v: (ctypes.c_uint32 * 12)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)])
    val = lambda arr: sum(arr[i] << (32 * i) for i in range(12))
    cases = [0, 1, 2, 3, P - 1, P, P + 1, 2 * P - 1, (P - 1) // 2, (P + 1) // 2, 1 << 380, (1 << 380) - 1,
             (1 << 381) - 1 - P, RM % P, pow(RM, -1, P)]
    cases += [(1 << k) % P for k in range(0, 381, 7)] + [((1 << k) - 1) % P for k in range(1, 381, 11)]
    cases += [rng.randrange(2 * P) for _ in range(400)]
    for am in cases:
        out = (ctypes.c_uint32 * 12)()
        emu.emu_fp_inv_mont(limbs(am), out)
        a = am * pow(RM, -1, P) % P          # the field element aR -> a
        want = 0 if a == 0 else pow(a, -1, P) * RM % P
        assert val(out) == want, hex(am)


def test_miller_pingpong_matches_inplace(emu, vectors):
    """The two-waves-per-SIMD Miller loop (bls/miller2.hpp: accumulator
    ping-ponging between two stores, streamed line multiplies and squaring)
    gives the same Fp12 as the one-wave in-place loop on the golden records."""
    n = 0
    for c in vectors["cases"][:24]:
        s, m, k = bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"])
        r = emu.emu_miller_pp_matches(s, m, len(m), k)
        assert r != 0, c["name"]
        n += r == 1
    assert n >= 8


def test_g2_subgroup_check_via_prepare(emu, vectors):
    """The kernels split G2Affine::from_compressed: k_decode_pk decodes the
    on-curve point, k_prepare checks psi(Q) == -[|x|]Q on the T its
    G2Prepared iteration ends with.  Same acceptance as the one-piece decode
    (and the oracle) on every golden key and on random on-curve points outside
    G2 (cofactor not cleared), including their negations."""
    import random

    import oracle.bls_oracle as o
    seen = set()
    for c in vectors["cases"]:
        k = bytes.fromhex(c["pk"])
        if len(k) != 96 or k in seen:
            continue
        seen.add(k)
        assert emu.emu_g2_accept(k, 1) == emu.emu_g2_accept(k, 0), c["name"]
    rng = random.Random(17)
    B2 = (4, 4)
    bad = 0
    while bad < 12:
        x = (rng.randrange(o.P), rng.randrange(o.P))
        rhs = o.f2_add(o.f2_mul(o.f2_sqr(x), x), B2)
        if not o.f2_is_square(rhs):
            continue
        y = o.f2_sqrt(rhs)
        for pt in ((x, y), (x, o.f2_neg(y))):
            enc = o.g2_to_compressed(pt)
            want = 1 if o.g2_in_subgroup(pt) else 0
            assert emu.emu_g2_accept(enc, 1) == want == emu.emu_g2_accept(enc, 0)
            bad += want == 0
    ok = [bytes.fromhex(c["pk"]) for c in vectors["cases"] if c["code"] == 0][:4]
    assert ok and all(emu.emu_g2_accept(k, 1) in (1, 2) for k in ok)


def test_g1_subgroup_check_jacobian(emu):
    """field/curve.hpp g1_is_torsion_free: one Jacobian ladder over x^2 with
    incomplete formulas agrees with the complete-formula form and with the
    oracle on G1 points, on random on-curve points outside G1 and on points of
    small order (3-torsion: y^2 = x^3 + 4 has the order-3 points (0, +-2))."""
    import random

    import oracle.bls_oracle as o
    rng = random.Random(23)
    limbs = lambda v: (ctypes.c_uint32 * 12)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)])
    pts = [(0, 2), (0, o.P - 2)]
    while len(pts) < 26:
        x = rng.randrange(o.P)
        rhs = (x * x * x + 4) % o.P
        if pow(rhs, (o.P - 1) // 2, o.P) != 1:
            continue
        pts.append((x, o.fp_sqrt(rhs)))
    g = o.G1_GEN if hasattr(o, "G1_GEN") else None
    if g:
        for k in (1, 2, 3, 12345, o.R - 1):
            pts.append(o.ec_mul(o.FP, g, k) if hasattr(o, "FP") else g)
    for (x, y) in pts:
        want = 1 if o.g1_in_subgroup((x, y)) else 0
        assert emu.emu_g1_torsion_free(limbs(x), limbs(y), 0) == want, (x, y)
        assert emu.emu_g1_torsion_free(limbs(x), limbs(y), 1) == want, (x, y)


VARIANT_FLAGS = ["-DCESS_MUL014_LOOP=1"]


@pytest.fixture(scope="module")
def emu_loops():
    """The host build of the same headers with the code-size loop forms of the
    sparse Fp12 products (mul014 / mul014_one as two-pass loops, the forms
    k_miller_rr is built with): staged.hpp CESS_MUL014_LOOP."""
    lib = os.path.join(HERE, "hostemu", "libemu_loops.so")
    hdr_dir = os.path.join(HERE, "..", "cess_amd", "csrc", "bls")
    newest = max(os.path.getmtime(os.path.join(hdr_dir, f)) for f in os.listdir(hdr_dir))
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(newest, os.path.getmtime(SRC)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCESS_HOSTEMU", *VARIANT_FLAGS, "-shared", "-fPIC", SRC,
                               "-o", lib])
    return ctypes.CDLL(lib)


@pytest.mark.parametrize("norm_pk", [0, 1])
def test_loop_forms_keep_codes_and_gt(emu_loops, vectors, norm_pk):
    """The loop forms compute the same Miller loop and final exponentiation:
    golden codes and Gt bytes, with per-signature and normalised key lines."""
    old = emu_loops.emu_set_norm_pk(norm_pk)
    try:
        for c in vectors["cases"]:
            s, m, k = bytes.fromhex(c["sig"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["pk"])
            gt = (ctypes.c_uint8 * 576)()
            code = emu_loops.emu_verify(s, m, len(m), k, gt)
            assert code == c["code"], c["name"]
            if "gt" in c:
                assert bytes(gt).hex() == c["gt"], c["name"]
    finally:
        emu_loops.emu_set_norm_pk(old)


def test_subfield_miller_value_degenerate_chain(emu):
    """Secret keys 1 and r - 1 (key +-G2, signature +-H(m)): the Miller value
    lies in Fp6, the easy part gives m = 1 and the hard part's compressed
    powers are all zero -- the staged program's Granger-Scott fallback
    (bls/staged.hpp cyc_chain) must still return Gt = 1, code 0, as the oracle
    (and the value-based code) do (tests/test_gpu_subfield.py on the GPU)."""
    import oracle.bls_oracle as o
    one = o.gt_to_bytes(o.F12_ONE)
    for msg in (b"", b"subfield miller value"):
        h = o.hash_to_g1(msg)
        for sig_pt, pk_pt in ((h, o.G2_GEN), (o.ec_neg(o.FP, h), o.ec_neg(o.FP2, o.G2_GEN))):
            s, k = o.g1_to_compressed(sig_pt), o.g2_to_compressed(pk_pt)
            g1 = (ctypes.c_uint8 * 576)()
            g2 = (ctypes.c_uint8 * 576)()
            assert emu.emu_verify(s, msg, len(msg), k, g1) == 0
            assert emu.emu_gt_valuebased(s, msg, len(msg), k, g2) == 0
            assert bytes(g1) == one and bytes(g2) == one
