"""CPU: the Makefile's CHAIN_FLAGS still put every Montgomery column on one mad
chain.

The kernel units are compiled with LLVM's IR-level Reassociate pass switched
off by name (cess_amd/csrc/Makefile, CHAIN_FLAGS): with the pass on, each
column's a_i*b_j products are summed first and the carried `acc >> 28` last, so
every column costs a v_lshl_add_u64 to join two mad chains.  A toolchain that
no longer knows the pass name ignores the option without a word and compiles
the old code; nothing else would show it.  tools/chain_probe.hip (one bls::mul
and one bls::sqr per thread) is compiled for gfx950 with the flags the Makefile
gives k_decode, and again with CHAIN_FLAGS empty:
  * no v_lshl_add_u64 in either probe kernel;
  * no more v_mad_u64_u32 than without CHAIN_FLAGS plus 1 % (the pass also
    folds a few unrelated products, 696 -> 698 in the probe)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cess_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _mix(tmp_path, tag, makevars):
    import isa_mix
    flags = isa_mix.unit_flags("k_decode", makevars)
    out = str(tmp_path / f"probe_{tag}.s")
    isa_mix.compile_to_asm(os.path.join(ROOT, "tools", "chain_probe.hip"), flags, out)
    counts, notes = isa_mix.mix_of_asm(out)
    kernels = {name: c for name, c, _ in isa_mix.rows(counts, notes)}
    assert sorted(kernels) == ["k_probe_mul", "k_probe_sqr"], sorted(kernels)
    return flags, kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not in this image")
def test_columns_on_one_mad_chain(tmp_path):
    flags, new = _mix(tmp_path, "chain", [])
    base_flags, base = _mix(tmp_path, "base", ["CHAIN_FLAGS="])
    assert flags != base_flags, "k_decode no longer takes CHAIN_FLAGS"
    for k in ("k_probe_mul", "k_probe_sqr"):
        print(k, "chain", new[k], "base", base[k])
        assert new[k]["v_mad_u64_u32"] >= 14 * 14      # the probe did compile a reduction's m_i * p_j products
        assert new[k]["v_lshl_add_u64"] == 0, (k, new[k])
        assert new[k]["v_mad_u64_u32"] <= 1.01 * base[k]["v_mad_u64_u32"], (k, new[k], base[k])
