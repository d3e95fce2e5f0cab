"""CPU: bench.py's --dump-outputs writer and the --full switch (no GPU: the
helpers are called on arrays made here).

* verdict_bits unpacks the bitmap as include/cess_bls.h defines it: bit
  (i % 64) of word i / 64, LSB first.
* dump_outputs writes float32 DIR/<name>.npy; bytes and bits survive exactly;
  arrays past their share of the 64 MB budget are cut to the same seeded
  sample on every call, and the whole dump stays within the budget.
* --full is off by default and --dump-outputs takes a directory.
"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_outputs_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_verdict_bits_order(bench):
    words = np.array([0b1011, 1 << 63, 1], dtype=np.uint64)
    bits = bench.verdict_bits(words, 130)
    assert bits.shape == (130,)
    assert set(np.flatnonzero(bits)) == {0, 1, 3, 127, 128}


def test_dump_small_arrays_exact(bench, tmp_path):
    codes = (np.arange(1000) % 6).astype(np.uint8)
    bits = (codes == 0).astype(np.uint8)
    bench.dump_outputs(str(tmp_path / "d"), {"codes": codes, "verdict_bits": bits})
    c = np.load(tmp_path / "d" / "codes.npy")
    v = np.load(tmp_path / "d" / "verdict_bits.npy")
    assert c.dtype == np.float32 and v.dtype == np.float32
    assert (c == codes).all() and (v == bits).all()


def test_budget_is_64_mb(bench):
    assert bench.DUMP_BUDGET_BYTES == 64 << 20


def test_dump_large_array_is_a_fixed_sample_within_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 16)   # the rule at a small size
    cap = bench.DUMP_BUDGET_BYTES // 4
    big = (np.arange(cap + 12345, dtype=np.uint32) % 251).astype(np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"signatures": big})
    a = np.load(tmp_path / "a" / "signatures.npy")
    b = np.load(tmp_path / "b" / "signatures.npy")
    assert a.shape == (cap,) and a.nbytes <= bench.DUMP_BUDGET_BYTES
    assert (a == b).all()
    # a sample of the array's own elements, in index order
    pick = np.sort(np.random.default_rng((0xD0, big.size)).choice(big.size, size=cap, replace=False))
    assert (a == big[pick]).all()


def test_full_is_off_by_default(bench, monkeypatch):
    monkeypatch.delenv("CESS_BENCH_ARGV", raising=False)
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "out"
