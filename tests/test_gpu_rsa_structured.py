"""GPU: RSA keys made of Mersenne primes, end to end (tests/rsa_structured_keys.py;
the CPU half is tests/test_rsa_primitives.py).

An all-ones modulus (ninv = 1), products with long zero and one runs
(ninv = 2^28 - 1), a prime modulus, a 92-bit key, exponents 2, 65537, 2^32 + 1
and 0x1fffffffd (every bit but one multiplies): valid signatures, tampered
messages, s at 0, 1, n - 1, n, n + 1, 2^(8k) - 1 and all ones, block type 02
and a missing separator, through rsa_verify_batch, rsa_verify_batch_device and
verify_rsa.  Every code equals oracle.verify_code; every key has both a 0 and
a 4, so a kernel that fails everything on such a modulus cannot pass."""
import numpy as np
import pytest

from oracle import rsa_oracle as o

import rsa_structured_keys as sk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def structured():
    keys, rows = sk.structured()
    table = [(key, e) for key in keys for e in sk.EXPONENTS]      # one table entry per (modulus, e)
    return keys, rows, table


def ders(table):
    return [o.encode_spki(key.n, e) for key, e in table]


def host_codes(c, idx, rows):
    return list(c.rsa_verify_batch(idx, [r.msg for r in rows], [r.sig for r in rows]))


def device_codes(c, idx, rows):
    S, M = b"".join(r.sig for r in rows), b"".join(r.msg for r in rows)
    so = np.cumsum([0] + [len(r.sig) for r in rows]).astype(np.uint64)
    mo = np.cumsum([0] + [len(r.msg) for r in rows]).astype(np.uint64)
    d = [c.to_device(np.array(idx, dtype=np.uint32)), c.to_device(S), c.to_device(so), c.to_device(M if M else b"\0"),
         c.to_device(mo)]
    dc = c.device_alloc(len(rows))
    try:
        c.rsa_verify_batch_device(len(rows), d[0], d[1], d[2], d[3], d[4], dc)
        c.synchronize()
        return list(c.from_device(dc, len(rows)))
    finally:
        for p in d + [dc]:
            c.device_free(p)


def context():
    from cess_amd import bls
    return bls.Context(max_batch=4096)


def test_gpu_structured_all_rows(structured):
    """every row, all size classes in one batch, through the host-buffer and
    the device-resident entry points"""
    keys, rows, table = structured
    where = {(id(key), e): j for j, (key, e) in enumerate(table)}
    idx = [where[(id(r.key), r.e)] for r in rows]
    want = [r.code for r in rows]
    assert len(rows) <= 4096
    c = context()
    try:
        assert c.rsa_keys_load(ders(table)) == [0] * len(table)
        got_h = host_codes(c, idx, rows)
        got_d = device_codes(c, idx, rows)
    finally:
        c.close()
    for got in (got_h, got_d):
        bad = [(r.key.name, hex(r.e), r.what, g, r.code) for r, g in zip(rows, got) if g != r.code]
        assert not bad, bad[:8]
        for key in keys:
            assert {0, 4} <= {g for r, g in zip(rows, got) if r.key is key}, key.name
    assert set(want) == {0, 2, 3, 4}


def test_gpu_structured_verify_rsa(structured):
    """verify_rsa (the single-key table and key_row's R^2 on these moduli):
    one valid and one tampered row per key and exponent"""
    keys, rows, table = structured
    c = context()
    try:
        for key, e in table:
            mine = [r for r in rows if r.key is key and r.e == e]
            good = next(r for r in mine if r.code == 0)
            tampered = [r for r in mine if r.code == 4]      # a changed message byte where the key has one
            bad = next((r for r in tampered if r.what in ("first byte", "last byte")), tampered[0])
            der = o.encode_spki(key.n, e)
            assert c.verify_rsa(der, good.msg, good.sig) is True, (key.name, hex(e))
            assert c.verify_rsa(der, bad.msg, bad.sig) is False, (key.name, hex(e))
    finally:
        c.close()


def cycled(rows_by_key, per_key):
    """(idx, rows): per_key records of each key, its rows repeated in order"""
    idx, out = [], []
    for j, mine in enumerate(rows_by_key):
        for i in range(per_key):
            idx.append(j)
            out.append(mine[i % len(mine)])
    order = np.random.RandomState(5).permutation(len(out))
    return [idx[i] for i in order], [out[i] for i in order]


@pytest.mark.parametrize("extra_keys", [0, 20], ids=["k_rsa_verify_2048u", "k_rsa_verify_2048"])
@pytest.mark.parametrize("e", sk.EXPONENTS, ids=hex)
def test_gpu_structured_2048_kernels(structured, e, extra_keys):
    """An all-ones key (M1279) and a two-factor key (M1279 M607) alone in the
    table, 260 records each: at most 4096 keys with at least 256 records per
    key take the key-sorted, wave-padded lists and k_rsa_verify_2048u (the
    modulus in SGPRs); 20 unused extra keys in the table and the same records
    take the unsorted lists and k_rsa_verify_2048 (the routing of
    test_rsa.py test_gpu_device_batch_many)."""
    keys, rows, _ = structured
    two = [next(k for k in keys if k.name == nm) for nm in ("M1279", "M1279x607")]
    assert all(k.L == 74 for k in two)
    by_key = [[r for r in rows if r.key is k and r.e == e] for k in two]
    idx, recs = cycled(by_key, 260)
    assert len(recs) >= 256 * len(two) and len(recs) < 256 * (len(two) + 20)
    table = [(k, e) for k in two]
    c = context()
    try:
        assert c.rsa_keys_load(ders(table) + ders(table[:1]) * extra_keys) == [0] * (2 + extra_keys)
        got_h = host_codes(c, idx, recs)
        got_d = device_codes(c, idx, recs)
    finally:
        c.close()
    want = [r.code for r in recs]
    assert got_h == want and got_d == want
    for j in (0, 1):
        assert {0, 2, 4} <= {g for i, g in zip(idx, got_d) if i == j}


@pytest.mark.parametrize("size", [1, 65, 257])
@pytest.mark.parametrize("name", ["M521", "M1279x607", "M2203x1279"])
def test_gpu_structured_batch_sizes(structured, name, size):
    """1, 65 and 257 records of one structured key alone in the table:
    k_rsa_verify_1024; k_rsa_verify_2048 (1 and 65) and k_rsa_verify_2048u
    (257 >= 256 records per key); k_rsa_verify_big"""
    keys, rows, _ = structured
    key = next(k for k in keys if k.name == name)
    e = (1 << 32) + 1
    mine = [r for r in rows if r.key is key and r.e == e]
    mine.sort(key=lambda r: r.code)          # the single record is a valid signature
    idx, recs = [0] * size, [mine[i % len(mine)] for i in range(size)]
    c = context()
    try:
        assert c.rsa_keys_load(ders([(key, e)])) == [0]
        got_h = host_codes(c, idx, recs)
        got_d = device_codes(c, idx, recs)
    finally:
        c.close()
    want = [r.code for r in recs]
    assert got_h == want and got_d == want
    assert want[0] == 0 and (size == 1 or 4 in want)
