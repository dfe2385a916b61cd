"""Pin oracle/hash_ref.py, the numpy restatement of the device dropout mask
(include/gcnk.h, GCNK_EPI_BIAS_RELU_HASH), without a GPU: known answers, a
second writing in C (oracle/spmm_ref.c, oracle_hash_u24), and the statistics a
dropout mask must have at fixed seeds.  tests/test_hash_dropout.py then holds
every kernel that draws the mask to this oracle, element by element.

The z bounds are conditions on the spec, not measurements: a keep count of N
independent draws at rate p has standard deviation sqrt(N p (1 - p)); |z| <= 4
for one count, 5 / 5.5 for the maximum over 200 columns / 7,724 rows (the
two-sided tail of a normal at 5.5 times 7,724 rows is 3e-4).
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import csr_ref, hash_ref

KNOWN = [
    (0, 0, 130277),
    (123, 0, 6665104),
    (123, 1, 10450060),
    (50494, 1544800, 1597159),
    (0xDEADBEEF12345678, 2**32 - 1, 15404805),
    (0xDEADBEEF12345678, 2**32, 4698292),
    (5, 2**64 - 1, 1056652),
]


@pytest.mark.parametrize("seed,idx,want", KNOWN)
def test_known_answers(seed, idx, want):
    assert int(hash_ref.hash_u24(seed, np.uint64(idx))[0]) == want
    u = hash_ref.hash_uniform(seed, np.array([idx], np.uint64))
    assert u.dtype == np.float32 and float(u[0]) == want / 16777216.0


def test_keep_mask_known_answer():
    """The index crosses 2^32 inside the matrix and seed_hi != 0."""
    m = hash_ref.keep_mask(2**40 + 3, 2**32 - 1000, 0, 64, 52, 52, 0.5)
    assert m.shape == (64, 52) and m.dtype == np.bool_
    assert int(m.sum()) == 1655
    assert "".join("1" if b else "0" for b in m[0, :16]) == "0011110110110100"


def test_keep_mask_is_the_hash_of_base_plus_offset_plus_r_ldm_plus_c():
    """keep_mask against a scalar Python-int loop of the contract (index sum
    modulo 2^64: base + offset past 2^64, and rows that wrap)."""
    seed, base, offset, M, F, ldm = 0xDEADBEEF12345678, 2**64 - 40, 2**64 - 33, 9, 7, 19
    got = hash_ref.keep_mask(seed, base, offset, M, F, ldm, 0.37)
    for r in range(M):
        for c in range(F):
            idx = (base + offset + r * ldm + c) % 2**64
            u = hash_ref.hash_uniform(seed, np.uint64(idx))[0]
            assert bool(got[r, c]) == bool(u < np.float32(0.37)), (r, c)
    # base and offset only enter through their sum
    assert np.array_equal(got, hash_ref.keep_mask(seed, 0, (base + offset) % 2**64, M, F, ldm, 0.37))


def _c_hash():
    assert os.path.exists(csr_ref.LIB_PATH), "oracle/liboracle.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(csr_ref.LIB_PATH)
    lib.oracle_hash_u24.restype = None
    lib.oracle_hash_u24.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    return lib.oracle_hash_u24


def test_c_writing_equals_numpy_on_indices_straddling_2_32_and_2_64():
    fn = _c_hash()
    n = 25_000
    run = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng(0)
    idx = np.concatenate([
        np.uint64(2**32 - n // 2) + run,                      # across 2^32
        np.uint64(2**64 - n // 2) + run,                      # across 2^64 (wraps to 0, 1, ...)
        rng.integers(0, 2**64, n, dtype=np.uint64),           # anywhere
        np.uint64(7 * 2**32 - n // 2) + run,                  # a carry into a non-zero high word
    ])
    assert idx.size == 100_000 and idx[n + n // 2] == 0 and idx[n // 2] == 2**32
    for seed in (0, 123, 0xDEADBEEF12345678, 2**64 - 1, 2**40 + 3):
        out = np.empty(idx.size, np.uint32)
        fn(seed, idx.ctypes.data, idx.size, out.ctypes.data)
        assert np.array_equal(out, hash_ref.hash_u24(seed, idx)), seed
    for seed, i, want in KNOWN:
        one, out = np.array([i], np.uint64), np.empty(1, np.uint32)
        fn(seed, one.ctypes.data, 1, out.ctypes.data)
        assert int(out[0]) == want


def _z(count, n, p):
    return (np.asarray(count, np.float64) - n * p) / np.sqrt(n * p * (1.0 - p))


@pytest.fixture(scope="module", params=[50494, 99346, 0, 2**64 - 1])
def step_masks(request):
    """The masks of steps 0..3 of an R8-sized hidden layer (base = t * M * F)."""
    M, F = 7724, 200
    seed = request.param
    return seed, [hash_ref.keep_mask(seed, t * M * F, 0, M, F, F, 0.5) for t in range(4)]


def test_keep_rates_overall_per_column_and_per_row(step_masks):
    seed, masks = step_masks
    m = masks[0]
    M, F = m.shape
    z_all = float(_z(m.sum(), M * F, 0.5))
    z_col = float(np.abs(_z(m.sum(0), M, 0.5)).max())
    z_row = float(np.abs(_z(m.sum(1), F, 0.5)).max())
    print(f"seed {seed}: overall z {z_all:.2f}, columns max |z| {z_col:.2f}, rows max |z| {z_row:.2f}")
    assert abs(z_all) <= 4
    assert z_col <= 5
    assert z_row <= 5.5


def test_successive_steps_draw_independent_masks(step_masks):
    """Two independent masks at keep 0.5 agree on each element with probability 1/2."""
    seed, masks = step_masks
    for t in range(3):
        z = float(_z((masks[t] == masks[t + 1]).sum(), masks[t].size, 0.5))
        print(f"seed {seed}: steps {t}/{t + 1} agreement z {z:.2f}")
        assert abs(z) <= 4


def test_adjacent_elements_are_independent(step_masks):
    seed, masks = step_masks
    m = masks[0]
    zh = float(_z((m[:, 1:] == m[:, :-1]).sum(), m[:, 1:].size, 0.5))
    zv = float(_z((m[1:] == m[:-1]).sum(), m[1:].size, 0.5))
    print(f"seed {seed}: horizontal z {zh:.2f}, vertical z {zv:.2f}")
    assert abs(zh) <= 4 and abs(zv) <= 4


def test_keep_prob_edges_and_other_rates():
    assert hash_ref.keep_mask(7, 0, 0, 2000, 64, 64, 1.0).all()
    assert not hash_ref.keep_mask(7, 0, 0, 2000, 64, 64, 0.0).any()
    for keep in (0.9, 0.1):
        m = hash_ref.keep_mask(7, 0, 0, 2000, 64, 64, keep)
        z = float(_z(m.sum(), m.size, keep))
        print(f"keep {keep}: z {z:.2f}")
        assert abs(z) <= 4
