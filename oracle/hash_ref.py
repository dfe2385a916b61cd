"""ORACLE (test infrastructure only): the device dropout mask, restated in numpy.

Written from the contract of GCNK_EPI_BIAS_RELU_HASH in include/gcnk.h --
element (r, c) is kept iff hash(seed, base + offset + r*ldm + c) < keep_prob --
and the three mixing rounds of the counter-based hash (a lowbias32-style
avalanche: xor-shift 16, multiply 0x7feb352d, xor-shift 15, multiply
0x846ca68b, xor-shift 16):

    h = mix(lo32(idx) ^ lo32(seed))
    h = mix(h ^ hi32(idx) ^ hi32(seed))
    h = mix(h + 0x9e3779b9)
    u = (h >> 8) * 2^-24                      (float32, exact)

Every 32-bit step is modulo 2^32 and the index sum is modulo 2^64.  The
arithmetic is carried in uint64 and masked, so nothing depends on how numpy
treats an overflowing uint32.  Imports nothing from the product package.
oracle/spmm_ref.c holds a second writing (oracle_hash_u24) that
tests/test_hash_ref.py compares with this one.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_M64 = (1 << 64) - 1


def _mix32(x):
    """One avalanche round on uint64 arrays holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def hash_u24(seed, idx):
    """h >> 8 (the 24 bits the uniform is made of) as uint32, for a 64-bit
    ``seed`` (any Python int, taken modulo 2^64) and uint64 ``idx`` (array or
    scalar)."""
    seed = int(seed) & _M64
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    h = _mix32((idx & _M32) ^ lo)
    h = _mix32(h ^ (idx >> np.uint64(32)) ^ hi)
    h = _mix32((h + np.uint64(0x9E3779B9)) & _M32)
    return (h >> np.uint64(8)).astype(np.uint32)


def hash_uniform(seed, idx):
    """The uniform in [0, 1) of (seed, idx): (h >> 8) * 2^-24 as float32."""
    return hash_u24(seed, idx).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_mask(seed, base, offset, M, F, ldm, keep_prob):
    """bool [M, F]: element (r, c) is kept iff
    hash_uniform(seed, base + offset + r*ldm + c) < float32(keep_prob), the
    index sum modulo 2^64.  ``ldm`` is the element stride between rows (the
    kernels take 0 as F; here it is explicit)."""
    start = (int(base) + int(offset)) & _M64
    rows = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(int(ldm) & _M64)
    cols = np.arange(F, dtype=np.uint64)[None, :]
    idx = (rows + cols + np.uint64(start)).reshape(-1)      # uint64 arrays wrap modulo 2^64
    u = hash_uniform(seed, idx).reshape(M, F)
    return u < np.float32(keep_prob)
