"""gcnk_hubfactor_gc1_f32 on hand-built block records: the item loop at the
per-row item counts the graph-built tests do not pin.

The kernel reads a row's A_H items ahead of their use (the next item's word
while the current item's S_T rows are in flight, the index clamped to the row's
last item).  What can go wrong in any such loop is a slot that uses a word it
must not: the next row's item, or the unused tail of the record.  So the rows
here have 0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17 items in one block (every count
around a read-ahead depth or group size of 2 to 4), empty rows next to long
ones and at the block's end, one row of 200 items, and the unused tail of every
record is NaN bits in both the hub and the value word -- a slot that used a
tail word would give a NaN or miss the float64 result.  F = 200, 52 and 36
also take the three ways the kernel deals its MFMA n-tiles over the waves (all
slots real or one short; some waves with no real tile).

Operands are made by hand (block record layout of csrc/factor.hip: 33 item
offsets, 3 pad words, 32 output row ids with -1 past M, then int2 {hub, value}
items; rec_words the common stride, a multiple of 4), so the expected values
come from the same arrays in float64 numpy and no row is left out.
"""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

M = 70                       # three 32-row blocks, the last with 6 real rows
ROWS, REC_ROW, REC_HEAD = 32, 36, 68
COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 0]   # ..., 17, 0, 0, 1, ... down a block
LONG_POS, LONG_ITEMS = 32 + 13, 200               # the long row: middle block, followed by an empty row
GUARD = 8                    # sentinel rows before and after the outputs
SENTINEL = -12345.0
NAN_BITS = np.int32(0x7FC00000)
K0 = 3


def _operands(nhub, Kc, F, P):
    rng = np.random.default_rng(1000 * nhub + 10 * Kc + F + P)
    perm = rng.permutation(M)                      # position in block order -> output row
    assert not np.array_equal(perm, np.arange(M))
    nblk = (M + ROWS - 1) // ROWS
    counts = np.array([COUNTS[(p % ROWS) % len(COUNTS)] for p in range(nblk * ROWS)])
    counts[M:] = 0                                 # rows past M hold nothing
    counts[LONG_POS] = LONG_ITEMS
    counts[LONG_POS + 1] = 0                       # an empty row right after the long one
    counts[2 * ROWS - 1] = 0                       # and one as that block's last row
    hubs = [rng.integers(0, nhub, c) for c in counts]             # repeated hubs allowed
    vals = [rng.uniform(-1.0, 1.0, c).astype(np.float32) for c in counts]
    per_block = counts.reshape(nblk, ROWS).sum(1)
    rec_words = (REC_HEAD + 2 * int(per_block.max()) + 3) // 4 * 4 + 4   # every record keeps a tail
    rec = np.full((nblk, rec_words), NAN_BITS, np.int32)
    for b in range(nblk):
        off = np.concatenate([[0], np.cumsum(counts[b * ROWS:(b + 1) * ROWS])])
        rec[b, :ROWS + 1] = off
        rec[b, ROWS + 1:REC_ROW] = 0
        ids = np.full(ROWS, -1, np.int64)
        real = min(ROWS, M - b * ROWS)
        ids[:real] = perm[b * ROWS:b * ROWS + real]
        rec[b, REC_ROW:REC_HEAD] = ids
        h = np.concatenate(hubs[b * ROWS:(b + 1) * ROWS]).astype(np.int32)
        v = np.concatenate(vals[b * ROWS:(b + 1) * ROWS]).astype(np.float32)
        rec[b, REC_HEAD:REC_HEAD + 2 * len(h):2] = h
        rec[b, REC_HEAD + 1:REC_HEAD + 2 * len(h):2] = v.view(np.int32)
    # U's leading dimension: a multiple of 4 (rows staged in LDS) or odd (fragments loaded directly)
    ldu = Kc + 2 if nhub == 7 else Kc + 1
    U = np.zeros((M, ldu), np.float32)
    U[:, :Kc] = rng.standard_normal((M, Kc)) * 0.3
    U[:, Kc:] = np.nan                             # columns past Kc are not the kernel's to read into Z
    W1 = rng.standard_normal((K0 + Kc + 5, F)).astype(np.float32)
    S = rng.standard_normal((nhub, F)).astype(np.float32)
    b1 = rng.standard_normal(F).astype(np.float32)
    W2 = rng.standard_normal((F, P)).astype(np.float32)
    # float64 from the same arrays, rows in output order
    Z = np.zeros((M, F))
    UW = U[:, :Kc].astype(np.float64) @ W1[K0:K0 + Kc].astype(np.float64)
    for pos in range(M):
        z = UW[pos].copy()
        for hcol, val in zip(hubs[pos], vals[pos]):
            z += np.float64(val) * S[hcol].astype(np.float64)
        Z[perm[pos]] = z
    return dict(rec=rec, rec_words=rec_words, ldu=ldu, U=U, W1=W1, S=S, b1=b1, W2=W2, Z=Z)


@pytest.mark.parametrize("P", [8, 20])
@pytest.mark.parametrize("F", [200, 52, 36])
@pytest.mark.parametrize("Kc", [50, 70])
@pytest.mark.parametrize("nhub", [7, 50])
def test_hubfactor_item_counts(nhub, Kc, F, P):
    """H1 and S2 of every one of the M rows against float64, for every
    non-dropout epilogue with and without the H1 store, each launch right after
    an LDS fill with NaN bits; finite outputs; S2 the same bits with and without
    the H1 store; nothing written outside the rows the record names."""
    o = _operands(nhub, Kc, F, P)
    lib = _lib.load()
    dev = {k: torch.from_numpy(o[k]).to(DEV) for k in ("rec", "U", "W1", "S", "b1", "W2")}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    W2d = o["W2"].astype(np.float64)

    def launch(epi, store_h1):
        Hbuf = torch.full((M + 2 * GUARD, F), SENTINEL, device=DEV)
        Cbuf = torch.full((M + 2 * GUARD, P), SENTINEL, device=DEV)
        H1, S2 = Hbuf[GUARD:GUARD + M], Cbuf[GUARD:GUARD + M]
        _lib.check(lib.gcnk_debug_poison_lds(0xFFFFFFFF, stream), "gcnk_debug_poison_lds")
        _lib.check(lib.gcnk_hubfactor_gc1_f32(
            M, F, Kc, nhub, P, p(dev["U"]), o["ldu"], p(dev["W1"]), F, K0, p(dev["S"]), F, p(dev["rec"]),
            o["rec_words"], p(dev["b1"]), epi, None, 0, 1.0, 1.0, 0, 0, None, p(dev["W2"]), P,
            p(H1) if store_h1 else None, F, p(S2), P, stream), "gcnk_hubfactor_gc1_f32")
        torch.cuda.synchronize()
        # the -1 row ids and everything else the record does not name: untouched
        for buf in (Hbuf, Cbuf):
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + M:] == SENTINEL).all())
        if not store_h1:
            assert bool((Hbuf == SENTINEL).all())
        return H1, S2

    for epi in (_lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_RELU):
        want = o["Z"] if epi == _lib.EPI_NONE else o["Z"] + o["b1"].astype(np.float64)
        if epi == _lib.EPI_BIAS_RELU:
            want = np.maximum(want, 0.0)
        want2 = want @ W2d
        H1, S2 = launch(epi, True)
        _, S2n = launch(epi, False)
        assert bool(torch.isfinite(H1).all()) and bool(torch.isfinite(S2).all()), epi
        err1 = np.abs(H1.double().cpu().numpy() - want).max()
        err2 = np.abs(S2.double().cpu().numpy() - want2).max()
        tol1, tol2 = 2e-5 * max(1.0, np.abs(want).max()), 2e-5 * max(1.0, np.abs(want2).max())
        print(f"epi {epi}: H1 max err {err1:.3e} (tol {tol1:.3e}), S2 max err {err2:.3e} (tol {tol2:.3e})")
        assert err1 <= tol1, (epi, err1, tol1)
        assert err2 <= tol2, (epi, err2, tol2)
        assert torch.equal(S2n, S2), epi
