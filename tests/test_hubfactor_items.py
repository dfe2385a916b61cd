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

Operands are made by hand (tests/hubfactor_cases.py operands(), shared with
tests/test_hubfactor_routes.py; the block records packed by
tests/hub_records.py), so the expected values come from the same arrays in
float64 numpy and no row is left out.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubfactor_cases as hc  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

M, K0 = hc.M, hc.K0          # three 32-row blocks, the last with 6 real rows
GUARD = 8                    # sentinel rows before and after the outputs
SENTINEL = -12345.0


def _operands(nhub, Kc, F, P):
    # U's leading dimension: a multiple of 4 (rows staged in LDS) or odd (fragments loaded directly)
    return hc.operands(nhub, Kc, F, P, Kc + 2 if nhub == 7 else Kc + 1)


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
