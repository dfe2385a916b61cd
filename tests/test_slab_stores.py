"""The small-M GEMM's slab partials, stored write-through through a buffer
resource over each slab (csrc/gemm.hip: a row past M lies past the resource, a
column past N is sent there), and the two kernels that sum them.

Every remainder of M mod 4, a last 16-row tile of 1 and 2 rows (multiplied on
the VALU) against a third and fourth MFMA tile, the full height; N below one
n-tile, with a partial second n-tile, and with a last column group whose second
n-tile is all padding; K ragged against 4, 16 and 256.  The workspace holds NaN
bits before every call (a word read but never written shows in the result) and
one more slab than the kernel writes; a sentinel guard follows the
gcnk_gemm_workspace_bytes bytes, and another surrounds C.  The buffer reduce
(C on 16-byte rows) and the pointer reduce (ldc % 4 != 0, or C one float past a
16-byte boundary) must agree bit for bit, for every epilogue.
"""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.0
GUARD = 64

ROWS = (1, 2, 3, 4, 5, 16, 17, 18, 19, 47, 50, 64)
EPILOGUES = ("none", "bias", "bias_relu", "mask_pos", "bias_null")
# C: (ldc - N, floats past a 16-byte boundary): contiguous and strided on 16-byte rows (the buffer reduce), rows
# of no multiple of 4 floats and a base off the boundary (the pointer reduce)
C_LAYOUTS = ((0, 0), (8, 0), (3, 0), (0, 1))


def _slabs(K):
    return (K + 255) // 256          # the small-M kernel's slabs: 8 waves x 32 k


def _slab_bytes(M, N, split):
    return split * M * N * 4         # [split][M][N] floats


def _epilogue(name, M, N, g):
    bias = torch.randn(N, generator=g) if name in ("bias", "bias_relu") else None
    R = torch.relu(torch.randn(M, N, generator=g)) if name == "mask_pos" else None
    code = {"none": _lib.GEMM_EPI_NONE, "bias": _lib.GEMM_EPI_BIAS, "bias_null": _lib.GEMM_EPI_BIAS,
            "bias_relu": _lib.GEMM_EPI_BIAS_RELU, "mask_pos": _lib.GEMM_EPI_MASK_POS}[name]

    def apply(ref):
        if bias is not None:
            ref = ref + bias.double().numpy()
        if name == "bias_relu":
            ref = np.maximum(ref, 0.0)
        if name == "mask_pos":
            ref = np.where(R.numpy() > 0, 2.0 * ref, 0.0)
        return ref

    return (bias.to(DEV) if bias is not None else None, code, R.to(DEV) if R is not None else None,
            2.0 if name == "mask_pos" else 1.0), apply


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _gemm(Ad, Bd, M, N, K, split, epi, ldc_pad, shift):
    """One gcnk_gemm_f32 call on the small-M route into a guarded C and a
    NaN-filled, guarded workspace; returns C's values after checking both guards."""
    lib = _lib.load()
    bias, code, R, scale = epi
    wsb = lib.gcnk_gemm_workspace_bytes(M, N, K, split)
    assert wsb == _slab_bytes(M, N, split)
    ws = torch.full((wsb // 4 + GUARD,), float("nan"), device=DEV)
    ws[wsb // 4:] = SENTINEL
    ldc = N + ldc_pad
    buf = torch.full((GUARD + M * ldc + GUARD,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    lo = GUARD + shift
    out = buf[lo:lo + M * ldc].view(M, ldc)[:, :N]
    rc = lib.gcnk_gemm_f32(0, 0, M, N, K, _ptr(Ad), Ad.stride(0), _ptr(Bd), Bd.stride(0), _ptr(out), ldc, _ptr(bias),
                           code, _ptr(R), R.stride(0) if R is not None else 0, scale, split, _ptr(ws), wsb,
                           _lib.stream(torch.device(DEV, torch.cuda.current_device())))
    _lib.check(rc, "gcnk_gemm_f32")
    assert bool((ws[wsb // 4:] == SENTINEL).all()), "workspace guard"
    # the slab past the kernel's own is never written; the written ones hold no NaN
    S = _slabs(K)
    per = wsb // 4 // split
    assert bool(torch.isnan(ws[S * per:wsb // 4]).all()), "a slab past the kernel's was written"
    assert bool(torch.isfinite(ws[:S * per]).all()), "a word of a written slab was left unwritten"
    written = torch.zeros_like(buf, dtype=torch.bool)
    written[lo:lo + M * ldc].view(M, ldc)[:, :N] = True
    assert bool((buf[~written] == SENTINEL).all()), "C guard"
    return out.clone()


@pytest.mark.parametrize("K", [512, 515, 1000])
@pytest.mark.parametrize("N", [4, 8, 36, 200])
def test_slab_stores_every_row_count(N, K):
    """|err| <= 2e-6 sqrt(K) 4 + 1e-5 |ref| against float64 (the small-M bound of
    tests/test_gemm_routes.py), at every M, epilogue and C layout; the pointer
    reduce's result is the buffer reduce's, bit for bit."""
    g = torch.Generator().manual_seed(1000 * N + K)
    B = torch.randn(K, N, generator=g)
    Bd = B.to(DEV)
    split = _slabs(K) + 1
    route = (ctypes.c_int32 * 4)()
    for M in ROWS:
        A = torch.randn(M, K, generator=g)
        Ap = torch.full((M, (K + 3) // 4 * 4), float("nan"))     # NaN in A's row padding
        Ap[:, :K] = A
        Ad = Ap.to(DEV)[:, :K]
        assert _lib.load().gcnk_gemm_route(0, 0, M, N, K, Ad.stride(0), N, 1, 1, split, route) == _lib.OK
        assert route[0] == _lib.GEMM_ROUTE_SMALLM
        ref = A.double().numpy() @ B.double().numpy()
        worst = 0.0
        for name in EPILOGUES:
            epi, apply = _epilogue(name, M, N, torch.Generator().manual_seed(M))
            want = apply(ref)
            bound = 2e-6 * np.sqrt(K) * 4 + 1e-5 * np.abs(want)
            first = None
            for ldc_pad, shift in C_LAYOUTS:
                got = _gemm(Ad, Bd, M, N, K, split, epi, ldc_pad, shift)
                gn = got.double().cpu().numpy()
                assert np.isfinite(gn).all(), (M, name, ldc_pad, shift)
                err = np.abs(gn - want)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (M, name, ldc_pad, shift, float((err - bound).max()))
                if first is None:
                    first = got
                assert torch.equal(got, first), (M, name, ldc_pad, shift)
        print(f"M={M}: worst err / bound {worst:.3f}")
