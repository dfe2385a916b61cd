"""The three short kernels of the factored eval forward after their serial
instruction paths were trimmed: values unchanged at every size where the trimmed
code takes another turn.

Small-M GEMM (gemm_smallm_wk_kernel<2, 2, NM, VREM>): every row count around
its 16-row tiles, a last tile of 1 or 2 rows (multiplied on the VALU) and of 3.
Slab reduce (gemm_slab_reduce4_buf_kernel<B> and the pointer kernel it falls
back to): slab counts that leave a group of the reduce 0, 1, 2 and more than 8
slabs, every epilogue, C strided / off a 16-byte boundary (the fall-back), and
the two kernels bit for bit equal.
Factored gc1 (hubfactor_gc1_kernel): W2's fragments now come straight from
global memory through a buffer resource: every projection width around the
16-column n-tile, F at both ends of its range, LDS poisoned with NaN bits first
and W2 surrounded by NaN in memory.
"""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, gemm

from hub_records import ROWS, pack, rec_words_for

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(got, ref, rtol, atol):
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    bound = atol + rtol * np.abs(ref)
    print(f"max err {err.max():.3e}, smallest margin {(bound - err).min():.3e}")
    assert (err <= bound).all(), float((err - bound).max())


def _route_family(M, N, K, lda, ldb, split):
    out = (ctypes.c_int32 * 4)()
    assert _lib.load().gcnk_gemm_route(0, 0, M, N, K, lda, ldb, 1, 1, split, out) == _lib.OK
    return out[0]


def _padded_a(M, K, g):
    """A [M x K] on rows padded to a multiple of 4 floats, NaN in the padding."""
    A = torch.randn(M, K, generator=g)
    Ap = torch.full((M, (K + 3) // 4 * 4), float("nan"))
    Ap[:, :K] = A
    Ad = Ap.to(DEV)[:, :K]
    assert Ad.stride(0) % 4 == 0
    return A, Ad


# ------------------------------------------------------------------ small-M GEMM

# ... and both sides of the 2-row bound of the last tile's VALU path at every tile count: 2|3, 18|19, 34|35, 50|51
SMALL_M = (1, 2, 3, 15, 16, 17, 18, 19, 33, 34, 35, 47, 48, 49, 50, 51, 63, 64)


@pytest.mark.parametrize("K", [515, 1000])
@pytest.mark.parametrize("N", [4, 36, 200, 332])
def test_small_m_gemm_row_counts(N, K):
    """Every M around the kernel's 16-row tiles against float64 (the bound of
    test_gemm_small_m_split_k), two calls bit for bit equal."""
    g = torch.Generator().manual_seed(1000 * N + K)
    B = torch.randn(K, N, generator=g)
    Bd = B.to(DEV)
    for M in SMALL_M:
        A, Ad = _padded_a(M, K, g)
        assert _route_family(M, N, K, Ad.stride(0), N, 8) == _lib.GEMM_ROUTE_SMALLM
        got = gemm(Ad, Bd, split_k=8)
        print(f"M={M}: ", end="")
        _close(got, A.double().numpy() @ B.double().numpy(), rtol=1e-5, atol=2e-6 * np.sqrt(K) * 4)
        assert torch.equal(got, gemm(Ad, Bd, split_k=8)), M


# ------------------------------------------------------------------ slab reduce

EPILOGUES = ("none", "bias", "bias_relu", "mask_pos", "bias_null")
_RED_M, _RED_N = 50, 200          # 2,500 float4 of output: the last workgroup of the reduce holds 4 of its 16


def _slab_k(s):
    """A K at which the small-M kernel leaves s slabs (256 k each), ragged
    against 4, 16 and 256; s = 1 and 2 lie below its range and at its bottom."""
    return {1: 515, 2: 512}.get(s, 256 * s - 3)


def _epilogue_args(name, M, N, g):
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

    kw = dict(bias=bias.to(DEV) if bias is not None else None, epilogue=code,
              R=R.to(DEV) if R is not None else None, scale=2.0 if name == "mask_pos" else 1.0)
    return kw, apply


@pytest.fixture(scope="module")
def slab_operands():
    """Per slab count s: A (padded rows, on the device), B, and the float64 product; built once."""
    made = {}

    def get(s):
        if s not in made:
            K = _slab_k(s)
            g = torch.Generator().manual_seed(77 + s)
            A, Ad = _padded_a(_RED_M, K, g)
            B = torch.randn(K, _RED_N, generator=g)
            made[s] = (K, Ad, B.to(DEV), A.double().numpy() @ B.double().numpy())
        return made[s]
    return get


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("s", [1, 2, 3, 15, 16, 17, 30, 31, 129])
def test_slab_reduce_slab_counts(slab_operands, s, epilogue):
    K, Ad, Bd, ref = slab_operands(s)
    if s > 1:
        assert _route_family(_RED_M, _RED_N, K, Ad.stride(0), _RED_N, s) == _lib.GEMM_ROUTE_SMALLM
    kw, apply = _epilogue_args(epilogue, _RED_M, _RED_N, torch.Generator().manual_seed(s))
    got = gemm(Ad, Bd, split_k=s, **kw)
    _close(got, apply(ref), rtol=1e-5, atol=2e-6 * np.sqrt(K) * 4)
    assert torch.equal(got, gemm(Ad, Bd, split_k=s, **kw))


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("s", [3, 16, 30, 129])
def test_slab_reduce_strided_and_unaligned_c(slab_operands, s, epilogue):
    """C with ldc > N on 16-byte rows (the buffer kernel, strided), with rows
    that are no multiple of 4 floats and with a base pointer one float past a
    16-byte boundary (both: the pointer kernel): each within the bound, nothing
    written outside C, and all three bit for bit the contiguous result -- the
    two reduce kernels add the same values in the same order."""
    K, Ad, Bd, ref = slab_operands(s)
    M, N = _RED_M, _RED_N
    kw, apply = _epilogue_args(epilogue, M, N, torch.Generator().manual_seed(s))
    want = gemm(Ad, Bd, split_k=s, **kw)
    sentinel = -12345.0
    for ldc, shift in ((N + 8, 0), (N + 3, 0), (N, 1)):
        buf = torch.full((M * ldc + 8,), sentinel, device=DEV)
        assert buf.data_ptr() % 16 == 0
        out = buf[shift:shift + M * ldc].view(M, ldc)[:, :N]
        assert (out.data_ptr() % 16 == 0) == (shift == 0)
        got = gemm(Ad, Bd, split_k=s, out=out, **kw)
        assert got.data_ptr() == out.data_ptr()
        _close(got, apply(ref), rtol=1e-5, atol=2e-6 * np.sqrt(K) * 4)
        assert torch.equal(got, want), (ldc, shift)
        written = torch.zeros(M * ldc + 8, dtype=torch.bool, device=DEV)
        written[shift:shift + M * ldc].view(M, ldc)[:, :N] = True
        assert bool((buf[~written] == sentinel).all()), (ldc, shift)


# ------------------------------------------------------------------ factored gc1 projection

FM = 70                                          # 70 rows: three 32-row blocks, the last with 6 real rows
NHUB, KC, K0 = 3, 50, 3
GUARD = 8
SENTINEL = -12345.0


def _factor_operands(F, P):
    """Hand-built operands (block records: tests/hub_records.py), and H1, S2 in
    float64 from the same arrays."""
    rng = np.random.default_rng(100 * F + P)
    M = FM
    perm = rng.permutation(M)
    nblk = (M + ROWS - 1) // ROWS
    counts = rng.integers(0, NHUB + 1, nblk * ROWS)
    counts[M:] = 0
    counts[5] = 40                                   # one long row
    hubs = [rng.integers(0, NHUB, c) for c in counts]
    vals = [rng.uniform(-1.0, 1.0, c).astype(np.float32) for c in counts]
    rec_words = rec_words_for(counts, tail=4)
    rec = pack([list(zip(h, v)) for h, v in zip(hubs, vals)], perm, M, rec_words, np.int32(0x7FC00000))
    ldu = KC + 2                                     # a multiple of 4: U's rows staged in LDS
    U = np.full((M, ldu), np.nan, np.float32)
    U[:, :KC] = rng.standard_normal((M, KC)) * 0.3
    W1 = rng.standard_normal((K0 + KC + 5, F)).astype(np.float32)
    S = rng.standard_normal((NHUB, F)).astype(np.float32)
    b1 = rng.standard_normal(F).astype(np.float32)
    W2 = rng.standard_normal((F, P)).astype(np.float32)
    Z = np.zeros((M, F))
    UW = U[:, :KC].astype(np.float64) @ W1[K0:K0 + KC].astype(np.float64)
    for pos in range(M):
        z = UW[pos].copy()
        for hcol, val in zip(hubs[pos], vals[pos]):
            z += np.float64(val) * S[hcol].astype(np.float64)
        Z[perm[pos]] = z
    H1 = np.maximum(Z + b1.astype(np.float64), 0.0)
    return dict(rec=rec, rec_words=rec_words, ldu=ldu, U=U, W1=W1, S=S, b1=b1, W2=W2, H1=H1,
                S2=H1 @ W2.astype(np.float64))


@pytest.mark.parametrize("P", [1, 7, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("F", [4, 60, 200, 256])
def test_hubfactor_projection_widths(F, P):
    """H1 and S2 = H1 W2 against float64 (max error over max(1, |ref|) below
    1e-6, the bound of tests/test_factor.py), after an LDS fill with NaN bits,
    with W2 lying between NaN words in memory: a fragment read for a row past F
    or a column past P must give 0, not its neighbour's bytes or an LDS word the
    kernel no longer writes.  S2 the same bits with and without the H1 store."""
    o = _factor_operands(F, P)
    lib = _lib.load()
    dev = {k: torch.from_numpy(o[k]).to(DEV) for k in ("rec", "U", "W1", "S", "b1")}
    pad = 8192                                       # more than the F P floats any padded fragment could reach into
    w2buf = torch.full((pad + F * P + pad,), float("nan"), device=DEV)
    W2 = w2buf[pad:pad + F * P].view(F, P)
    W2.copy_(torch.from_numpy(o["W2"]))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    M = FM

    def launch(store_h1):
        Hbuf = torch.full((M + 2 * GUARD, F), SENTINEL, device=DEV)
        Cbuf = torch.full((M + 2 * GUARD, P), SENTINEL, device=DEV)
        H1, S2 = Hbuf[GUARD:GUARD + M], Cbuf[GUARD:GUARD + M]
        _lib.check(lib.gcnk_debug_poison_lds(0xFFFFFFFF, stream), "gcnk_debug_poison_lds")
        _lib.check(lib.gcnk_hubfactor_gc1_f32(
            M, F, KC, NHUB, P, p(dev["U"]), o["ldu"], p(dev["W1"]), F, K0, p(dev["S"]), F, p(dev["rec"]),
            o["rec_words"], p(dev["b1"]), _lib.EPI_BIAS_RELU, None, 0, 1.0, 1.0, 0, 0, None, p(W2), P,
            p(H1) if store_h1 else None, F, p(S2), P, stream), "gcnk_hubfactor_gc1_f32")
        torch.cuda.synchronize()
        for buf in (Hbuf, Cbuf):
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + M:] == SENTINEL).all())
        return H1, S2

    H1, S2 = launch(True)
    _, S2n = launch(False)
    assert bool(torch.isfinite(H1).all()) and bool(torch.isfinite(S2).all())
    err1 = np.abs(H1.double().cpu().numpy() - o["H1"]).max() / max(1.0, np.abs(o["H1"]).max())
    err2 = np.abs(S2.double().cpu().numpy() - o["S2"]).max() / max(1.0, np.abs(o["S2"]).max())
    print(f"H1 err {err1:.3e}, S2 err {err2:.3e} (bound 1e-6)")
    assert err1 < 1e-6, err1
    assert err2 < 1e-6, err2
    assert torch.equal(S2n, S2)
