"""Every route of gcnk_gemm_f32, and gcnk_colsum_f32's block edges.

CPU (unmarked): gcnk_gemm_route -- the host function gcnk_gemm_f32's launch
switches on -- says which kernel each case of tests/gemm_cases.py reaches: each
case must reach the route it names, and the table every instantiation the
library compiles (so a moved threshold cannot orphan one unnoticed), with every
epilogue on every family.

GPU: every case against float64, on operands that are views into wider
buffers whose padding holds NaN (A, B, R) or a sentinel (C): the result must
be finite, within test_gemm_mfma's bound
    |err| <= 2e-6 * sqrt(K) * 4 + 1e-5 * |ref|
(split sums too: none needed the 1e-4 of test_gemm_epilogues_and_split_k), C's
padding bitwise untouched, and a second call bitwise equal.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib, colsum, gemm  # noqa: E402
from oracle import csr_ref  # noqa: E402

DEV = "cuda"
SENTINEL = -12345.0
EPI_CODE = {"none": _lib.GEMM_EPI_NONE, "bias": _lib.GEMM_EPI_BIAS, "bias_null": _lib.GEMM_EPI_BIAS,
            "bias_relu": _lib.GEMM_EPI_BIAS_RELU, "mask_pos": _lib.GEMM_EPI_MASK_POS}


def _route(c):
    out = (ctypes.c_int32 * 4)()
    rc = _lib.load().gcnk_gemm_route(c.ta, c.tb, c.M, c.N, c.K, c.lda, c.ldb, int(c.misalign != "a_base"),
                                     int(c.misalign != "b_base"), c.split_k, out)
    assert rc == _lib.OK
    return tuple(out)


# ------------------------------------------------------------------------------ CPU: the route table

def test_route_constants_match_the_binding():
    assert (gc.NARROW, gc.SKINNY, gc.SHORTK, gc.SMALLM, gc.TILED_N16, gc.TILED) == (
        _lib.GEMM_ROUTE_NARROW, _lib.GEMM_ROUTE_SKINNY, _lib.GEMM_ROUTE_SHORTK, _lib.GEMM_ROUTE_SMALLM,
        _lib.GEMM_ROUTE_TILED_N16, _lib.GEMM_ROUTE_TILED)
    assert (gc.SPLIT, gc.PTR_FETCH) == (_lib.GEMM_ROUTE_SPLIT, _lib.GEMM_ROUTE_PTR_FETCH)
    out = (ctypes.c_int32 * 4)()
    lib = _lib.load()
    assert lib.gcnk_gemm_route(0, 0, 4, 4, 4, 4, 4, 1, 1, 1, None) == _lib.EARG
    assert lib.gcnk_gemm_route(0, 0, 0, 4, 4, 4, 4, 1, 1, 1, out) == _lib.EARG


@pytest.mark.parametrize("case", gc.ALL_CASES, ids=lambda c: c.name)
def test_case_reaches_the_route_it_names(case):
    assert _route(case) == case.route
    assert case.epilogue in gc.EPILOGUES and case.misalign in ("", "a_base", "b_base")


def test_table_reaches_every_instantiation():
    """The instantiation list of csrc/gemm.hip (the comment block above
    gemm_route), mirrored by gemm_cases.INSTANTIATIONS: a case for each entry,
    pointer loads on both tiles, nothing reached that the list does not know."""
    reached = {_route(c) for c in gc.ALL_CASES}
    missing = [r for r in gc.INSTANTIATIONS if r not in reached]
    assert not missing, f"no case reaches {missing}"
    for fam in gc.PTR_FETCH_FAMILIES:
        assert any(r[0] == fam and r[3] & gc.PTR_FETCH for r in reached), f"no pointer-fetch case on family {fam}"
    unknown = [r for r in reached if (r[0], r[1], r[2], r[3] & ~gc.PTR_FETCH) not in gc.INSTANTIATIONS]
    assert not unknown, f"routes outside the instantiation list: {unknown}"
    # the list itself: 2 narrow, 15 skinny, 8 short-K, small-M, 2 tiles x 4 transposes x whole / split
    assert len(set(gc.INSTANTIATIONS)) == len(gc.INSTANTIATIONS) == 2 + 15 + 8 + 1 + 16


def test_every_epilogue_on_every_family():
    """NONE, BIAS, BIAS_RELU and MASK_POS on each family; for the split tiled
    kernels and the small-M kernel that is on their reduce kernels, so whole
    and split count as separate families."""
    seen = {}
    for c in gc.ALL_CASES:
        seen.setdefault((c.route[0], c.route[3] & gc.SPLIT), set()).add(c.epilogue)
    assert set(seen) == {(r[0], r[3] & gc.SPLIT) for r in gc.INSTANTIATIONS}
    for key, epis in seen.items():
        assert set(gc.REQUIRED_EPILOGUES) <= epis, f"family {key}: only {sorted(epis)}"
    # an epilogue together with each transpose, and the backward's own call: transB + MASK_POS
    assert any(c.ta and c.epilogue != "none" for c in gc.ALL_CASES)
    assert any(c.tb and not c.ta and c.epilogue == "mask_pos" for c in gc.ALL_CASES)


def test_fall_throughs_leave_the_fast_kernel():
    """One shape per fast family; A's base pointer off a 16-byte boundary, rows
    of A that are no multiple of 4 floats, and (narrow, short-K) such rows of B
    or such a base pointer of B each leave it: for the tiled kernel, except
    the narrow kernel's B, which the skinny kernel (scalar B loads) takes."""
    fast_seen = set()
    for fast, changed in gc.FALLTHROUGHS:
        fam = fast.route[0]
        assert fam in (gc.NARROW, gc.SKINNY, gc.SHORTK, gc.SMALLM) and _route(fast) == fast.route
        fast_seen.add(fam)
        kinds = set()
        for c in changed:
            diff = {f for f in c._fields if getattr(c, f) != getattr(fast, f)} - {"route"}
            assert len(diff) == 1, diff            # one change at a time
            got = _route(c)
            assert got == c.route and got[0] != fam
            what = diff.pop()
            if what == "misalign" and c.misalign == "b_base":
                what = "b_base"
                assert got[0] == (gc.SKINNY if fam == gc.NARROW else gc.TILED)
            elif what == "misalign":
                assert c.misalign == "a_base" and got[0] in (gc.TILED, gc.TILED_N16)
            elif what == "pad_a":
                assert c.lda % 4 != 0 and fast.lda % 4 == 0 and got[0] in (gc.TILED, gc.TILED_N16)
            else:
                assert what == "pad_b" and c.ldb % 4 != 0 and fast.ldb % 4 == 0
                assert got[0] == (gc.SKINNY if fam == gc.NARROW else gc.TILED)
            kinds.add(what)
        assert kinds == ({"misalign", "pad_a", "pad_b", "b_base"} if fam in (gc.NARROW, gc.SHORTK) else {"misalign", "pad_a"})
    assert fast_seen == {gc.NARROW, gc.SKINNY, gc.SHORTK, gc.SMALLM}


# ------------------------------------------------------------------------------ GPU: every case against float64

def _padded(rows, cols, pad, fill, g, misaligned=False, relu=False):
    """(device view [rows x cols] of a [rows x (cols + pad)] buffer whose padding is NaN, its float64 values)."""
    v = torch.randn(rows, cols, generator=g)
    if relu:
        v = torch.relu(v)                          # exact zeros
    ld = cols + pad
    flat = torch.full((rows * ld + 1,), fill)
    off = 1 if misaligned else 0
    flat[off:off + rows * ld].view(rows, ld)[:, :cols] = v
    d = flat.to(DEV)[off:off + rows * ld].view(rows, ld)[:, :cols]
    assert d.stride(0) == ld and (d.data_ptr() % 16 != 0) == misaligned
    return d, v.double().numpy()


def _reference(c, a, b, bias, r):
    ref = csr_ref.gemm(a, b, bool(c.ta), bool(c.tb))
    if c.epilogue in ("bias", "bias_relu"):
        ref = ref + bias[None, :]
    if c.epilogue == "bias_relu":
        ref = np.maximum(ref, 0.0)
    if c.epilogue == "mask_pos":
        ref = np.where(r > 0, 2.0 * ref, 0.0)
    return ref


def _run(c, A, B, bias, R):
    """(C's buffer, the result view into it) of one call."""
    buf = torch.full((c.M, c.N + c.pad_c), SENTINEL, device=DEV)
    out = buf[:, :c.N]
    got = gemm(A, B, transA=bool(c.ta), transB=bool(c.tb), bias=bias, epilogue=EPI_CODE[c.epilogue], R=R,
               scale=2.0 if c.epilogue == "mask_pos" else 1.0, split_k=c.split_k, out=out)
    assert got.data_ptr() == out.data_ptr()
    return buf, out


def _check(c, A, a, g):
    """Case `c` on left operand A (float64 values a): B, bias, R drawn from g."""
    B, b = _padded(*((c.N, c.K) if c.tb else (c.K, c.N)), c.pad_b, float("nan"), g, misaligned=c.misalign == "b_base")
    bias = torch.randn(c.N, generator=g) if c.epilogue in ("bias", "bias_relu") else None
    R, r = _padded(c.M, c.N, gc.PAD_R, float("nan"), g, relu=True) if c.epilogue == "mask_pos" else (None, None)
    ref = _reference(c, a, b, bias.double().numpy() if bias is not None else None, r)
    buf, out = _run(c, A, B, bias.to(DEV) if bias is not None else None, R)
    got = out.double().cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    bound = 2e-6 * np.sqrt(c.K) * 4 + 1e-5 * np.abs(ref)
    print(f"gemm {c.name}: max err {err.max():.3e}, err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"max err {err.max():.3e} (bound at worst {bound.flat[np.argmax(err - bound)]:.3e})"
    assert torch.equal(buf[:, c.N:], torch.full((c.M, c.pad_c), SENTINEL, device=DEV))
    buf2, out2 = _run(c, A, B, bias.to(DEV) if bias is not None else None, R)
    assert torch.equal(out, out2) and torch.equal(buf, buf2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_gemm_case_against_float64(case):
    c = case
    g = torch.Generator().manual_seed(1000003 * c.M + 1009 * c.N + c.K + 7 * c.pad_a + c.split_k)
    A, a = _padded(*((c.K, c.M) if c.ta else (c.M, c.K)), c.pad_a, float("nan"), g, misaligned=c.misalign == "a_base")
    assert A.stride(0) == c.lda
    _check(c, A, a, g)


@pytest.mark.gpu
def test_gemm_operands_past_32_bit_offsets():
    """The tiled kernel's pointer loads (both tiles, whole and split) and the
    small-M dispatch's fall-through past its buffer offsets: A is a strided
    view of one uninitialised ~2.15 GB buffer (only the views are filled), the
    products themselves are tiny."""
    big = torch.empty(gc.BIG_FLOATS, dtype=torch.float32, device=DEV)
    try:
        for c in gc.BIG_CASES:
            rows, cols = (c.K, c.M) if c.ta else (c.M, c.K)
            assert (rows - 1) * c.lda + cols <= gc.BIG_FLOATS and rows * c.lda * 4 >= 0x7ff00000
            g = torch.Generator().manual_seed(c.lda + c.N)
            v = torch.randn(rows, cols, generator=g)
            A = big.as_strided((rows, cols), (c.lda, 1))
            A.copy_(v.to(DEV))
            _check(c, A, v.double().numpy(), g)
            del A
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------ GPU: colsum

@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 63, 64, 65, 1025])
def test_colsum_block_edges(M, N):
    """gcnk_colsum_f32 at the 16-row batch and 64-row block edges and across
    256-column blocks, on rows padded with NaN (ldx > N); bitwise reproducible."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    X, x = _padded(M, N, 3, float("nan"), g)
    got = colsum(X)
    ref = csr_ref.colsum(x)
    err = np.abs(got.double().cpu().numpy() - ref)
    bound = 2e-5 * np.sqrt(M) + 1e-5 * np.abs(ref)
    print(f"colsum {M}x{N}: max err {err.max():.3e}, err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"max err {err.max():.3e}"
    assert torch.equal(got, colsum(X))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 257])
def test_colsum_of_no_rows_is_zero(N):
    X = torch.empty((0, N + 3), dtype=torch.float32, device=DEV)[:, :N]
    out = colsum(X)
    assert out.shape == (N,) and torch.equal(out, torch.zeros(N, device=DEV))
