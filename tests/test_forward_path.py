"""Which of the four schedules the two-layer forward takes: the numeric part of
ops.choose_forward (ops.forward_kind), the rule launch records and the per-op
path share.  No GPU: numbers and booleans only."""
import inspect
import itertools

import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, ops, record

LDS = ops.FACTOR_LDS_BUDGET
ON_OFF = (False, True)


def kind(F, P, dense_ax=False, factored=False, lds=0, fuse=True, fuse_max_p=8, proj_ntile=0):
    return ops.forward_kind(F, P, dense_ax, factored, lds if factored else 0, fuse, fuse_max_p, proj_ntile)


def test_kind_constants_mirror_the_header():
    assert (record.FACTORED, record.SPMM_PROJ, record.SPMM_GEMM, record.DENSE_AX) == (1, 2, 3, 4)
    assert (ops.FWD_FACTORED, ops.FWD_SPMM_PROJ, ops.FWD_SPMM_GEMM, ops.FWD_DENSE_AX) == (1, 2, 3, 4)
    assert record.KIND_NAMES == {1: "factored", 2: "spmm+proj", 3: "spmm+gemm", 4: "dense-ax"}
    assert LDS == 160 * 1024


@pytest.mark.parametrize("dense_ax,factored,fuse,ntile", list(itertools.product(ON_OFF, ON_OFF, ON_OFF, (0, 1))))
def test_priority_order_at_r8_widths(dense_ax, factored, fuse, ntile):
    """F = 200, P = 8 is inside every kernel's range: dense-AX before factored
    before the fused projection (fuse knob on, no tile chunks) before SpMM + GEMM."""
    want = record.DENSE_AX if dense_ax else record.FACTORED if factored else \
        record.SPMM_PROJ if fuse and ntile == 0 else record.SPMM_GEMM
    assert kind(200, 8, dense_ax, factored, 1024, fuse, 8, ntile) == want


def test_narrow_hidden_width_takes_the_fused_projection():
    assert kind(36, 8) == record.SPMM_PROJ


@pytest.mark.parametrize("F", [50, 300])   # not a multiple of 4 (no 16-B rows); past the 256-column tile
@pytest.mark.parametrize("dense_ax,factored,fuse,ntile", list(itertools.product(ON_OFF, ON_OFF, ON_OFF, (0, 1))))
def test_widths_outside_the_fused_kernels_take_spmm_gemm(F, dense_ax, factored, fuse, ntile):
    for P in (8, 20, 33):
        assert kind(F, P, dense_ax, factored, 1024, fuse, 8, ntile) == record.SPMM_GEMM
        assert kind(F, P, dense_ax, factored, 1024, fuse, 64, ntile) == record.SPMM_GEMM


def test_classes_past_fuse_max_p():
    """P = 20 with FUSE_MAX_P = 8: the factored kernel still projects (P <= 32),
    the fused SpMM projection is not taken."""
    assert kind(200, 20, factored=True, lds=1024, fuse_max_p=8) == record.FACTORED
    assert kind(200, 20, dense_ax=True, fuse_max_p=8) == record.DENSE_AX
    assert kind(200, 20, fuse_max_p=8) == record.SPMM_GEMM
    assert kind(200, 20, fuse_max_p=20) == record.SPMM_PROJ


@pytest.mark.parametrize("dense_ax,factored,fuse,ntile", list(itertools.product(ON_OFF, ON_OFF, ON_OFF, (0, 1))))
def test_more_than_32_classes_take_spmm_gemm_only(dense_ax, factored, fuse, ntile):
    assert kind(200, 33, dense_ax, factored, 1024, fuse, 8, ntile) == record.SPMM_GEMM
    assert kind(200, 32, True, factored, 1024, fuse, 8, ntile) == record.DENSE_AX   # (the last width inside)


def test_factored_kernel_lds_budget():
    assert kind(200, 8, factored=True, lds=LDS) == record.FACTORED
    assert kind(200, 8, factored=True, lds=LDS + 1) == record.SPMM_PROJ
    assert kind(200, 8, factored=True, lds=LDS + 1, fuse=False) == record.SPMM_GEMM
    assert kind(200, 20, factored=True, lds=LDS + 1) == record.SPMM_GEMM


def test_projection_plan_with_tile_chunks_takes_spmm_gemm():
    assert kind(200, 8, proj_ntile=0) == record.SPMM_PROJ
    assert kind(200, 8, proj_ntile=3) == record.SPMM_GEMM
    assert kind(64, 4, proj_ntile=1) == record.SPMM_GEMM


def test_epilogue_c_arguments():
    """ops.Epilogue.c_args: the tail every entry point takes -- epilogue, mask,
    ldm (0 without a mask), scale, keep_prob, seed and offset as uint64, rng_base."""
    assert ops.Epilogue(_lib.EPI_BIAS_RELU).c_args() == (_lib.EPI_BIAS_RELU, None, 0, 1.0, 1.0, 0, 0, None)
    mask = torch.ones((5, 8), dtype=torch.uint8)
    base = torch.zeros(1, dtype=torch.int64)
    e = ops.Epilogue(_lib.EPI_BIAS_RELU_HASH, mask, 2, 0.5, -1, 2**64 + 3, base)
    assert e.c_args() == (_lib.EPI_BIAS_RELU_HASH, mask.data_ptr(), 8, 2.0, 0.5, 2**64 - 1, 3, base.data_ptr())
    for op in (ops.spmm, ops.spmm_proj, ops.hubfactor_gc1, ops.dense_gc1):   # (``**epi._asdict()`` passes one on)
        assert set(e._fields) <= set(inspect.signature(op).parameters)
    strided = ops.Epilogue(_lib.EPI_BIAS_RELU_DROP, torch.ones((5, 16), dtype=torch.uint8)[:, ::2])
    assert strided.on(mask.device).mask.is_contiguous() and e.on(mask.device) == e
    assert [type(a) for a in e.on(mask.device)[2:6]] == [float, float, int, int]
    with pytest.raises(RuntimeError):
        ops.Epilogue(_lib.EPI_BIAS_RELU_HASH, rng_base=base.int()).on(base.device)
