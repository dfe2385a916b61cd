"""CPU check of the row-unit SpMM control logic (light units, heavy segments
with interleaved lane groups, partial slots, last-arriver combine) through its
Python model tests/path_model.py, which mirrors the planner in
graph-convolutional-networks-for-text-classification_amd/csrc/spmm_plan.cpp
and the row kernel in csrc/spmm.hip."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_model  # noqa: E402
from oracle import csr_ref  # noqa: E402


@pytest.mark.parametrize("groups,ipc", [(1, 32), (32, 8), (1, 4), (4, 16), (8, 3), (1, 1), (64, 8)])
def test_model_on_r8(r8, groups, ipc):
    rp, ci, v = csr_ref.coo_to_csr(r8["adj"]._indices()[0].numpy(), r8["adj"]._indices()[1].numpy(),
                                   r8["adj"]._values().numpy(), (r8["nodes"], r8["nodes"]))
    B = np.random.default_rng(groups * 10 + ipc).standard_normal((r8["nodes"], 3))
    C = path_model.spmm(rp, ci, v, B, ipc, groups)
    np.testing.assert_allclose(C, csr_ref.spmm_csr(rp, ci, v, B), atol=1e-12)


def test_r8_plan_shape(r8):
    """R8: document rows (5 nonzeros) are light units, the 50 topic rows (up to
    ~1.8k nonzeros over all document columns) split at the 8 column classes
    into <= 64 segments each; padding stays small."""
    rp, ci, v = csr_ref.coo_to_csr(r8["adj"]._indices()[0].numpy(), r8["adj"]._indices()[1].numpy(),
                                   r8["adj"]._values().numpy(), (r8["nodes"], r8["nodes"]))
    units, heavy, nh, nslots = path_model.host_plan(rp, ci, r8["nodes"], 32, 1)
    light = [x for x in units[nh:] if x[0] >= 0]
    assert len(light) == 7674 and len(heavy) == 50
    assert all(1 < h[2] <= path_model.K_MAX_SEG and h[3] == -1 for h in heavy)
    assert nslots == sum(h[2] for h in heavy)
    assert sum(1 for x in units if x[0] < 0) < 0.05 * len(units)


@pytest.mark.parametrize("seed", range(6))
def test_model_on_skewed_random(seed):
    rng = np.random.default_rng(seed)
    M, K = int(rng.integers(1, 300)), int(rng.integers(1, 200))
    deg = rng.choice([0, 1, 2, 5, 40, 300, 5000], size=M, p=[0.2, 0.2, 0.2, 0.25, 0.1, 0.04, 0.01])
    rows = np.repeat(np.arange(M), deg)
    cols = rng.integers(0, K, rows.size)
    rp, ci, v = csr_ref.coo_to_csr(rows, cols, rng.standard_normal(rows.size), (M, K))
    B = rng.standard_normal((K, 2))
    for groups, ipc in [(1, 4), (1, 32), (32, 8), (4, 3)]:
        C = path_model.spmm(rp, ci, v, B, ipc, groups)
        np.testing.assert_allclose(C, csr_ref.spmm_csr(rp, ci, v, B), atol=1e-10)


def test_power_law_row_takes_two_combine_levels():
    """A row of ~90 k nonzeros (a power-law hub) keeps base-length segments:
    > 64 of them, in groups of <= 64 under one top entry, and the model's
    two-level combine gives the float64 product."""
    rng = np.random.default_rng(11)
    M, K = 40, 5000
    deg = np.array([90_000, 3000, 0, 7] + [20] * (M - 4))
    rows = np.repeat(np.arange(M), deg)
    cols = rng.integers(0, K, rows.size)
    rp, ci, v = csr_ref.coo_to_csr(rows, cols, rng.standard_normal(rows.size), (M, K))
    ipc, groups = 12, 1
    units, heavy, nh, nslots = path_model.host_plan(rp, ci, K, ipc, groups)
    seg = ipc * path_model.geometry(groups)[2]
    hub = [u for u in units[:nh] if u[0] == 0]
    assert len(hub) > path_model.K_MAX_SEG and max(u[2] - u[1] for u in hub) <= seg
    tops = [h for h in heavy if h[0] == 0 and h[3] == -2]
    assert len(tops) == 1 and 1 < tops[0][2] <= path_model.K_MAX_SEG
    assert all(h[2] <= path_model.K_MAX_SEG for h in heavy)
    B = rng.standard_normal((K, 2))
    np.testing.assert_allclose(path_model.spmm(rp, ci, v, B, ipc, groups), csr_ref.spmm_csr(rp, ci, v, B), rtol=1e-9,
                               atol=1e-9)


def test_combine_levels_at_the_boundaries():
    """csrc/spmm_plan.cpp's heavy-row plan at its boundaries (segment length 16 at
    ipc 4 with one lane group): 64 segments -> one combine; 65 -> a top entry
    over 2 groups; 4,375 segments (> 4,096) -> the segment length doubles, then
    groups of <= 64 under a top entry; the model's product is the float64 one."""
    rng = np.random.default_rng(3)
    K = 80_000
    degs = [1024, 1025, 70_000, 3]
    # rows 0 and 1 inside one column class (K / 8 columns): one run, so their
    # segment counts are exactly ceil(deg / 16) = 64 and 65
    span = [K // 8, K // 8, K, K]
    rows = np.concatenate([np.full(d, r) for r, d in enumerate(degs)])
    cols = np.concatenate([np.sort(rng.choice(sp, d, replace=False)) for d, sp in zip(degs, span)])
    rp, ci, v = csr_ref.coo_to_csr(rows, cols, rng.standard_normal(rows.size), (len(degs), K))
    ipc, groups = 4, 1
    units, heavy, nh, nslots = path_model.host_plan(rp, ci, K, ipc, groups)
    seg = ipc * path_model.geometry(groups)[2]
    assert seg == 16

    def entries(r):
        return [h for h in heavy if h[0] == r]
    e0 = entries(0)
    assert len(e0) == 1 and e0[0][2] == 64 and e0[0][3] == -1
    e1 = entries(1)
    assert [h[3] for h in e1].count(-2) == 1 and len(e1) == 3
    e2 = entries(2)
    top = [h for h in e2 if h[3] == -2]
    assert len(top) == 1 and top[0][2] == len(e2) - 1
    assert all(h[2] <= path_model.K_MAX_SEG for h in e2)
    seglens = [u[2] - u[1] for u in units[:nh] if u[0] == 2]
    assert max(seglens) <= 2 * seg < 3 * seg and len(seglens) <= 4096
    B = rng.standard_normal((K, 2))
    np.testing.assert_allclose(path_model.spmm(rp, ci, v, B, ipc, groups), csr_ref.spmm_csr(rp, ci, v, B),
                               rtol=1e-9, atol=1e-9)
