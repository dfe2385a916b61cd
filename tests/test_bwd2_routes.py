"""Every instantiation and run-time branch of the fused gc2 backward
(gcnk_gcn_bwd2_f32, csrc/bwd.hip), exactly.

CPU (unmarked): gcnk_gcn_bwd2_route -- the host function the launch is made
from, with the predicates the kernel itself evaluates -- says what each case of
tests/bwd2_cases.py reaches: each case must reach the route it names, and the
table all eight instantiations, each of the three branch flags set and clear,
several slices, several rows per workgroup, a lane with a second batch of rows
and more workgroups than one round of the side reduce.

GPU: the library called through ctypes on operands that are views into wider
buffers, against float64 numpy, EXACTLY.  The inputs sit on small binary quanta
(H on 1/2 in [-2, 2] with exact zeros, -0.0 and negative values; gS2 on 1/4 in
[-1, 1]; W2 on 1/2 in [-1, 1]; G integer in [-2, 2]), so every term of every sum
is a multiple of the sum's quantum, and where the largest sum of absolute terms
stays below 2^24 quanta (test_case_inputs_are_exact_in_fp32: asserted for every
case on the float64 reference alone; the worst case by construction is
M = 65,793 rows x 4 x 4 quanta = 2^20) every partial sum in any order is exact
in fp32: gZ1, gW2, gb1 and gb2 must EQUAL the float64 reference, whichever
instantiation, staging, reduce or workgroup split ran.  One dropped row, row
lane or workgroup partial shows, however small.

Memory: the workspace, every output and all padding hold NaN before each call.
A partial read before it was written, an output left unwritten or padding read
into a result shows as a NaN; gZ1's padding columns, the floats around every
output and the outputs that were not asked for must still be NaN afterwards.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwd2_cases as bc  # noqa: E402
from test_backward_branches import _equal  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib  # noqa: E402

DEV = "cuda"
GUARD = 16                                       # NaN floats before and after every device buffer (64 B)
Q_H, Q_GS, Q_W, Q_G = 0.5, 0.25, 0.5, 1.0        # the quanta of the operands
H_VALUES = np.array([0.0, -0.0, -2.0, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0])
H_PROBS = np.array([0.25, 0.05, 0.03, 0.04, 0.03, 0.15, 0.15, 0.15, 0.15])
SCALES = (2.0, 1.0)
NULLABLE = {"gw_null": ("gb1", "g"), "gb1_null": ("gw", "g"), "g_null": ("gw", "gb1"), "all_null": ()}


def _route(c):
    """(vec, pm, slices, nblk, rpb, flags), part_ld of the case, as the library reports them."""
    out = (ctypes.c_int64 * 9)()
    rc = _lib.load().gcnk_gcn_bwd2_route(c.M, c.N, c.P, c.ldh, c.ldz, c.h_align, c.z_align, c.ldgs, int(c.with_g),
                                         c.ldg, c.ldw, int(c.w_off % 4 == 0), out)
    assert rc == _lib.OK, _lib.load().gcnk_last_error()
    flags = (bc.DMA if out[6] else 0) | (bc.W_RUNS if out[7] else 0) | (bc.VEC_REDUCE if out[8] else 0)
    assert all(out[i] in (0, 1) for i in (6, 7, 8))
    return (out[0], out[1], out[2], out[3], out[4], flags), out[5]


def _row_lanes(c):
    """Row lanes of a workgroup of column slice 0."""
    vec = c.route[0]
    return 256 // min((c.N + vec - 1) // vec, 256 // vec)


# ------------------------------------------------------------------------------ CPU: the route table

def test_route_refuses_bad_arguments():
    lib = _lib.load()
    out = (ctypes.c_int64 * 9)()
    good = [300, 200, 8, 200, 200, 16, 16, 8, 1, 8, 8, 1, out]
    assert lib.gcnk_gcn_bwd2_route(*good) == _lib.OK
    for i, bad in ((0, 0), (1, 0), (2, 0), (2, 33), (3, 199), (4, 199), (5, 2), (6, 32), (7, 7), (9, 7), (10, 7),
                   (12, None)):
        args = list(good)
        args[i] = bad
        assert lib.gcnk_gcn_bwd2_route(*args) == _lib.EARG, i
    assert b"gcnk_gcn_bwd2_route" in lib.gcnk_last_error()
    args = list(good)
    args[8], args[9] = 0, 0           # no G: ldg is not looked at
    assert lib.gcnk_gcn_bwd2_route(*args) == _lib.OK


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_case_reaches_the_route_it_names(case):
    route, part_ld = _route(case)
    assert route == case.route
    assert part_ld == (case.N * case.P + case.N + case.P + 3) // 4 * 4
    assert _lib.load().gcnk_gcn_bwd2_workspace_bytes(case.M, case.N, case.P) == route[3] * part_ld * 4


def test_table_reaches_every_instantiation_and_branch():
    assert len(set(bc.CASES)) == len(bc.CASES) and len({c.name for c in bc.CASES}) == len(bc.CASES)
    routes = {c: _route(c)[0] for c in bc.CASES}
    reached = {r[:2] for r in routes.values()}
    assert len(bc.INSTANTIATIONS) == 8
    missing = [i for i in bc.INSTANTIATIONS if i not in reached]
    assert not missing, f"no case reaches gcn_bwd2_kernel<{missing}>"
    assert reached <= set(bc.INSTANTIATIONS)
    for flag, what in ((bc.DMA, "LDS-DMA staging"), (bc.W_RUNS, "W2 row runs"), (bc.VEC_REDUCE, "float4 lane sum")):
        for vec in (4, 2, 1):
            if flag == bc.VEC_REDUCE and vec != 4:
                assert not any(r[5] & flag for r in routes.values() if r[0] == vec)     # a VEC 4 path only
                continue
            assert any(r[5] & flag for r in routes.values() if r[0] == vec), f"{what} never set on VEC {vec}"
            assert any(not r[5] & flag for r in routes.values() if r[0] == vec), f"{what} never clear on VEC {vec}"
    for vec in (4, 2, 1):
        mine = [(c, r) for c, r in routes.items() if r[0] == vec]
        assert any(r[2] > 1 for _, r in mine), f"VEC {vec}: no case of several slices"
        assert any(r[4] > 1 for _, r in mine), f"VEC {vec}: no case of several rows per workgroup"
        assert any(r[4] >= _row_lanes(c) > 1 and not r[5] & bc.VEC_REDUCE for c, r in mine), \
            f"VEC {vec}: the per-float lane sum never has a row on every one of several lanes"
    assert any(r[4] > 8 * _row_lanes(c) for c, r in routes.items() if r[0] == 4), "no second batch on VEC 4"
    assert any(r[4] > 8 * _row_lanes(c) for c, r in routes.items() if r[0] == 1), "no second batch on VEC 1"
    assert any(r[3] > 256 for r in routes.values()), "the side reduce's second round is never reached"
    assert any(r[4] == 256 for r in routes.values())


def test_table_holds_the_required_cases():
    """The shapes the table was written for (a case deleted by mistake shows here)."""
    cs = bc.CASES
    assert {c.P for c in cs if c.N == 200} >= set(bc.REQUIRED_P)
    assert any(c.N == 200 and c.P == 20 and c.route[:2] == (2, 32) for c in cs)
    # the float4 lane sum at P = 8 and 16, the per-float one on VEC 4 at P = 2 and 9
    assert {c.P for c in cs if c.route[0] == 4 and c.route[5] & bc.VEC_REDUCE} >= {8, 16}
    assert {c.P for c in cs if c.route[0] == 4 and not c.route[5] & bc.VEC_REDUCE} >= {2, 9}
    # staging: DMA at P = 32 on VEC 2 and without G; left by ldgs > P, by ldg > P alone, by P < pm
    assert any(c.route[:2] == (2, 32) and c.route[5] & bc.DMA for c in cs)
    assert any(c.route[5] & bc.DMA and not c.with_g for c in cs)
    p_eq_pm = [c for c in cs if c.P == c.route[1] and not c.route[5] & bc.DMA]
    assert any(c.pad_gs for c in p_eq_pm) and any(c.pad_g and not c.pad_gs and c.with_g for c in p_eq_pm)
    assert any(c.P < c.route[1] for c in cs)
    # W2: row runs, rows apart, base one float off
    runs_off = [c for c in cs if c.P == c.route[1] and not c.route[5] & bc.W_RUNS]
    assert any(c.pad_w and not c.w_off for c in runs_off) and any(c.w_off == 1 and not c.pad_w for c in runs_off)
    # slices, each with G
    for N, vec, slices in ((260, 4, 2), (1030, 2, 5), (257, 1, 2)):
        assert any(c.N == N and c.route[0] == vec and c.route[2] == slices and c.with_g for c in cs), N
    # rows
    assert {1, 255, 256, 257} <= {c.M for c in cs}
    assert any((c.M, c.N, c.route[0], c.route[4]) == (2305, 256, 1, 10) for c in cs)
    assert any((c.M, c.N, c.route[0], c.route[4]) == (8449, 256, 4, 34) for c in cs)
    assert any((c.M, c.N, c.P, c.route[3], c.route[4]) == (65793, 4, 8, 258, 256) for c in cs)
    # strides
    assert any(c.pad_h and not c.pad_z for c in cs) and any(c.pad_z and not c.pad_h for c in cs)
    assert {c.route[0] for c in bc.NULLABLE_CASES} == {4, 2, 1} and all(c.with_g for c in bc.NULLABLE_CASES)


# ------------------------------------------------------------------------------ the problems and their float64 answers

class Problem:
    """One case's seeded operands (float64 numpy, every value an fp32 number) and its float64 answers."""

    def __init__(self, c):
        rng = np.random.default_rng([c.M, c.N, c.P, c.pad_h, c.pad_gs, c.pad_w, c.h_off])
        self.H = rng.choice(H_VALUES, size=(c.M, c.N), p=H_PROBS)
        self.gS = rng.integers(-4, 5, (c.M, c.P)) * Q_GS
        self.W = rng.integers(-2, 3, (c.N, c.P)) * Q_W
        self.G = rng.integers(-2, 3, (c.M, c.P)) * Q_G
        self.T = self.gS @ self.W.T
        self.gW = self.H.T @ self.gS
        self.gb2 = self.G.sum(0)

    def gZ(self, scale):
        return np.where(self.H > 0, scale * self.T, 0.0)

    def exactness_ratio(self):
        """(largest sum of absolute terms) / quantum of each of the four sums, at the larger scale."""
        return {"gS2 W2^T": (np.abs(self.gS) @ np.abs(self.W).T).max() / (Q_GS * Q_W),
                "H1^T gS2": (np.abs(self.H).T @ np.abs(self.gS)).max() / (Q_H * Q_GS),
                "colsum gZ1": np.abs(self.gZ(max(SCALES))).sum(0).max() / (Q_GS * Q_W),
                "colsum G": np.abs(self.G).sum(0).max() / Q_G}


@functools.lru_cache(maxsize=None)
def problem(case):
    return Problem(case)


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_case_inputs_are_exact_in_fp32(case):
    """The precondition, on the float64 reference alone (no GPU): every sum's
    absolute terms stay below 2^24 quanta, and H holds what the kernel must
    tell apart (positive, +0, -0, negative)."""
    pb = problem(case)
    worst = pb.exactness_ratio()
    name = max(worst, key=worst.get)
    print(f"{case.name}: max ratio / 2^24 = {worst[name] / 2**24:.5f} ({name})")
    assert worst[name] < 2**24, (name, worst[name])
    for x in (pb.H, pb.gS, pb.W, pb.G):
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    if case.M * case.N >= 200:
        neg0 = (pb.H == 0) & np.signbit(pb.H)
        assert neg0.any() and ((pb.H == 0) & ~np.signbit(pb.H)).any() and (pb.H < 0).any() and (pb.H > 0).any()
        assert np.signbit(pb.H.astype(np.float32)[neg0]).all()
        assert (pb.T[pb.H <= 0] != 0).any()        # a gZ1 that is 0 only because of H


# ------------------------------------------------------------------------------ GPU: every case, exactly

def _embed(vals, ld, off):
    """fp32 [GUARD | off | rows x ld | GUARD] floats, all NaN but vals in the first columns of each row."""
    rows, cols = vals.shape
    flat = np.full(GUARD + off + rows * ld + GUARD, np.nan, np.float32)
    flat[GUARD + off:GUARD + off + rows * ld].reshape(rows, ld)[:, :cols] = vals
    return flat


def _ptr(t, off=0):
    assert t.data_ptr() % 16 == 0
    return ctypes.c_void_p(t.data_ptr() + 4 * (GUARD + off))


@functools.lru_cache(maxsize=2)
def _inputs(c):
    pb = problem(c)
    return tuple(torch.from_numpy(_embed(v, ld, off)).to(DEV) for v, ld, off in
                 ((pb.H, c.ldh, c.h_off), (pb.gS, c.ldgs, 0), (pb.W, c.ldw, c.w_off), (pb.G, c.ldg, 0)))


def _call(c, scale, want=("gw", "gb1", "g")):
    """One call on NaN-filled outputs and workspace; the buffers afterwards, as host arrays.
    want: which of gW, gb1 and G (hence gb2) are passed; the others are null."""
    lib = _lib.load()
    H, gS, W, G = _inputs(c)
    wsb = lib.gcnk_gcn_bwd2_workspace_bytes(c.M, c.N, c.P)
    assert wsb > 0 and wsb % 16 == 0
    nan = float("nan")
    bufs = {"z": torch.full((2 * GUARD + c.z_off + c.M * c.ldz,), nan, device=DEV),
            "gw": torch.full((2 * GUARD + c.N * c.P,), nan, device=DEV),
            "gb1": torch.full((2 * GUARD + c.N,), nan, device=DEV),
            "gb2": torch.full((2 * GUARD + c.P,), nan, device=DEV),
            "ws": torch.full((2 * GUARD + wsb // 4,), nan, device=DEV)}
    rc = lib.gcnk_gcn_bwd2_f32(
        _ptr(H, c.h_off), c.ldh, _ptr(gS), c.ldgs, _ptr(W, c.w_off), c.ldw, _ptr(G) if "g" in want else None, c.ldg,
        c.M, c.N, c.P, scale, _ptr(bufs["z"], c.z_off), c.ldz, _ptr(bufs["gw"]) if "gw" in want else None,
        _ptr(bufs["gb1"]) if "gb1" in want else None, _ptr(bufs["gb2"]), _ptr(bufs["ws"]), wsb,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "gcnk_gcn_bwd2_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _check(c, got, scale, want=("gw", "gb1", "g")):
    """Every requested output equals float64; everything else is still NaN."""
    pb = problem(c)
    what = f"{c.name} scale={scale} want={want}"
    zref = pb.gZ(scale)
    z0 = GUARD + c.z_off
    z = got["z"][z0:z0 + c.M * c.ldz].reshape(c.M, c.ldz)
    _equal(z[:, :c.N], zref, f"gZ1 ({what})")
    assert np.isnan(z[:, c.N:]).all(), f"gZ1's padding columns were written ({what})"
    assert np.isnan(got["z"][:z0]).all() and np.isnan(got["z"][z0 + c.M * c.ldz:]).all(), f"around gZ1 ({what})"
    for key, n, ref, asked in (("gw", c.N * c.P, pb.gW.reshape(-1), "gw" in want),
                               ("gb1", c.N, zref.sum(0), "gb1" in want), ("gb2", c.P, pb.gb2, "g" in want)):
        body = got[key][GUARD:GUARD + n]
        if asked:
            _equal(body, ref, f"{key} ({what})")
        else:
            assert np.isnan(body).all(), f"{key} was not asked for and was written ({what})"
        assert np.isnan(got[key][:GUARD]).all() and np.isnan(got[key][GUARD + n:]).all(), f"around {key} ({what})"
    assert np.isnan(got["ws"][:GUARD]).all() and np.isnan(got["ws"][-GUARD:]).all(), f"around the workspace ({what})"


@pytest.mark.gpu
@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_bwd2_case_equals_float64(case):
    """gZ1, gW2, gb1 and gb2 (gb2 where the case has G) equal float64 at scale
    2 and at scale 1; a second call is bitwise the first, workspace included."""
    want = ("gw", "gb1", "g") if case.with_g else ("gw", "gb1")
    for scale in SCALES:
        got = _call(case, scale, want)
        _check(case, got, scale, want)
        again = _call(case, scale, want)
        for k in got:
            assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), f"{k}: two calls, different bits"


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(NULLABLE))
@pytest.mark.parametrize("case", bc.NULLABLE_CASES, ids=lambda c: c.name)
def test_bwd2_nullable_outputs(case, which):
    """gW null, gb1 null, G null (no gb2) and all three null, on one case of
    several slices per column path: the others still equal float64 and a buffer
    that was not asked for keeps its NaN."""
    want = NULLABLE[which]
    got = _call(case, 2.0, want)
    _check(case, got, 2.0, want)
