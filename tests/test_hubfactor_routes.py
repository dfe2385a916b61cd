"""Every instantiation of the factored gc1 kernel (gcnk_hubfactor_gc1_f32,
csrc/factor.hip) and both ways it reads U, against float64.

CPU (unmarked): gcnk_hubfactor_gc1_route -- the host function the launch is
made from -- says what each case of tests/hubfactor_cases.py reaches: each case
must reach the route it names, and the table all 24 instantiations
hubfactor_gc1_kernel<KS, NTQ, NP>, U staged in LDS and loaded directly at every
KS (directly both for an ldu that is no multiple of 4 and for the LDS budget),
and Kc, F and P on both sides of every cut.

GPU: every case on the hand-built operands of tests/test_hubfactor_items.py
(hubfactor_cases.operands: M = 70 in three blocks, the last ragged; a permuted
block order; item counts 0 .. 17 and one row of 200; NaN bits in every record
tail and in U's columns past Kc; W1's rows from k0 = 3; sentinel rows around H1
and S2; LDS filled with NaN bits before each launch), for the epilogues NONE,
BIAS and BIAS_RELU with and without the H1 store.  What the never-run
instantiations could get wrong -- the zero fill after W1[Kc], U's LDS row
stride at KS = 32, the pad at NTQ = 3 -- shows as a NaN or a wrong sum.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubfactor_cases as hc  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib  # noqa: E402

DEV = "cuda"
M, K0 = hc.M, hc.K0
GUARD = 8                    # sentinel rows before and after the outputs
SENTINEL = -12345.0
LDS_LIMIT = 160 * 1024


def _route(Kc, F, P, nhub, ldu, u_aligned16=1, rec_words=hc.REC_WORDS):
    """(rc, (KS, NTQ, NP, u_lds), LDS bytes of the launch, workgroups per 32 rows)"""
    out = (ctypes.c_int64 * 6)()
    rc = _lib.load().gcnk_hubfactor_gc1_route(F, Kc, nhub, rec_words, P, ldu, u_aligned16, out)
    return rc, tuple(out[:4]), out[4], out[5]


# ------------------------------------------------------------------------------ CPU: the route table

def test_route_refusals():
    lib = _lib.load()
    out = (ctypes.c_int64 * 6)()
    good = [200, 50, 50, 800, 8, 52, 1, out]      # F, Kc, nhub, rec_words, P, ldu, u_aligned16, out6
    assert lib.gcnk_hubfactor_gc1_route(*good) == _lib.OK
    for i, bad in ((0, 0), (1, 0), (2, 0), (4, 0), (5, 49), (3, 64), (3, 802), (7, None)):
        args = list(good)
        args[i] = bad
        assert lib.gcnk_hubfactor_gc1_route(*args) == _lib.EARG, i
        assert b"gcnk_hubfactor_gc1_route" in lib.gcnk_last_error()
    for i, bad in ((0, 202), (0, 260), (1, 129), (4, 33), (2, 400)):
        args = list(good)
        args[i] = bad
        if i == 1:
            args[5] = 132
        assert lib.gcnk_hubfactor_gc1_route(*args) == _lib.EUNSUP, i
    args = list(good)
    args[6] = 0                                    # a U off a 16-B boundary: accepted, loaded directly
    assert lib.gcnk_hubfactor_gc1_route(*args) == _lib.OK and out[3] == 0


@pytest.mark.parametrize("case", hc.CASES, ids=lambda c: c.name)
def test_case_reaches_the_route_it_names(case):
    rc, route, lds, wgs = _route(case.Kc, case.F, case.P, case.nhub, case.ldu)
    assert rc == _lib.OK, _lib.load().gcnk_last_error()
    assert route == case.route
    assert wgs == 1
    # the launch's LDS: the operands' bytes, plus U's 32 staged rows (stride 64 ceil((4 KS - 4) / 64) + 4 floats)
    base = _lib.load().gcnk_hubfactor_lds_bytes(case.F, case.Kc, case.nhub, hc.REC_WORDS, case.P)
    ks = route[0]
    u_bytes = 4 * 32 * (64 * ((4 * ks - 4 + 63) // 64) + 4)
    assert lds == base + (u_bytes if route[3] else 0) and lds <= LDS_LIMIT
    assert case.ldu >= case.Kc and case.nhub >= 1


def test_table_reaches_every_instantiation_and_cut():
    assert len(set(hc.CASES)) == len(hc.CASES) and len({c.name for c in hc.CASES}) == len(hc.CASES)
    routes = {}
    for c in hc.CASES:
        rc, route, _, _ = _route(c.Kc, c.F, c.P, c.nhub, c.ldu)
        assert rc == _lib.OK, c.name
        routes[c] = route
    assert len(hc.INSTANTIATIONS) == 24
    assert {r[:3] for r in routes.values()} == set(hc.INSTANTIATIONS)
    # U staged and U loaded directly at every KS; directly for each of the two reasons
    assert {(r[0], r[3]) for r in routes.values()} == {(ks, u) for ks in hc.KS_VALUES for u in (0, 1)}
    for ks in hc.KS_VALUES:
        direct = [c for c, r in routes.items() if r[0] == ks and not r[3]]
        assert any(c.ldu % 4 for c in direct), f"KS {ks}: no direct case by ldu"
        by_budget = [c for c in direct if c.ldu % 4 == 0]
        assert by_budget, f"KS {ks}: no direct case by the LDS budget"
        for c in by_budget:                        # ... which is the only reason left for those
            assert _lib.load().gcnk_hubfactor_lds_bytes(c.F, c.Kc, c.nhub, hc.REC_WORDS, c.P) <= LDS_LIMIT
        assert any(c.Kc % 4 for c, r in routes.items() if r[0] == ks), f"KS {ks}: no Kc % 4 != 0"
    assert {c.Kc for c in hc.CASES} >= set(hc.REQUIRED_KC)
    assert {c.F for c in hc.CASES} >= set(hc.REQUIRED_F)
    assert {c.P for c in hc.CASES} >= set(hc.REQUIRED_P)
    # the cuts are where the table says: the values on either side of each land in different instantiations
    ks_of = {c.Kc: r[0] for c, r in routes.items()}
    assert [ks_of[k] for k in hc.REQUIRED_KC] == [13, 13, 13, 18, 18, 25, 25, 32, 32, 32]
    ntq_of = {c.F: r[1] for c, r in routes.items()}
    assert [ntq_of[f] for f in hc.REQUIRED_F] == [2, 2, 3, 3, 4, 4]
    np_of = {c.P: r[2] for c, r in routes.items()}
    assert [np_of[p] for p in hc.REQUIRED_P] == [1, 1, 2, 2]
    # Kc = 128, F = 256: past the budget with U staged, inside it without
    big = [r for c, r in routes.items() if (c.Kc, c.F) == (128, 256)]
    assert big and all(r[3] == 0 for r in big)
    # the cases that fill the budget: one more hub is refused
    assert hc.LAST_HUB_CASES
    for c in hc.LAST_HUB_CASES:
        assert _route(c.Kc, c.F, c.P, c.nhub + 1, c.ldu)[0] == _lib.EUNSUP, c.name
    # the case of the refusal test is refused for LDS alone
    Kc, F, P, nhub, ldu = hc.LDS_REFUSED
    assert _route(Kc, F, P, nhub, ldu)[0] == _lib.EUNSUP
    assert _route(Kc, F, P, 7, ldu)[0] == _lib.OK
    assert _lib.load().gcnk_hubfactor_lds_bytes(F, Kc, nhub, hc.REC_WORDS, P) > LDS_LIMIT


# ------------------------------------------------------------------------------ GPU: every case against float64

@functools.lru_cache(maxsize=2)
def _problem(nhub, Kc, F, P, ldu):
    o = hc.operands(nhub, Kc, F, P, ldu)
    dev = {k: torch.from_numpy(o[k]).to(DEV) for k in ("rec", "U", "W1", "S", "b1", "W2")}
    return o, dev


def _launch(o, dev, Kc, F, P, nhub, epi, store_h1):
    """(rc, Hbuf, Cbuf): one launch into sentinel-filled outputs right after an LDS fill with NaN bits."""
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    Hbuf = torch.full((M + 2 * GUARD, F), SENTINEL, device=DEV)
    Cbuf = torch.full((M + 2 * GUARD, P), SENTINEL, device=DEV)
    H1, S2 = Hbuf[GUARD:GUARD + M], Cbuf[GUARD:GUARD + M]
    assert dev["U"].data_ptr() % 16 == 0
    _lib.check(lib.gcnk_debug_poison_lds(0xFFFFFFFF, stream), "gcnk_debug_poison_lds")
    rc = lib.gcnk_hubfactor_gc1_f32(
        M, F, Kc, nhub, P, p(dev["U"]), o["ldu"], p(dev["W1"]), F, K0, p(dev["S"]), F, p(dev["rec"]),
        o["rec_words"], p(dev["b1"]), epi, None, 0, 1.0, 1.0, 0, 0, None, p(dev["W2"]), P,
        p(H1) if store_h1 else None, F, p(S2), P, stream)
    torch.cuda.synchronize()
    return rc, Hbuf, Cbuf


@pytest.mark.gpu
@pytest.mark.parametrize("case", hc.CASES, ids=lambda c: c.name)
def test_hubfactor_case_against_float64(case):
    """H1 and S2 of every one of the M rows against float64 within
    2e-5 max(1, max|ref|) (the bound of tests/test_hubfactor_items.py), for
    every non-dropout epilogue with and without the H1 store; finite outputs;
    S2 the same bits with and without the H1 store; a second identical launch
    the same bits; nothing written outside the rows the record names."""
    Kc, F, P, nhub = case.Kc, case.F, case.P, case.nhub
    o, dev = _problem(nhub, Kc, F, P, case.ldu)
    assert o["rec_words"] == hc.REC_WORDS
    W2d = o["W2"].astype(np.float64)

    def launch(epi, store_h1):
        rc, Hbuf, Cbuf = _launch(o, dev, Kc, F, P, nhub, epi, store_h1)
        _lib.check(rc, "gcnk_hubfactor_gc1_f32")
        # the -1 row ids and everything else the record does not name: untouched
        for buf in (Hbuf, Cbuf):
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + M:] == SENTINEL).all())
        if not store_h1:
            assert bool((Hbuf == SENTINEL).all())
        return Hbuf[GUARD:GUARD + M], Cbuf[GUARD:GUARD + M]

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
        print(f"{case.name} epi {epi}: H1 max err {err1:.3e} (tol {tol1:.3e}), "
              f"S2 max err {err2:.3e} (tol {tol2:.3e})")
        assert err1 <= tol1, (epi, err1, tol1)
        assert err2 <= tol2, (epi, err2, tol2)
        assert torch.equal(S2n, S2), epi
        H1b, S2b = launch(epi, True)
        assert torch.equal(H1b.view(torch.int32), H1.view(torch.int32)), epi
        assert torch.equal(S2b.view(torch.int32), S2.view(torch.int32)), epi


REFUSED = {"lds": hc.LDS_REFUSED, "Kc129": (129, 64, 8, 7, 132), "F260": (50, 260, 8, 7, 52),
           "P33": (50, 64, 33, 7, 52)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(REFUSED))
def test_hubfactor_refusals_leave_outputs_untouched(which):
    """More than 160 KiB of LDS, Kc = 129, F = 260 and P = 33: GCNK_EUNSUP from
    the entry point as from the route report, nothing written."""
    Kc, F, P, nhub, ldu = REFUSED[which]
    assert _route(Kc, F, P, nhub, ldu)[0] == _lib.EUNSUP
    o, dev = _problem(nhub, Kc, F, P, ldu)
    for store_h1 in (True, False):
        rc, Hbuf, Cbuf = _launch(o, dev, Kc, F, P, nhub, _lib.EPI_BIAS_RELU, store_h1)
        assert rc == _lib.EUNSUP
        assert bool((Hbuf == SENTINEL).all()) and bool((Cbuf == SENTINEL).all())
