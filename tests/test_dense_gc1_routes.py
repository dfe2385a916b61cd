"""Every instantiation of the narrow-feature gc1 kernel (gcnk_dense_gc1_f32,
csrc/dense_gc1.hip), by bits.

CPU (unmarked): gcnk_dense_gc1_route -- the host function the launch is made
from -- says what each case of tests/dense_gc1_cases.py reaches: each case must
reach the route it names, and the table all 18 instantiations
dense_gc1_kernel<KS, NI, NPM, PV> and K, F and P on both sides of every cut.
The entry point's own refusals (alignment, leading dimensions, null operands,
the 32-bit offset limits) come before any HIP call.

GPU: the library called through ctypes on operands that are views into
NaN-filled parents (dense_gc1_cases.operands: NaN in AX's columns K .. ldax - 1
and its rows around M, in every row pad and guard row of W1 / W2, around b1),
outputs inside sentinel-filled parents, LDS filled with NaN bits before every
launch.  The inputs sit on binary quanta where every fp32 sum is exact in any
order (asserted per case on the float64 reference alone), so H1 and S2 must
EQUAL float64 -- whichever instantiation, tail wave, LDS buffer or slot order
ran.  One dropped k-step, column, slot or row shows, however small; a read one
element outside an operand shows as a NaN.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_gc1_cases as dc  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib  # noqa: E402
from oracle import hash_ref  # noqa: E402

DEV = "cuda"
NAME = "gcnk_dense_gc1_f32"
PTR = 0x10000   # a 16-byte aligned address that no refused call dereferences
G, SENTINEL, SCALE = dc.GUARD, dc.SENTINEL, dc.SCALE


def _route(M, K, F, P):
    out = (ctypes.c_int64 * 6)()
    rc = _lib.load().gcnk_dense_gc1_route(M, K, F, P, out)
    return rc, tuple(out)


# ------------------------------------------------------------------------------ CPU: the route table

def test_route_refusals():
    lib = _lib.load()
    out = (ctypes.c_int64 * 6)()
    good = [515, 50, 200, 8, out]                  # M, K, F, P, out6
    assert lib.gcnk_dense_gc1_route(*good) == _lib.OK and tuple(out) == (13, 3, 1, 0, 1, 33)
    for i, bad in ((4, None), (0, 0), (1, 0), (2, 0), (3, 0), (0, -1), (1, -4), (2, -4), (3, -1)):
        args = list(good)
        args[i] = bad
        assert lib.gcnk_dense_gc1_route(*args) == _lib.EARG, (i, bad)
        assert b"gcnk_dense_gc1_route" in lib.gcnk_last_error()
    for i, bad in ((1, 129), (2, 260), (2, 6), (3, 33)):
        args = list(good)
        args[i] = bad
        assert lib.gcnk_dense_gc1_route(*args) == _lib.EUNSUP, (i, bad)
        assert b"gcnk_dense_gc1_route" in lib.gcnk_last_error()
    assert _route(2**31 - 1, 128, 256, 32) == (_lib.OK, (32, 4, 2, 0, 0, 2**27))   # ntiles without overflow


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_reaches_the_route_it_names(case):
    rc, route = _route(case.M, case.K, case.F, case.P)
    assert rc == _lib.OK, _lib.load().gcnk_last_error()
    assert route == case.route
    assert route[4] == int(route[1] == 3 and case.F > 192) and route[5] == (case.M + 15) // 16
    # every case is strided, the way the table says
    assert case.ldax in (case.K + 1, (case.K + 3) // 4 * 4 + 4) and case.ldax > case.K
    assert (case.ldw1, case.ldw2, case.ldh, case.ldc2, case.ldm) == (case.F + 4, case.P + 3, case.F + 4, case.P + 5,
                                                                     case.F + 3)
    if route[4]:
        assert case.M == dc.TAIL_M


def test_table_reaches_every_instantiation_and_cut():
    cases = dc.CASES
    assert len(set(cases)) == len(cases) and len({c.name for c in cases + dc.PERSISTENT_CASES}) == len(cases) + 2
    routes = {}
    for c in cases:
        rc, routes[c] = _route(c.M, c.K, c.F, c.P)
        assert rc == _lib.OK, c.name
    assert len(dc.INSTANTIATIONS) == len(set(dc.INSTANTIATIONS)) == 18
    assert {r[:4] for r in routes.values()} == set(dc.INSTANTIATIONS)
    # the required values, on both NI where reachable
    assert {c.K for c in cases} >= set(dc.REQUIRED_K)
    assert {c.F for c, r in routes.items() if r[1] == 3} >= set(dc.REQUIRED_F_NI3)
    assert {c.F for c, r in routes.items() if r[1] == 4} >= set(dc.REQUIRED_F_NI4)
    assert {c.P for c, r in routes.items() if r[1] == 3} == {p for p in dc.REQUIRED_P if p <= 20} | {8}
    assert {c.P for c, r in routes.items() if r[1] == 4} >= set(dc.REQUIRED_P)
    assert {c.M for c in cases} >= set(dc.REQUIRED_M)
    for ks in dc.KS_VALUES:
        assert any(c.K % 4 for c, r in routes.items() if r[0] == ks), f"KS {ks}: no K % 4 != 0"
    # both kinds of ldax on every KS, the odd one and the multiple of 4
    for ks in dc.KS_VALUES:
        lds = {c.ldax % 4 == 0 and c.ldax > c.K + 1 for c, r in routes.items() if r[0] == ks}
        assert lds == {True, False}, ks
    # the tail: 4, 8, 12 and 16 columns, each at M = 515; with and without the VALU columns
    tails = [c for c, r in routes.items() if r[4]]
    assert {c.F for c in tails} == {196, 200, 204, 208} and {c.M for c in tails} == {dc.TAIL_M}
    assert {routes[c][3] for c in tails} == {0, 4}
    first_rot = {((b >> 3) + (b >> 8)) & 3 for b in range((dc.TAIL_M + 15) // 16)}
    assert first_rot == {0, 1, 2, 3}
    # the NI = 3 shift: F % 3 == 1 (shift 2) and F % 3 == 2 (shift 1) below 192
    ni3 = [c for c, r in routes.items() if r[1] == 3 and c.F < 192]
    assert any(c.F % 3 == 1 for c in ni3) and any(c.F % 3 == 2 for c in ni3)
    # the cuts are where the table says: the values on either side of each land in different instantiations
    ks_of = {c.K: r[0] for c, r in routes.items()}
    assert [ks_of[k] for k in dc.REQUIRED_K] == list(dc.REQUIRED_K_KS)
    for (a, b) in ((32, 33), (52, 53), (64, 65), (100, 101)):
        assert _route(70, a, 200, 8)[1][:4] != _route(70, b, 200, 8)[1][:4]
    assert _route(70, 50, 208, 8)[1][:4] == (13, 3, 1, 0) and _route(70, 50, 212, 8)[1][:4] == (13, 4, 1, 0)
    assert _route(70, 50, 192, 8)[1][4] == 0 and _route(70, 50, 196, 8)[1][4] == 1
    assert _route(70, 50, 200, 16)[1][:4] == (13, 3, 1, 0) and _route(70, 50, 200, 17)[1][:4] == (13, 3, 1, 4)
    assert _route(70, 50, 200, 20)[1][:4] == (13, 3, 1, 4) and _route(70, 50, 200, 21)[1][:4] == (13, 4, 2, 0)
    assert _route(70, 50, 256, 16)[1][:4] == (13, 4, 1, 0) and _route(70, 50, 256, 17)[1][:4] == (13, 4, 2, 0)
    assert _route(70, 100, 200, 8)[1][1] == 3 and _route(70, 101, 200, 8)[1][1] == 4      # KS 32 has no NI = 3
    for f, pairs in ((dc.REQUIRED_F_NI3, ((192, 196),)), (dc.REQUIRED_P, ((16, 17), (20, 21)))):
        assert all(a in f and b in f for a, b in pairs)
    # the persistent cases name what the issue's shapes reach, at any CU count
    for c, inst in zip(dc.PERSISTENT_CASES, ((8, 3, 1, 4, 1), (13, 4, 2, 0, 0))):
        assert c.M == 0 and c.route[:5] == inst
        for cus in (1, 80, 256, 304):
            m = dc.persistent_M(cus)
            rc, route = _route(m, c.K, c.F, c.P)
            assert rc == _lib.OK and route == dc.with_M(c, m).route
            tiles, grid = route[5], 2 * cus
            assert tiles == 4 * grid + 4 and m % 16 == 5          # four workgroups run five tiles, the rest four
    assert {routes[c][:5] for c in dc.NAN_ROW_CASES} == {(25, 4, 1, 0, 0), (13, 3, 1, 0, 0), (13, 3, 1, 0, 1)}


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_inputs_are_exact_in_fp32(case):
    """The precondition of comparing by bits, on the float64 reference alone (operands asserts it)."""
    o = dc.operands(case)
    print(f"{case.name}: bits {o['bits']}, kept by the mask {o['mask'].mean():.3f}")
    assert np.isnan(o["AXp"][:G]).all() and np.isnan(o["AXp"][G + case.M:]).all()
    assert np.isnan(o["AXp"][:, case.K:]).all() and not np.isnan(o["AXp"][G:G + case.M, :case.K]).any()
    for key, rows, cols in (("W1p", case.K, case.F), ("W2p", case.F, case.P)):
        p = o[key]
        assert np.isnan(p[:G]).all() and np.isnan(p[G + rows:]).all() and np.isnan(p[:, cols:]).all()
        assert p.shape[1] > cols and not np.isnan(p[G:G + rows, :cols]).any()
    assert np.isnan(o["b1p"][:dc.GUARD_B1]).all() and np.isnan(o["b1p"][-dc.GUARD_B1:]).all()
    assert (o["maskp"][:, case.F:] == 255).all() and np.abs(o["b1"]).max() == 4.0


def _entry(M=70, K=50, F=200, P=8, AX=PTR, ldax=51, W1=PTR, ldw1=204, b1=PTR, epi=None, mask=None, ldm=0, W2=PTR,
           ldw2=11, H=PTR, ldh=204, C2=PTR, ldc2=13):
    lib = _lib.load()
    rc = lib.gcnk_dense_gc1_f32(M, K, F, P, AX, ldax, W1, ldw1, b1, _lib.EPI_BIAS_RELU if epi is None else epi, mask,
                                ldm, 1.0, 1.0, 0, 0, None, W2, ldw2, H, ldh, C2, ldc2, None)
    return rc, lib.gcnk_last_error().decode()


@pytest.mark.parametrize("kw", [dict(ldw1=202), dict(ldw1=205), dict(W1=PTR + 4), dict(W1=PTR + 8), dict(b1=PTR + 4),
                                dict(H=PTR + 8), dict(ldh=206), dict(ldh=201), dict(K=129, ldax=132),
                                dict(F=260, ldw1=260, ldh=260), dict(F=6, ldw1=8, ldh=8), dict(P=33, ldw2=36, ldc2=36),
                                dict(ldax=0x7ff00000 // 64), dict(K=128, ldax=128, ldw1=2**22),
                                dict(F=256, ldw1=256, ldh=256, ldw2=2**21)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_entry_refuses_unsupported_before_any_launch(kw):
    """ldw1 % 4, W1 / b1 / H off 16 bytes, ldh % 4, the route's own refusals, and 16 ldax 4, K ldw1 4 and F ldw2 4
    bytes past their 32-bit limits: GCNK_EUNSUP on pointers nothing may read."""
    rc, msg = _entry(**kw)
    assert rc == _lib.EUNSUP and NAME in msg


def test_entry_32_bit_limits_are_where_the_kernel_needs_them():
    """One below each limit passes the shape checks (and is refused only by the epilogue code, still before
    any launch): a tile of A, 16 ldax 4 bytes, ends below the offset 0x7ff00000 that turns a lane off, and W1's and
    W2's byte offsets fit 31 bits."""
    bad_epi = dict(epi=_lib.EPI_NONE)
    for kw in (dict(ldax=0x7ff00000 // 64 - 1), dict(K=128, ldax=128, ldw1=2**22 - 4),
               dict(F=256, ldw1=256, ldh=256, ldw2=2**21 - 1)):
        rc, msg = _entry(**kw, **bad_epi)
        assert rc == _lib.EARG and "epilogue" in msg, kw
    assert _entry(epi=_lib.EPI_BIAS_RELU_DROP, mask=PTR, ldm=199)[0] == _lib.EARG     # a mask row shorter than F
    assert _entry(epi=_lib.EPI_BIAS_RELU_DROP, mask=None, ldm=200)[0] == _lib.EARG


@pytest.mark.parametrize("kw", [dict(ldax=49), dict(ldw1=196), dict(ldw2=7), dict(ldh=196), dict(ldc2=7),
                                dict(AX=None), dict(W1=None), dict(W2=None), dict(C2=None), dict(M=0), dict(K=0),
                                dict(F=0), dict(P=0), dict(M=-1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_entry_refuses_bad_arguments_before_any_launch(kw):
    """Each leading dimension shorter than its row, each null operand, each size <= 0: GCNK_EARG."""
    rc, msg = _entry(**kw)
    assert rc == _lib.EARG and NAME in msg


# ------------------------------------------------------------------------------ GPU: every case, by bits

def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _resolve(case):
    """The case itself; a persistent case with its M from the device, its route checked here."""
    if case.M:
        return case
    cus = _cus()
    c = dc.with_M(case, dc.persistent_M(cus))
    rc, route = _route(c.M, c.K, c.F, c.P)
    assert rc == _lib.OK and route == c.route
    assert route[5] == 4 * (2 * cus) + 4, "four workgroups run five tiles, the rest four"
    return c


class Problem:
    """A case's operands on the device, and launches into fresh sentinel-filled output parents."""

    def __init__(self, c):
        self.c, self.o = c, dc.operands(c)
        self.dev = {k: torch.from_numpy(self.o[k]).to(DEV) for k in ("AXp", "W1p", "W2p", "b1p", "maskp")}
        ones = np.full_like(self.o["maskp"], 255)
        ones[G:G + c.M, :c.F] = 1
        self.dev["onesp"] = torch.from_numpy(ones).to(DEV)

    def ptr(self, key, skip):
        t = self.dev[key]
        assert t.data_ptr() % 16 == 0
        return ctypes.c_void_p(t.data_ptr() + t.element_size() * skip)

    def launch(self, epi, bias=True, store=True, mask="maskp", scale=SCALE, AXp=None):
        """One launch right after an LDS fill with NaN bits -> (H1 or None, S2) as host arrays [M x F], [M x P];
        everything around them must still be the sentinel, by bits."""
        c, lib = self.c, _lib.load()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        Hbuf = torch.full((c.M + 2 * G, c.ldh), SENTINEL, device=DEV)
        Cbuf = torch.full((c.M + 2 * G, c.ldc2), SENTINEL, device=DEV)
        seed, offset, ldm_hash, base = dc.hash_args(c)
        bt = torch.tensor([base], dtype=torch.int64, device=DEV)
        hashed, dropped = epi == _lib.EPI_BIAS_RELU_HASH, epi == _lib.EPI_BIAS_RELU_DROP
        ax = self.dev["AXp"] if AXp is None else AXp
        assert Hbuf.data_ptr() % 16 == 0 and (G * c.ldh) % 4 == 0 and (G * c.ldw1) % 4 == 0
        _lib.check(lib.gcnk_debug_poison_lds(0xFFFFFFFF, stream), "gcnk_debug_poison_lds")
        rc = lib.gcnk_dense_gc1_f32(
            c.M, c.K, c.F, c.P, ctypes.c_void_p(ax.data_ptr() + 4 * G * c.ldax), c.ldax, self.ptr("W1p", G * c.ldw1),
            c.ldw1, self.ptr("b1p", dc.GUARD_B1) if bias else None, epi,
            self.ptr(mask, G * c.ldm) if dropped else None, c.ldm if dropped else ldm_hash if hashed else 0,
            scale, 0.5 if hashed else 1.0, seed if hashed else 0, offset if hashed else 0,
            ctypes.c_void_p(bt.data_ptr()) if hashed else None, self.ptr("W2p", G * c.ldw2), c.ldw2,
            ctypes.c_void_p(Hbuf.data_ptr() + 4 * G * c.ldh) if store else None, c.ldh,
            ctypes.c_void_p(Cbuf.data_ptr() + 4 * G * c.ldc2), c.ldc2, stream)
        _lib.check(rc, NAME)
        torch.cuda.synchronize()
        assert int(bt.item()) == base, "the kernel only reads *rng_base"
        Hn, Cn = Hbuf.cpu().numpy(), Cbuf.cpu().numpy()
        sent = np.float32(SENTINEL).view(np.int32)
        for what, buf, cols in (("H1", Hn, c.F if store else 0), ("S2", Cn, c.P)):
            bits = buf.view(np.int32)
            assert (bits[:G] == sent).all() and (bits[G + c.M:] == sent).all(), f"{c.name}: {what}'s guard rows written"
            assert (bits[:, cols:] == sent).all(), f"{c.name}: {what}'s padding written"
        return (Hn[G:G + c.M, :c.F] if store else None), Cn[G:G + c.M, :c.P]


@functools.lru_cache(maxsize=2)
def _problem(case):
    return Problem(_resolve(case))


def _equal(got, ref64, what):
    """got (fp32) is float64's answer, bit for bit."""
    want = np.asarray(ref64, np.float64).astype(np.float32)
    g, w = np.ascontiguousarray(got).view(np.int32), want.view(np.int32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        r, col = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {w.size} elements differ from float64; rows "
                             f"{sorted({int(b[0]) for b in bad})[:8]}, columns {sorted({int(b[1]) for b in bad})[:8]}; "
                             f"first ({r}, {col}): got {got[r, col]!r}, want {want[r, col]!r}")


def _same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32)), what


ALL_CASES = dc.CASES + dc.PERSISTENT_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_dense_gc1_bias_relu_equals_float64(case):
    """GCNK_EPI_BIAS_RELU with H1 stored: H1 and S2 equal float64; padding and guard rows untouched (launch); a
    second launch the same bits; S2 the same bits without the H1 store; b1 null: the answers without bias."""
    pb = _problem(case)
    c, ref = pb.c, pb.o["ref"]
    H1, S2 = pb.launch(_lib.EPI_BIAS_RELU)
    _equal(H1, ref[True, False][0], f"{c.name} H1")
    _equal(S2, ref[True, False][1], f"{c.name} S2")
    H1b, S2b = pb.launch(_lib.EPI_BIAS_RELU)
    _same_bits(H1b, H1, f"{c.name}: H1 of two launches")
    _same_bits(S2b, S2, f"{c.name}: S2 of two launches")
    Hn, S2n = pb.launch(_lib.EPI_BIAS_RELU, store=False)
    assert Hn is None
    _same_bits(S2n, S2, f"{c.name}: S2 without the H1 store")
    H1z, S2z = pb.launch(_lib.EPI_BIAS_RELU, bias=False)
    _equal(H1z, ref[False, False][0], f"{c.name} H1, b1 null")
    _equal(S2z, ref[False, False][1], f"{c.name} S2, b1 null")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_dense_gc1_mask_dropout_equals_float64(case):
    """GCNK_EPI_BIAS_RELU_DROP with a uint8 mask of ldm = F + 3 at scale 2: H1 = ref mask 2 and S2 from it."""
    pb = _problem(case)
    c, ref = pb.c, pb.o["ref"]
    H1, S2 = pb.launch(_lib.EPI_BIAS_RELU_DROP)
    _equal(H1, ref[True, True][0], f"{c.name} H1")
    _equal(S2, ref[True, True][1], f"{c.name} S2")
    _, S2n = pb.launch(_lib.EPI_BIAS_RELU_DROP, store=False)
    _same_bits(S2n, S2, f"{c.name}: S2 without the H1 store")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_dense_gc1_hash_dropout_equals_float64(case):
    """GCNK_EPI_BIAS_RELU_HASH at keep 0.5 and scale 2, the case's own (seed with high bits set, offset, ldm, device
    rng_base): the kept set is oracle.hash_ref's at every element, the values equal, and S2 from it."""
    pb = _problem(case)
    c, o = pb.c, pb.o
    seed, offset, ldm, base = dc.hash_args(c)
    assert seed >> 32 and ldm > c.F
    keep = hash_ref.keep_mask(seed, base, offset, c.M, c.F, ldm, 0.5)
    assert 0.4 <= keep.mean() <= 0.6 or keep.size < 200
    Href = np.where(keep, o["ref"][True, False][0] * SCALE, 0.0)
    H1, S2 = pb.launch(_lib.EPI_BIAS_RELU_HASH)
    live = o["pre"][True] > 0
    assert np.array_equal((H1 != 0)[live], keep[live]), f"{c.name}: kept set against the contract"
    _equal(H1, Href, f"{c.name} H1")
    _equal(S2, Href @ o["W2"] + 0.0, f"{c.name} S2")
    _, S2n = pb.launch(_lib.EPI_BIAS_RELU_HASH, store=False)
    _same_bits(S2n, S2, f"{c.name}: S2 without the H1 store")


@pytest.mark.gpu
@pytest.mark.parametrize("case", dc.NAN_ROW_CASES, ids=lambda c: c.name)
def test_nan_in_one_row_of_ax_stays_in_that_row(case):
    """A NaN in one element of AX row r: every other row of H1 and S2 keeps its bits, and row r is the same bits
    under BIAS_RELU (fmaxf) as under BIAS_RELU_DROP with an all-ones mask at scale 1 (v > 0 ? v : 0).  Both turn the
    NaN pre-activation into 0 where torch.relu keeps it: row r is printed, not compared with a
    reference."""
    pb = _problem(case)
    c = pb.c
    r, k = c.M - 3, c.K - 1
    H1, S2 = pb.launch(_lib.EPI_BIAS_RELU)
    ax = pb.dev["AXp"].clone()
    ax[G + r, k] = float("nan")
    Hn, Sn = pb.launch(_lib.EPI_BIAS_RELU, AXp=ax)
    Hd, Sd = pb.launch(_lib.EPI_BIAS_RELU_DROP, mask="onesp", scale=1.0, AXp=ax)
    others = np.arange(c.M) != r
    for what, got, was in (("H1", Hn, H1), ("S2", Sn, S2), ("H1 (all-ones mask)", Hd, H1),
                           ("S2 (all-ones mask)", Sd, S2)):
        _same_bits(got[others], was[others], f"{c.name}: {what} of the rows without the NaN")
    print(f"{c.name}: row {r} with a NaN in AX[{r}, {k}]: H1 NaN {int(np.isnan(Hn[r]).sum())} zero "
          f"{int((Hn[r] == 0).sum())} of {c.F}; S2 {Sn[r].tolist()}")
    _same_bits(Hd[r], Hn[r], f"{c.name}: row {r} of H1 under the two ReLU forms")
    _same_bits(Sd[r], Sn[r], f"{c.name}: row {r} of S2 under the two ReLU forms")
