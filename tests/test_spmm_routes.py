"""Every route of gcnk_spmm_csr_f32, gcnk_spmm_csr_f32_part and gcnk_spmm_proj_f32, on the GPU.

tests/spmm_cases.py is the case table; tests/test_spmm_cases.py checks on the
CPU, through gcnk_spmm_route, that it reaches every reachable instantiation
csrc/spmm.hip compiles.  Here every case runs under the five epilogue codes against float64
(oracle/csr_ref.py on the B rows the operand references, gathered into a
compact matrix).  B and C are views into wider buffers: B's padding and every
B row no nonzero references hold NaN, C's padding a sentinel that must stay
bitwise untouched; the result must be finite and a second call bitwise equal.
GCNK_EPI_BIAS_RELU_HASH goes through test_hash_dropout's device (a bias clear
of the ReLU, _arg_sets, _check_kernel): the mask against oracle/hash_ref.py
at every element with no tolerance, in every column window and with ldm != F.
Bounds, those of the existing float64 tests of the same kernels:
  row kernel, tile   |err| <= 2e-5 sqrt(max row degree) + 1e-5 |ref|
  projection         H: 2e-5 + 1e-5 |ref|;  S2 = H W: 2e-4 + 1e-5 |ref|
  HASH               test_hash_dropout's: the above times the dropout scale; S2: 2e-4 max(1, scale max|pre|)
Largest errors observed on an MI355X (profiles/r25_spmm_routes.log), NONE to DROP epilogues:
  row kernel (R, one window)      3.3e-05  (0.023 of the bound)    column windows   3.3e-05  (0.029)
  row kernel, offsets past 2^32   3.0e-05  (0.022)                 tile + row (T)   3.5e-05  (0.042)
  projection H                    2.7e-05  (0.76 at worst)         projection S2    2.7e-04  (0.61 at worst)
The sums' bound is the existing tests' and loose for these operands; what the cases pin is the routing: a mask
or hash offset that does not shift with the column window fails the window cases, and 32-bit gather offsets
launched past 4 GiB fail all twenty K = 2^20 + 16 cases at the float64 comparison (errors of 2e+01 to 7e+01:
the wrapped offsets land on other referenced rows); four such mutations, profiles/r25_spmm_routes.log.  No case
failed on the library as it was.
"""
import ctypes
import functools
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmm_cases as sc  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib, from_arrays  # noqa: E402
from graph_convolutional_networks_for_text_classification_amd.ops import _ptr, _stream  # noqa: E402
from oracle import csr_ref  # noqa: E402

from test_hash_dropout import SCALE as HASH_SCALE, _bias_clear_of_relu, _check_kernel  # noqa: E402
from test_spmm_cases import ALIGN_BIT, groups_of, ipc_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.0
DROP_SCALE = 1.5
EPI_CODE = {"none": _lib.EPI_NONE, "bias": _lib.EPI_BIAS, "bias_relu": _lib.EPI_BIAS_RELU,
            "drop": _lib.EPI_BIAS_RELU_DROP, "hash": _lib.EPI_BIAS_RELU_HASH}


@functools.lru_cache(maxsize=None)
def _device_csr(operand):
    rp, ci, v, shape = sc.operand(operand)
    return from_arrays(rp, ci, v, shape, DEV)


def _flat_view(rows, ld, cols, fill, misaligned):
    """(flat buffer, its [rows x ld] matrix, the [rows x cols] view) on the device, filled with `fill`; the view's
    base is 4 bytes past a 16-byte boundary when `misaligned`."""
    off = 1 if misaligned else 0
    flat = torch.full((rows * ld + 4,), fill, dtype=torch.float32, device=DEV)
    mat = flat[off:off + rows * ld].view(rows, ld)
    view = mat[:, :cols]
    assert view.stride(0) == ld and (view.data_ptr() % 16 != 0) == misaligned
    return flat, mat, view


class _Setup:
    """A case's operands on the device and its float64 sums."""

    def __init__(self, c, big=None):
        self.c = c
        rp, ci, v, (M, K) = sc.operand(c.operand)
        self.M, self.K, self.F = M, K, c.F
        self.maxdeg = int(np.diff(rp).max())
        a = _device_csr(c.operand)
        self.plan = a.plan(ipc_of(c), groups_of(c), c.dense)
        self.rng = np.random.default_rng(zlib.crc32(c.name.encode()))
        used = np.unique(ci)
        vals = self.rng.standard_normal((len(used), c.F)).astype(np.float32)
        used_t = torch.from_numpy(used).to(DEV)
        if big is not None:
            assert K <= sc.BIG_ROWS and c.F + c.pad_b == sc.BIG_LDB and not c.misalign
            big.fill_(float("nan"))
            self.B = big[:K, :c.F]
        else:
            self._bflat, _, self.B = _flat_view(K, c.F + c.pad_b, c.F, float("nan"), c.misalign == "b_base")
        self.B[used_t] = torch.from_numpy(vals).to(DEV)
        assert self.B.stride(0) == c.F + c.pad_b and bool(torch.isnan(self.B).any()) == (len(used) < K)
        # the float64 sums, from the referenced rows of B alone (columns renumbered)
        self.acc = csr_ref.spmm_csr(rp, np.searchsorted(used, ci), v, vals.astype(np.float64))
        wsb = self.plan.workspace_bytes(c.F)
        assert wsb > 0 or c.misalign != "ws_base"
        self.wsb = wsb
        if wsb > 0:
            off = 1 if c.misalign == "ws_base" else 0
            self.ws = torch.empty((wsb + 3) // 4 + 4, dtype=torch.float32, device=DEV)[off:]
            assert (self.ws.data_ptr() % 16 != 0) == bool(off)
        else:
            self.ws = None
        self.cnt = self.plan.counters(self.B.device)
        if c.P:
            self.W = self.rng.standard_normal((c.F, c.P)).astype(np.float32)
            self.Wt = torch.from_numpy(self.W).to(DEV)

    def bias(self, values):
        _, _, b = _flat_view(1, self.F, self.F, 0.0, self.c.misalign == "bias_base")
        b[0] = torch.from_numpy(np.asarray(values, np.float32)).to(DEV)
        return b[0]

    def call(self, code, bias, mask=None, ldm=0, scale=1.0, keep=1.0, seed=0, offset=0, base=None, store=True,
             parts=False):
        """One product into fresh buffers: (C's [M x ldc] matrix, H view or None, S2 or None).  C's padding, the
        words around it, a C that is not to be stored and S2's padding must come back untouched."""
        c, lib = self.c, _lib.load()
        ldc = c.F + c.pad_c
        cflat, cmat, C = _flat_view(self.M, ldc, c.F, SENTINEL, c.misalign == "c_base")
        head = (_ptr(self.plan.buf), ctypes.cast(self.plan.hdr, ctypes.c_void_p), _ptr(self.B), self.B.stride(0), c.F,
                _ptr(C if store else None), ldc, _ptr(bias), code, _ptr(mask), int(ldm), float(scale), float(keep),
                int(seed), int(offset), _ptr(base))
        tail = (_ptr(self.ws), self.wsb, _ptr(self.cnt), 4 * self.cnt.numel() if self.cnt is not None else 0, c.lanes)
        st = _stream(C.device)
        S2 = None
        if c.P:
            s2flat, s2mat, S2 = _flat_view(self.M, c.P + 3, c.P, SENTINEL, False)
            rc = lib.gcnk_spmm_proj_f32(*head, _ptr(self.Wt), self.Wt.stride(0), c.P, _ptr(S2), S2.stride(0), *tail, st)
            _lib.check(rc, "gcnk_spmm_proj_f32")       # (GCNK_EUNSUP would mean the fused kernel did not run)
            assert bool((s2mat[:, c.P:] == SENTINEL).all()) and bool((s2flat[s2mat.numel():] == SENTINEL).all())
        elif parts:
            _lib.check(lib.gcnk_spmm_csr_f32_part(*head, *tail, 1, st), "gcnk_spmm_csr_f32_part 1")
            _lib.check(lib.gcnk_spmm_csr_f32_part(*head, *tail, 2, st), "gcnk_spmm_csr_f32_part 2")
        else:
            _lib.check(lib.gcnk_spmm_csr_f32(*head, *tail, st), "gcnk_spmm_csr_f32")
        off = (C.data_ptr() - cflat.data_ptr()) // 4
        pad = torch.cat([cmat[:, c.F:].reshape(-1), cflat[:off], cflat[off + cmat.numel():]])
        assert bool((pad == SENTINEL).all()), "the launch wrote outside C's view"
        if not store:
            assert bool((cflat == SENTINEL).all()), "H is not to be stored"
        return cmat, (C if store else None), S2


def _within(what, got, ref, atol):
    got = got.detach().double().cpu().numpy()
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bound = atol + 1e-5 * np.abs(ref)
    print(f"spmm {what}: max err {err.max():.3e}, err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"{what}: max err {err.max():.3e} (bound at worst {bound.flat[np.argmax(err - bound)]:.3e})"


def _check_case(c, big=None):
    s = _Setup(c, big)
    out = (ctypes.c_int32 * 16)()
    aligned = _lib.SPMM_ALIGNED_ALL & ~ALIGN_BIT.get(c.misalign, 0)
    assert _lib.load().gcnk_spmm_route(ctypes.cast(s.plan.hdr, ctypes.c_void_p), c.F, s.B.stride(0), c.F + c.pad_c,
                                       aligned, c.lanes, c.P, 0, out) == _lib.OK
    assert tuple(out)[:14] == c.route, "the device plan's route"
    assert s.plan.has_tops == c.tops
    h_atol = 2e-5 if c.P else 2e-5 * np.sqrt(s.maxdeg)
    noise = s.rng.standard_normal(c.F)
    ldm = c.F + 5
    mask = (s.rng.random((s.M, ldm)) < 0.6).astype(np.uint8)
    mask_t = torch.from_numpy(mask).to(DEV)
    for epi in sc.EPILOGUES[:4]:
        bias_t = s.bias(noise)
        bias64 = noise.astype(np.float32).astype(np.float64)
        ref = csr_ref.spmm_epilogue(s.acc, bias64 if epi != "none" else None, relu=epi in ("bias_relu", "drop"),
                                    mask=mask[:, :c.F] if epi == "drop" else None, scale=DROP_SCALE)
        kw = dict(mask=mask_t, ldm=ldm, scale=DROP_SCALE) if epi == "drop" else {}
        cmat, H, S2 = s.call(EPI_CODE[epi], bias_t, store=c.store_main, **kw)
        if H is not None:
            _within(f"{c.name} {epi} H", H, ref, h_atol)
        if c.P:
            _within(f"{c.name} {epi} S2", S2, ref @ s.W.astype(np.float64), 2e-4)
        cmat2, _, S2b = s.call(EPI_CODE[epi], bias_t, store=c.store_main, **kw)
        assert torch.equal(cmat, cmat2) and (S2 is None or torch.equal(S2, S2b)), f"{epi}: a second call differs"
        if c.two_part:
            two, _, _ = s.call(EPI_CODE[epi], bias_t, parts=True, **kw)
            assert torch.equal(two, cmat), f"{epi}: the two-part launch differs from the single one"
    # HASH: the mask at every element, in every column window, ldm != F among the argument sets
    bias, pre = _bias_clear_of_relu(s.acc, s.rng)
    bias_t = s.bias(bias)

    def run(seed, offset, base, ldm, keep, store):
        cmat, H, S2 = s.call(EPI_CODE["hash"], bias_t, None, ldm, HASH_SCALE, keep, seed, offset, base, store)
        if c.two_part:
            two, _, _ = s.call(EPI_CODE["hash"], bias_t, None, ldm, HASH_SCALE, keep, seed, offset, base, parts=True)
            assert torch.equal(two, cmat), "hash: the two-part launch differs from the single one"
        return H, S2
    if c.P:
        _check_kernel(run, pre, h_atol=2e-5 * HASH_SCALE, W2=s.W, s2_atol=2e-4 * max(1.0, HASH_SCALE * pre.max()),
                      unstored=True)
    else:
        _check_kernel(run, pre, h_atol=h_atol * HASH_SCALE)


@pytest.mark.parametrize("case", sc.SMALL_CASES, ids=lambda c: c.name)
def test_spmm_case_against_float64(case):
    _check_case(case)


@pytest.fixture(scope="module")
def big_b():
    """One [2^20 + 16 x 1024] float32 B (4 GiB + 64 KiB) for the module."""
    big = torch.empty((sc.BIG_ROWS, sc.BIG_LDB), dtype=torch.float32, device=DEV)
    yield big
    del big
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", sc.BIG_CASES, ids=lambda c: c.name)
def test_spmm_gather_offsets_at_and_past_32_bits(case, big_b):
    """B rows at byte offsets 0, 2^31 and just under K ldb 4: K = 2^20 - 1 keeps
    32-bit offsets (O32) up to just under 2^32, K = 2^20 is the first without,
    K = 2^20 + 16 gathers past 2^32."""
    _, ci, _, (_, K) = sc.operand(case.operand)
    assert ci.max() == K - 1 and (ci == 2**19).any() and ci.min() == 0
    assert (K * sc.BIG_LDB * 4 + case.F * 4 < 2**32) == (case.tag == "lo")
    assert case.tag != "hi" or (K - 1) * sc.BIG_LDB * 4 >= 2**32
    _check_case(case, big_b)
