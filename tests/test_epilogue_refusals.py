"""The host-side refusals of the SpMM epilogue's nine ABI arguments (bias,
epilogue, drop_mask, ldm, drop_scale, keep_prob, seed, offset, rng_base), which
gcnk_spmm_csr_f32, gcnk_spmm_proj_f32, gcnk_hubfactor_gc1_f32 and
gcnk_dense_gc1_f32 all turn into one Epi through make_epi (csrc/gcnk_common.h).

Each entry point is called through ctypes with otherwise valid tiny operands
(ops.py would refuse some of these calls itself, or allocate the outputs):
  SpMM        a 32-row ring graph, M = K = 32, F = 8
  projection  the same graph at the smallest F and P it takes: F = 4 (one
              16-B piece per row), P = 1, whole-wave groups
  hubfactor   the smallest case of tests/hubfactor_cases.py (Kc = 1, F = 4, P = 1, 7 hubs)
  dense gc1   M = 32, K = 4, F = 8, P = 4
A bad epilogue -- code -1 or 5, GCNK_EPI_BIAS_RELU_DROP with a null mask or with
ldm = F - 1, and for the dense gc1 GCNK_EPI_NONE, which is no gc1 epilogue --
returns GCNK_EARG with the entry point's own name in gcnk_last_error(), before
any launch: the outputs keep the bit pattern they were filled with.  And a hash
epilogue's ldm = 0 means ldm = F: the two calls give the same bits.
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
from graph_convolutional_networks_for_text_classification_amd import _lib, ops  # noqa: E402
from graph_convolutional_networks_for_text_classification_amd.sparse import CSR  # noqa: E402

DEV = "cuda"
SENTINEL = 0x7FC5A5A5            # a NaN's bits: any store of a computed value changes them
N = 32                           # rows of the ring graph and of the dense gc1's A-hat X
HUB = hc.CASES[0]                # Kc = 1, F = 4, P = 1, 7 hubs, ldu = 4
assert (HUB.Kc, HUB.F, HUB.P) == (1, 4, 1)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == SENTINEL).all())


def _randn(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


def _ring():
    """A-hat-like ring: row i holds columns i - 1, i, i + 1 (mod 32), sorted."""
    cols = np.sort(np.stack([(np.arange(N) + d) % N for d in (-1, 0, 1)], 1), 1).astype(np.int32)
    vals = np.random.default_rng(3).uniform(0.1, 1.0, cols.shape).astype(np.float32)
    return CSR(torch.arange(0, 3 * N + 1, 3, dtype=torch.int32, device=DEV), torch.from_numpy(cols.ravel()).to(DEV),
               torch.from_numpy(vals.ravel()).to(DEV), (N, N))


class Entry:
    """One entry point on fixed valid operands: call(epi) with epi = (epilogue,
    mask, ldm, drop_scale, keep_prob, seed, offset, rng_base) launches into
    freshly sentinel-filled outputs and returns (rc, outputs)."""

    def __init__(self, name, F, outputs, launch):
        self.name, self.F, self._outputs, self._launch = name, F, outputs, launch

    def call(self, epi):
        outs = [_filled(*s) for s in self._outputs]
        rc = self._launch(_lib.load(), outs, epi)
        torch.cuda.synchronize()
        return rc, outs


def _spmm_entry():
    F = 8
    a, B, bias = _ring(), _randn(1, N, F), _randn(2, F)
    plan = ops.plan_for(a, F)
    wsb = plan.workspace_bytes(F)
    ws, cnt = ops.workspace(wsb, B.device), plan.counters(B.device)

    def launch(lib, outs, epi):
        return lib.gcnk_spmm_csr_f32(_p(plan.buf), ctypes.cast(plan.hdr, ctypes.c_void_p), _p(B), F, F, _p(outs[0]), F,
                                     _p(bias), *epi, _p(ws), wsb, _p(cnt), 4 * cnt.numel() if cnt is not None else 0,
                                     0, _stream())
    return Entry("gcnk_spmm_csr_f32", F, [(N, F)], launch)


def _proj_entry():
    F, P, lanes = 4, 1, 64
    a, B, bias, W = _ring(), _randn(4, N, F), _randn(5, F), _randn(6, F, P)
    plan = ops.plan_for(a, F, lanes, dense=2.0)      # (no dense blocks: the projection takes row-kernel rows only)
    wsb = plan.workspace_bytes(F)
    ws, cnt = ops.workspace(wsb, B.device), plan.counters(B.device)

    def launch(lib, outs, epi):
        return lib.gcnk_spmm_proj_f32(_p(plan.buf), ctypes.cast(plan.hdr, ctypes.c_void_p), _p(B), F, F, _p(outs[0]), F,
                                      _p(bias), *epi, _p(W), P, P, _p(outs[1]), P, _p(ws), wsb, _p(cnt),
                                      4 * cnt.numel() if cnt is not None else 0, lanes, _stream())
    return Entry("gcnk_spmm_proj_f32", F, [(N, F), (N, P)], launch)


def _hubfactor_entry():
    c = HUB
    o = hc.operands(c.nhub, c.Kc, c.F, c.P, c.ldu)
    d = {k: torch.from_numpy(o[k]).to(DEV) for k in ("rec", "U", "W1", "S", "b1", "W2")}

    def launch(lib, outs, epi):
        return lib.gcnk_hubfactor_gc1_f32(hc.M, c.F, c.Kc, c.nhub, c.P, _p(d["U"]), c.ldu, _p(d["W1"]), c.F, hc.K0,
                                          _p(d["S"]), c.F, _p(d["rec"]), o["rec_words"], _p(d["b1"]), *epi,
                                          _p(d["W2"]), c.P, _p(outs[0]), c.F, _p(outs[1]), c.P, _stream())
    return Entry("gcnk_hubfactor_gc1_f32", c.F, [(hc.M, c.F), (hc.M, c.P)], launch)


def _dense_entry():
    K, F, P = 4, 8, 4
    AX, W1, b1, W2 = _randn(7, N, K), _randn(8, K, F), _randn(9, F), _randn(10, F, P)

    def launch(lib, outs, epi):
        return lib.gcnk_dense_gc1_f32(N, K, F, P, _p(AX), K, _p(W1), F, _p(b1), *epi, _p(W2), P, _p(outs[0]), F,
                                      _p(outs[1]), P, _stream())
    return Entry("gcnk_dense_gc1_f32", F, [(N, F), (N, P)], launch)


ENTRIES = {"spmm": _spmm_entry, "proj": _proj_entry, "hubfactor": _hubfactor_entry, "dense": _dense_entry}


def bad_epilogues(entry, kind):
    """[(label, epi)]: the calls that must be refused"""
    F = entry.F
    mask = torch.ones((hc.M if kind == "hubfactor" else N, F), dtype=torch.uint8, device=DEV)
    plain = (None, 0, 1.0, 1.0, 0, 0, None)
    bad = [("code -1", (-1, *plain)), ("code 5", (5, *plain)),
           ("drop, null mask", (_lib.EPI_BIAS_RELU_DROP, None, F, 2.0, 0.5, 0, 0, None)),
           ("drop, ldm = F - 1", (_lib.EPI_BIAS_RELU_DROP, _p(mask), F - 1, 2.0, 0.5, 0, 0, None))]
    if kind == "dense":
        bad.append(("code NONE", (_lib.EPI_NONE, *plain)))
    return bad, mask


def probe(kind):
    """[(label, rc, gcnk_last_error(), outputs untouched)] of an entry point's bad calls"""
    entry = ENTRIES[kind]()
    bad, _mask = bad_epilogues(entry, kind)
    rows = []
    for label, epi in bad:
        rc, outs = entry.call(epi)
        rows.append((label, rc, _lib.load().gcnk_last_error().decode(errors="replace"), all(map(_untouched, outs))))
    return entry, rows


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(ENTRIES))
def test_bad_epilogue_is_refused_on_the_host(kind):
    entry, rows = probe(kind)
    assert len(rows) == (5 if kind == "dense" else 4)
    for label, rc, msg, untouched in rows:
        print(f"{entry.name}: {label}: rc={rc} {msg!r} untouched={untouched}")
        assert rc == _lib.EARG, (label, rc, msg)
        with pytest.raises(_lib.GcnkError, match=r"rc=-1"):
            _lib.check(rc, entry.name)
        assert entry.name in msg, (label, msg)
        assert untouched, label


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(ENTRIES))
def test_hash_epilogue_ldm_zero_means_F(kind):
    entry = ENTRIES[kind]()
    results = []
    for ldm in (0, entry.F):
        rc, outs = entry.call((_lib.EPI_BIAS_RELU_HASH, None, ldm, 2.0, 0.5, 0x1234567 << 8, 77, None))
        _lib.check(rc, entry.name)
        assert not any(map(_untouched, outs))
        results.append(outs)
    for x, y in zip(*results):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    h = results[0][0]                                    # the dropout drew both kinds of element
    assert bool((h == 0).any()) and bool((h > 0).any())
