"""CPU checks of the native loss and optimiser: the float64 restatements the GPU
tests compare against (tests/train_ref.py) agree with torch in float64, and
every new entry point validates its arguments before any launch (no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, train

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ref  # noqa: E402


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


@pytest.mark.parametrize("idx", [None, [3, 0, 7, 11, 20, 36], [5, 2, 5, 5, 9, 5, 5, 2], [36]])
def test_loss_restatement_matches_torch_float64(idx):
    rng = np.random.default_rng(3)
    M, P = 37, 9
    z = rng.normal(0, 5, (M, P))
    t = rng.integers(0, P, M)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t)
    if idx is None:
        want = torch.nn.functional.cross_entropy(zt, tt)
        counts, n = None, None
    else:
        it = torch.tensor(idx)
        want = torch.nn.functional.cross_entropy(zt[it], tt[it])
        counts, n = train_ref.counts_of(idx, M), len(idx)
        assert counts[M] == 0 and counts[:M].sum() == n
    (want * 0.75).backward()
    lse, row, loss = train_ref.ce_forward(z, t, counts, n)
    assert _rel(loss, want.item()) <= 1e-12
    assert _rel(lse, torch.logsumexp(zt.detach(), 1).numpy()) <= 1e-12
    assert _rel(train_ref.ce_backward(z, t, counts, n, g=0.75), zt.grad.numpy()) <= 1e-12


def test_counts_restatement_out_of_range():
    c = train_ref.counts_of([0, 4, 4, -1, 5, 9], 5)
    assert c.tolist() == [1, 0, 0, 0, 2, 3]


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_restatement_matches_torch_float64(wd):
    rng = np.random.default_rng(5)
    p0 = rng.normal(0, 1, 301)
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=0.02, weight_decay=wd)
    q, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in range(1, 6):
        g = rng.normal(0, 1, 301)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        q, m, v = train_ref.adam_step(q, g, m, v, t, lr=0.02, weight_decay=wd)
        st = opt.state[p]
        assert _rel(q, p.detach().numpy()) <= 1e-12
        assert _rel(m, st["exp_avg"].numpy()) <= 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) <= 1e-12


# ------------------------------------------------------------------------------ argument validation, no GPU

P16 = ctypes.c_void_p(16)


def test_loss_entry_points_validate_arguments():
    lib = _lib.load()
    fwd = lambda **k: lib.gcnk_ce_forward_f32(*[k.get(a, d) for a, d in (   # noqa: E731
        ("logits", P16), ("ld", 8), ("M", 10), ("P", 8), ("target", P16), ("counts", None), ("n", 10),
        ("loss", P16), ("lse", None), ("ws", P16), ("ws_bytes", 1 << 20), ("stream", None))])
    bwd = lambda **k: lib.gcnk_ce_backward_f32(*[k.get(a, d) for a, d in (   # noqa: E731
        ("logits", P16), ("ld", 8), ("M", 10), ("P", 8), ("target", P16), ("counts", None), ("n", 10),
        ("lse", P16), ("grad_out", None), ("dlogits", P16), ("ldd", 8), ("stream", None))])
    for f in (fwd, bwd):
        assert f(P=0) == _lib.EARG and f(P=1025) == _lib.EARG
        assert f(ld=7) == _lib.EARG and b"ld" in lib.gcnk_last_error()
        assert f(logits=None) == _lib.EARG and f(target=None) == _lib.EARG
        assert f(M=-1) == _lib.EARG and f(n=-1) == _lib.EARG
        assert f(M=0) == _lib.OK and f(M=0, logits=None, target=None) == _lib.OK
    assert fwd(loss=None) == _lib.EARG
    assert bwd(lse=None) == _lib.EARG and bwd(dlogits=None) == _lib.EARG and bwd(ldd=7) == _lib.EARG
    # the loss workspace: one float64 per workgroup of 256 / lanes-per-row rows
    assert lib.gcnk_ce_workspace_bytes(7724, 8) == ((7724 + 127) // 128) * 8
    assert lib.gcnk_ce_workspace_bytes(257, 257) == ((257 + 3) // 4) * 8
    assert lib.gcnk_ce_workspace_bytes(1000, 1) == ((1000 + 255) // 256) * 8
    assert lib.gcnk_ce_workspace_bytes(0, 8) == 0
    assert lib.gcnk_ce_workspace_bytes(10, 0) == _lib.EARG and lib.gcnk_ce_workspace_bytes(10, 1025) == _lib.EARG
    need = lib.gcnk_ce_workspace_bytes(1000, 8)
    assert fwd(M=1000, ws_bytes=need - 8) == _lib.EARG and b"workspace" in lib.gcnk_last_error()
    assert fwd(M=1000, ws=None) == _lib.EARG
    assert fwd(M=1000, ws=ctypes.c_void_p(20)) == _lib.EARG
    # row multiplicities
    assert lib.gcnk_ce_row_counts(None, 5, 10, P16, None) == _lib.EARG
    assert lib.gcnk_ce_row_counts(P16, 5, 10, None, None) == _lib.EARG
    assert lib.gcnk_ce_row_counts(P16, -1, 10, P16, None) == _lib.EARG
    assert lib.gcnk_ce_row_counts(P16, 5, -1, P16, None) == _lib.EARG


def _table(n, **over):
    tab = (_lib.AdamTensor * max(1, n))()
    for i in range(n):
        tab[i].p, tab[i].g, tab[i].m, tab[i].v, tab[i].numel = 16, 16, 16, 16, 100
    for k, val in over.items():
        setattr(tab[0], k, val)
    return tab


def test_adam_entry_point_validates_arguments():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.AdamTensor) == 40 and _lib.ADAM_MAX_TENSORS == 8

    def call(tab, n, lr=0.02, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, state=P16, flags=0):
        return lib.gcnk_adam_f32(tab, n, lr, b1, b2, eps, wd, state, flags, None)

    assert call(_table(9), 9) == _lib.EARG and b"ntensors" in lib.gcnk_last_error()
    assert call(_table(1), -1) == _lib.EARG
    assert call(_table(1), 1, b1=1.0) == _lib.EARG and call(_table(1), 1, b2=1.0) == _lib.EARG
    assert call(_table(1), 1, b1=-0.1) == _lib.EARG and call(_table(1), 1, b2=float("nan")) == _lib.EARG
    assert call(_table(1), 1, eps=-1e-8) == _lib.EARG and call(_table(1), 1, lr=-1.0) == _lib.EARG
    assert call(_table(1), 1, wd=-0.01) == _lib.EARG
    assert call(_table(1), 1, state=None) == _lib.EARG
    assert call(None, 1) == _lib.EARG
    assert call(_table(1), 1, flags=64) == _lib.EARG
    for field in ("p", "g", "m", "v"):
        assert call(_table(2, **{field: None}), 2) == _lib.EARG and b"tensor 0" in lib.gcnk_last_error()
    assert call(_table(1, numel=-1), 1) == _lib.EARG
    # nothing to do: succeeds without a table, a state or a device
    assert call(None, 0, state=None) == _lib.OK
    assert call(_table(1), 0) == _lib.OK


def test_python_layer_refuses_what_it_does_not_implement():
    w = torch.nn.Parameter(torch.zeros(4))
    for kw in ({"amsgrad": True}, {"maximize": True}, {"foreach": True}, {"fused": True}):
        with pytest.raises(ValueError):
            train.Adam([w], **kw)
    with pytest.raises(ValueError):
        train.Adam([w], betas=(0.9, 1.0))
    opt = train.Adam([w], lr=0.02, zero_grad_in_step=True)
    assert opt.defaults == {"lr": 0.02, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0}
    w.grad = torch.zeros(4)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        opt.step()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        train.cross_entropy(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64), torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        train.IndexedCrossEntropy()(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64))
    from graph_convolutional_networks_for_text_classification_amd import metrics
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        metrics.evaluate_with_loss(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64), None, 3)
