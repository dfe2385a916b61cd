"""Held-graph scoring: classify documents that are NOT in the training graph
(csrc/score_docs.hip, gcnk_score_docs_f32).

A trained GCN labels the nodes of the graph it ran on (reference
layer.py:164-190).  On the reference's doc-topic graph (trainer.py:98-148,
build_graph.py:99-133) a document row of A-hat holds its diagonal and topic
(hub) columns only and a document row of X the topic-weight columns
k0 .. k0 + Kc only -- the structure factor.py checks -- so the row a NEW
document would have in that forward depends on its own Kc feature values, its
own H edge weights, the parameters and two small matrices of the training
graph, S_T = X[hubs] W1 and the hub rows of S2 = H1 W2.  With the hub nodes'
state (their degrees, S_T, S2[hubs]) held as the training graph left it, a
batch of documents is ONE launch: no node appended, nothing rebuilt, no
host synchronisation.

    scorer = DocumentScorer(model, features, adj)
    logits = scorer(x, a)            # [B x P]
    labels = scorer.predict(x, a)    # int64 [B]

``x`` [B x Kc]: the feature values on columns k0 .. k0 + Kc; ``a`` [B x H]:
the raw edge weight to each hub, in ``scorer.hubs`` order (ascending node id:
the reference's topic order), 0 for no edge.  Negative or non-finite weights
are the caller's error: nothing checks them, on the host or on the device.
For a document that IS in the graph, x = its X row and
a = A-hat[d, hub_j] / (sqrt(A-hat[d, d]) dh_j) give exactly its row of
``model(features, adj)`` in eval mode.
"""
import numpy as np
import torch

from . import _lib, factor, ops
from .derived import Cache
from .ops import Epilogue, Operand, _ptr
from .sparse import as_csr, require_device

_EVAL = Epilogue(_lib.EPI_BIAS_RELU)


class _Held:
    """What a launch reads besides (x, a): built once per (parameters, A-hat, X)."""

    __slots__ = ("fac", "dh", "W1", "b1", "W2", "b2", "S_T", "S2_T", "F", "P", "pinned")


def _hub_dh(adj, fac):
    """dh[j] = sqrt(float64(A-hat[hub_j, hub_j])): the hub's D^-1/2, because
    (A + I)_tt = 1 on the reference's graphs (no topic self-edges,
    build_graph.py:116-133).  float64 [H] on adj's device."""
    rp, ci, v = (t.cpu().numpy() for t in (adj.rowptr, adj.colind, adj.val))
    dh = np.empty(fac.H, np.float64)
    for j, h in enumerate(fac.hubs.tolist()):
        s, e = int(rp[h]), int(rp[h + 1])
        at = np.flatnonzero(ci[s:e] == h)
        if at.size != 1 or not v[s + at[0]] > 0:
            raise ValueError(f"DocumentScorer: hub node {h} has no positive diagonal entry in A-hat "
                             "(not a normalised adjacency)")
        dh[j] = np.sqrt(np.float64(v[s + at[0]]))
    return torch.from_numpy(dh).to(adj.device)


def _rows16(t, what, width):
    """``t`` [B x width] fp32 on the device with 16-byte aligned rows (the kernel's
    operand form); anything else is copied once into padded rows."""
    require_device(t, what)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width:
        raise RuntimeError(f"{what} must be float32 [B x {width}], got {t.dtype} {tuple(t.shape)}")
    if t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= width and t.data_ptr() % 16 == 0:
        return t
    buf = torch.empty((t.shape[0], (width + 3) // 4 * 4), dtype=torch.float32, device=t.device)[:, :width]
    buf.copy_(t)
    return buf


class DocumentScorer:
    """Scores unseen documents against ``model`` trained on (``features``, ``adj``).

    The held state is built here with one eval forward under ``no_grad`` and is
    valid while derived.stamp() of the four parameters, of ``adj`` and of
    ``features`` is unchanged (derived.py's one rule); the next call after an
    in-place change rebuilds it, so a scorer made before ``fit`` scores with the
    fitted model afterwards.  ValueError when the graph is not doc-topic
    structured (factor.get is None); RuntimeError on CPU tensors."""

    def __init__(self, model, features, adj):
        for what, t in (("features", features), ("adj", adj), ("gc1.weight", model.gc1.weight)):
            require_device(t if isinstance(t, torch.Tensor) else t.val, what)
        self.model, self.features, self.adj = model, features, adj
        self._cache = Cache(1)
        self._state()

    def _sources(self):
        m = self.model
        return tuple(p for p in (m.gc1.weight, m.gc1.bias, m.gc2.weight, m.gc2.bias) if p is not None) + \
            (self.adj, self.features)

    def _state(self):
        h = self._cache.get("held", self._sources(), self._build)
        if torch.cuda.is_current_stream_capturing():
            h.pinned = True   # (a captured launch keeps reading these buffers: derived.py)
        return h

    def _build(self):
        m = self.model
        adj, xop = as_csr(self.adj), Operand(self.features)
        fac = factor.get(adj, xop)
        if fac is None:
            raise ValueError("DocumentScorer: the graph is not doc-topic structured (hub rows, and document rows "
                             "holding only hub columns and their diagonal, with X's document rows on one column "
                             "range): factor.get found no hub factorisation")
        h = _Held()
        h.fac, h.pinned = fac, False
        h.dh = _hub_dh(adj, fac)
        with torch.no_grad():
            W1, W2 = m.gc1.weight.detach(), m.gc2.weight.detach()
            b1 = m.gc1.bias.detach() if m.gc1.bias is not None else None
            b2 = m.gc2.bias.detach() if m.gc2.bias is not None else None
            # (views of the parameters where they are contiguous: rows of F floats, F % 4 == 0, are 16-B aligned)
            h.W1, h.W2 = W1.contiguous(), W2.contiguous()
            h.b1, h.b2 = (b if b is None else b.contiguous() for b in (b1, b2))
            h.F, h.P = W1.shape[1], W2.shape[1]
            h.S_T = fac.hub_times(h.W1).contiguous()                       # X[hubs] W1   (layer.py:102)
            # S2 = H1 W2 of the eval forward on the training graph, from that forward's own launches
            S2 = ops._gc1_per_op(adj, xop, h.W1, h.b1, h.W2, _EVAL, False)[1]
            h.S2_T = S2.index_select(0, fac.hubs.to(S2.device)).contiguous()
        return h

    @property
    def hubs(self):
        """The hub (topic) node ids, ascending: the column order of ``a``."""
        return self._state().fac.hubs

    @property
    def k0(self):
        return self._state().fac.k0

    @property
    def Kc(self):
        return self._state().fac.Kc

    def _run(self, x, a, want_labels):
        h = self._state()
        fac = h.fac
        x, a = _rows16(x, "x", fac.Kc), _rows16(a, "a", fac.H)
        B = x.shape[0]
        if a.shape[0] != B or a.device != x.device or x.device != h.W1.device:
            raise RuntimeError(f"DocumentScorer: x {tuple(x.shape)} on {x.device}, a {tuple(a.shape)} on {a.device}, "
                               f"model on {h.W1.device}")
        out = torch.empty((B, h.P), dtype=torch.float32, device=x.device)
        labels = torch.empty(B, dtype=torch.int32, device=x.device) if want_labels else None
        with torch.cuda.device(x.device):
            rc = _lib.load().gcnk_score_docs_f32(
                B, h.F, fac.Kc, fac.H, h.P, fac.k0, _ptr(x), x.stride(0), _ptr(a), a.stride(0), _ptr(h.W1),
                h.W1.stride(0), _ptr(h.S_T), h.S_T.stride(0), _ptr(h.W2), h.W2.stride(0), _ptr(h.S2_T),
                h.S2_T.stride(0), _ptr(h.dh), _ptr(h.b1), _ptr(h.b2), _ptr(out), out.stride(0), _ptr(labels),
                _lib.stream(x.device))
        _lib.check(rc, "gcnk_score_docs_f32")   # (no fallback: a shape the kernel refuses is an error)
        return out, labels

    def __call__(self, x, a):
        """Logits [B x P] of the B documents (x [B x Kc], a [B x H])."""
        return self._run(x, a, False)[0]

    def predict(self, x, a):
        """int64 labels [B]: first index of the maximum, a NaN maximal (metrics' rule).
        The launch writes int32 labels; widening them is one more (asynchronous) torch kernel."""
        return self._run(x, a, True)[1].to(torch.int64)


def from_theta(theta, threshold):
    """(x, a) of documents from their topic distribution ``theta`` [B x H], on
    theta's device, as the reference produces them for the graph's documents:
    x = theta / (sum theta + 1e-8) rounded to fp32, then L2-normalised per row
    (trainer.py:205-221; a zero row stays zero); a = theta where
    theta >= threshold, else 0 (build_graph.py:105-110).  The norm is taken in
    float64, so x is the correctly rounded quotient.  A convenience: the
    kernel's contract is (x, a)."""
    theta = torch.as_tensor(theta)
    if theta.dim() != 2 or not theta.is_floating_point():
        raise RuntimeError(f"theta must be a floating-point [B x H] tensor, got {theta.dtype} {tuple(theta.shape)}")
    p = (theta / (theta.sum(1, keepdim=True) + 1e-8)).to(torch.float32).to(torch.float64)
    norm = p.square().sum(1, keepdim=True).sqrt()
    x = (p / torch.where(norm == 0, torch.ones_like(norm), norm)).to(torch.float32)
    a = torch.where(theta >= threshold, theta, torch.zeros_like(theta)).to(torch.float32)
    return x, a
