"""The GCN off the main road, compared exactly: more than 32 classes (the
unfused backward: colsum, transA GEMM, transB GEMM with MASK_POS, colsum), the
fused backward against the unfused one on every forward kind, and every
subset of frozen parameters.

The inputs are chosen so that fp32 arithmetic is exact: the adjacency's values
are drawn from {+-1/4, +-1/2, +-1}, X is integer in [-2, 2], the weights are in
{-1, -1/2, 0, 1/2, 1}, the biases multiples of 1/4, dropout 0.5 (scale 2) and
the loss (out * Wt).sum() with integer Wt.  Every term of every product is then
a multiple of the product's quantum, and where the largest row-by-column sum of
absolute terms stays below 2^24 quanta (test_inputs_are_exact_in_fp32, on the
float64 reference alone, both associations (A X) W1 and A (X W1)) every partial
sum in any order is exact: logits and gradients must EQUAL the float64
reference cast to fp32, whatever kernel, association or summation order ran.
No allowance for the ReLU kink is needed (Z1 is the same number on every path)
and a single mis-indexed element shows, however small.  No product here is
inexact by design, so nothing falls back to a tolerance.

The reference is a float64 torch-autograd restatement of the reference's
layer.py:164-190 with an explicit keep mask: with dropout_rng="cpu" the module
draws torch.empty(M, F).bernoulli_(0.5) from the default generator
(tests/test_rng.py pins that), so the same torch.manual_seed gives the mask.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, _lib, datasets

DEV = "cuda"
NDOC, NTOPIC = 600, 12          # several 32- and 64-row blocks and ragged tails (612 rows)
# 3 of 12 topic columns fill a 64-row block of doc rows to the planner's dense threshold (sparse.DENSE_THRESHOLD):
# the adjacency's plan has tile blocks, which the fused projection does not take.  With 16 topics it has none.
NTOPIC_NO_TILES = 16
MASK_SEED = 3
PARAMS = ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias")
Q_A, Q_X, Q_W, Q_B = 0.25, 1.0, 0.5, 0.25    # the quanta of the operands


class Problem:
    """One seeded (A, X, W1, b1, W2, b2, Wt) in float64 numpy, its keep mask, and its float64 answers."""

    def __init__(self, nfeat, x_kind, F, P, ntopic=NTOPIC, seed=0):
        rng = np.random.default_rng([seed, nfeat, F, P, ntopic])
        n = NDOC + ntopic
        av = np.array([-1.0, -0.5, -0.25, 0.25, 0.5, 1.0])
        A = np.zeros((n, n))
        for d in range(NDOC):               # doc rows: a self loop plus 3 topic columns
            A[d, d] = rng.choice(av)
            for t in rng.choice(ntopic, 3, replace=False):
                A[d, NDOC + t] = rng.choice(av)
                A[NDOC + t, d] = rng.choice(av)     # topic rows: their docs ...
        tt = rng.random((ntopic, ntopic)) < 0.3     # ... other topics and a self loop
        np.fill_diagonal(tt, True)
        A[NDOC:, NDOC:] = np.where(tt, rng.choice(av, (ntopic, ntopic)), 0.0)
        xv = np.array([-2.0, -1.0, 1.0, 2.0])
        X = np.zeros((n, nfeat))
        if x_kind == "dense":                # 30 % full everywhere: above ops.DENSE_OPERAND_FILL
            X = np.where(rng.random((n, nfeat)) < 0.3, rng.choice(xv, (n, nfeat)), 0.0)
        elif x_kind == "sparse":             # ~5 % full: doc rows inside columns [20, 120), topic rows dense
            X[:NDOC, 20:120] = np.where(rng.random((NDOC, 100)) < 0.15, rng.choice(xv, (NDOC, 100)), 0.0)
            X[NDOC:] = np.where(rng.random((ntopic, nfeat)) < 0.6, rng.choice(xv, (ntopic, nfeat)), 0.0)
        else:                                # "sparse_red", ~6 % full: the doc rows crowd 32 columns, so those 32
            # rows of X^T fill a tile block ~600 condensed columns (10 chunks) wide: X^T's plan ends in a tile
            # REDUCE launch, the one that carries the backward's side reduce ("sparse": no such launch)
            X[:NDOC, 20:52] = np.where(rng.random((NDOC, 32)) < 0.45, rng.choice(xv, (NDOC, 32)), 0.0)
            X[NDOC:] = np.where(rng.random((ntopic, nfeat)) < 0.6, rng.choice(xv, (ntopic, nfeat)), 0.0)
        wv = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
        self.A, self.X = A, X
        self.W1, self.W2 = rng.choice(wv, (nfeat, F)), rng.choice(wv, (F, P))
        self.b1, self.b2 = rng.integers(-4, 5, F) / 4.0, rng.integers(-4, 5, P) / 4.0
        self.Wt = rng.integers(-2, 3, (n, P)).astype(np.float64)
        self.nfeat, self.F, self.P, self.n = nfeat, F, P, n
        torch.manual_seed(MASK_SEED)
        self.keep = torch.empty(n, F).bernoulli_(0.5).double().numpy()
        self._dev = None

    def reference(self, train):
        """(logits, {parameter: gradient}) in float64 (torch autograd on the restated forward)."""
        t = {k: torch.from_numpy(getattr(self, k)) for k in ("A", "X", "W1", "b1", "W2", "b2", "Wt")}
        for k in ("W1", "b1", "W2", "b2"):
            t[k].requires_grad_(True)
        H1 = torch.relu(t["A"] @ (t["X"] @ t["W1"]) + t["b1"])          # layer.py:102,106,110,182
        if train:
            H1 = H1 * torch.from_numpy(self.keep) * 2.0                  # layer.py:185, p = 0.5
        out = t["A"] @ (H1 @ t["W2"]) + t["b2"]                          # gc2
        (out * t["Wt"]).sum().backward()
        grads = dict(zip(PARAMS, (t[k].grad.numpy() for k in ("W1", "b1", "W2", "b2"))))
        return out.detach().numpy(), grads

    def exactness_ratio(self, train):
        """max over every product of forward and backward, both associations of
        gc1, of (largest row-by-column sum of absolute terms) / quantum."""
        A, X, W1, b1, W2, b2, G = self.A, self.X, self.W1, self.b1, self.W2, self.b2, self.Wt
        worst = {}

        def prod(name, L, R, q, add=None):
            s = np.abs(L) @ np.abs(R)
            if add is not None:
                s = s + np.abs(add)
            worst[name] = s.max() / q
            return L @ R + (0.0 if add is None else add)

        S1 = prod("X W1", X, W1, Q_X * Q_W)
        Z1 = prod("A (X W1) + b1", A, S1, Q_A * Q_X * Q_W, b1[None, :])
        AX = prod("A X", A, X, Q_A * Q_X)
        Z1b = prod("(A X) W1 + b1", AX, W1, Q_A * Q_X * Q_W, b1[None, :])
        assert np.array_equal(Z1, Z1b)
        q_h = Q_A * Q_X * Q_W                     # relu(Z1); times 2 in train mode is a multiple of it too
        H1 = np.maximum(Z1, 0.0) * (self.keep * 2.0 if train else 1.0)
        S2 = prod("H1 W2", H1, W2, q_h * Q_W)
        prod("A S2 + b2", A, S2, Q_A * q_h * Q_W, b2[None, :])
        gS2 = prod("A^T G", A.T, G, Q_A)
        T = prod("gS2 W2^T", gS2, W2.T, Q_A * Q_W)
        gZ1 = np.where(H1 > 0, 2.0 * T if train else T, 0.0)
        q_z = Q_A * Q_W
        prod("H1^T gS2", H1.T, gS2, q_h * Q_A)
        ones = np.ones((1, self.n))
        prod("colsum G", ones, G, 1.0)
        prod("colsum gZ1", ones, gZ1, q_z)
        gS1 = prod("A^T gZ1", A.T, gZ1, Q_A * q_z)
        prod("X^T gS1", X.T, gS1, Q_X * Q_A * q_z)
        prod("(A X)^T gZ1", AX.T, gZ1, Q_A * Q_X * q_z)
        return worst

    def on_device(self):
        """(X, A) as the module takes them: torch sparse COO on the GPU (made once)."""
        if self._dev is None:
            self._dev = (datasets.dense_to_coo(self.X.astype(np.float32)).to(DEV),
                         datasets.dense_to_coo(self.A.astype(np.float32)).to(DEV))
        return self._dev

    def model(self, dropout_rng="cpu", trainable=PARAMS):
        m = GCN(nfeat=self.nfeat, nhid=self.F, nclass=self.P, dropout=0.5, dropout_rng=dropout_rng)
        with torch.no_grad():
            for name, v in zip(PARAMS, (self.W1, self.b1, self.W2, self.b2)):
                m.get_parameter(name).copy_(torch.from_numpy(v))
        for name in PARAMS:
            m.get_parameter(name).requires_grad_(name in trainable)
        return m.to(DEV)

    def train_step(self, m):
        """(train-mode logits, {parameter: gradient or None}) of one step on the seeded mask."""
        X, A = self.on_device()
        m.train()
        m.zero_grad(set_to_none=True)
        torch.manual_seed(MASK_SEED)
        out = m(X, A)
        (out * torch.from_numpy(self.Wt).float().to(DEV)).sum().backward()
        return out.detach().cpu().numpy(), {k: (p.grad.cpu().numpy() if p.grad is not None else None)
                                            for k, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def problem(x_kind, F, P, ntopic=NTOPIC):
    assert x_kind in ("dense", "sparse", "sparse_red")
    return Problem(100 if x_kind == "dense" else 300, x_kind, F, P, ntopic)


@functools.lru_cache(maxsize=None)
def reference(x_kind, F, P, train, ntopic=NTOPIC):
    return problem(x_kind, F, P, ntopic).reference(train)


def _equal(got, ref64, what):
    want = ref64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref64), f"{what}: the reference is not an fp32 number"
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
                           f"{tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r}, want {want[bad][0]!r}")


SHAPES = [(x, F, P, NTOPIC) for x in ("dense", "sparse") for F in (200, 50) for P in (33, 52)] + \
         [(x, 200, P, NTOPIC) for x in ("dense", "sparse") for P in (8, 20)] + \
         [("sparse_red", 200, P, NTOPIC) for P in (8, 20)] + \
         [("sparse_red", 200, P, NTOPIC_NO_TILES) for P in (8, 20)]


def _host_plan(A, F, lanes):
    """Header of the plan ops.plan_for(A, F, lanes) builds for the matrix A (the same planner, run on the host)."""
    import ctypes

    from graph_convolutional_networks_for_text_classification_amd.sparse import DENSE_THRESHOLD, PlanHeader
    lib = _lib.load()
    M, K = A.shape
    rows, cols = np.nonzero(A)
    rp = np.zeros(M + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=M))
    ci, v = cols.astype(np.int32), A[rows, cols].astype(np.float32)
    ipc, groups = lib.gcnk_spmm_default_ipc(M, len(ci), F, lanes), lib.gcnk_spmm_groups(F, lanes)
    nbytes = lib.gcnk_spmm_plan_bytes_host(rp.ctypes.data, ci.ctypes.data, M, K, len(ci), ipc, groups, DENSE_THRESHOLD)
    assert nbytes > 0, lib.gcnk_last_error()
    buf = np.zeros(nbytes // 4, np.int32)
    assert lib.gcnk_spmm_plan_build_host(rp.ctypes.data, ci.ctypes.data, v.ctypes.data, M, K, len(ci), ipc, groups,
                                         ctypes.c_float(DENSE_THRESHOLD), buf.ctypes.data, nbytes) == 0
    return PlanHeader(buf)


@pytest.mark.parametrize("x_kind,F,P,ntopic", SHAPES)
def test_inputs_are_exact_in_fp32(x_kind, F, P, ntopic):
    """The precondition, on the float64 reference alone (no GPU): every product's
    absolute row-by-column sums stay below 2^24 quanta, in eval and train mode."""
    pb = problem(x_kind, F, P, ntopic)
    # the adjacency's lanes-64 plan (the fused projection's): tile chunks with 12 topics, none with 16
    assert (_host_plan(pb.A, F, 64).ntile == 0) == (ntopic == NTOPIC_NO_TILES)
    if x_kind != "dense":
        # X^T's plan (record.BackwardRecord: ops.plan_for(xT, F)): a tile reduce launch -- the one the side
        # reduce of gcn_bwd2 is carried into (csrc/spmm.hip, spmm_csr_f32_side) -- for "sparse_red" only
        xt = _host_plan(np.ascontiguousarray(pb.X.T), F, 0)
        print(f"{x_kind} topics={ntopic}: X^T plan ntile={xt.ntile} nred={xt.nred}")
        assert (xt.nred > 0) == (x_kind == "sparse_red")
    assert (pb.X != 0).mean() >= (0.25 if x_kind == "dense" else 0.03)
    assert (pb.X != 0).mean() <= (1.0 if x_kind == "dense" else 0.19)     # below ops.DENSE_OPERAND_FILL
    for train in (False, True):
        worst = pb.exactness_ratio(train)
        name = max(worst, key=worst.get)
        print(f"{x_kind} F={F} P={P} topics={ntopic} train={train}: max ratio / 2^24 = {worst[name] / 2**24:.4f} ({name})")
        assert worst[name] < 2**24, (name, worst[name])


def _records(A):
    from graph_convolutional_networks_for_text_classification_amd.sparse import as_csr
    return [r.rec for r in getattr(as_csr(A), "_records", {}).values()]


def _forget_records(A):
    from graph_convolutional_networks_for_text_classification_amd.sparse import as_csr
    as_csr(A).__dict__.pop("_records", None)


# ------------------------------------------------------------------------------ a. more than 32 classes

@pytest.mark.gpu
@pytest.mark.parametrize("P", [33, 52])
@pytest.mark.parametrize("F", [200, 50])
@pytest.mark.parametrize("x_kind", ["dense", "sparse"])
def test_more_than_32_classes_train_exactly(x_kind, F, P):
    """A GCN with 33 and 52 classes (R52 has 52): the forward is SpMM + GEMM,
    the backward the per-op unfused branch (no BackwardRecord for P > 32).
    Eval logits, train-mode logits and all four gradients equal float64."""
    from graph_convolutional_networks_for_text_classification_amd import record
    pb = problem(x_kind, F, P)
    X, A = pb.on_device()
    _forget_records(A)
    m = pb.model()
    m.eval()
    with torch.no_grad():
        ev = m(X, A).cpu().numpy()
    _equal(ev, reference(x_kind, F, P, False)[0], "eval logits")
    out, grads = pb.train_step(m)
    ref_out, ref_grads = reference(x_kind, F, P, True)
    _equal(out, ref_out, "train logits")
    for k in PARAMS:
        _equal(grads[k], ref_grads[k], k)
    recs = _records(A)
    fwd = [r for r in recs if isinstance(r, record.ForwardRecord)]
    assert fwd and all(r.kind == record.SPMM_GEMM for r in fwd)
    assert not any(isinstance(r, record.BackwardRecord) for r in recs)


# ------------------------------------------------------------------------------ b. fused against unfused backward

@pytest.mark.gpu
@pytest.mark.parametrize("P", [8, 20])
@pytest.mark.parametrize("path", ["factored", "spmm_proj", "spmm_gemm", "dense_ax"])
def test_fused_and_unfused_backward_agree_exactly(path, P, monkeypatch):
    """ops.FUSE_BACKWARD on (gcn_bwd2 through the backward record) and off
    (colsum + the two GEMMs), on each forward kind the record test forces:
    gradients equal float64 either way; with device dropout (the same forward
    bits both ways) they equal each other.  The factored and fused-projection
    paths run on the X whose X^T plan carries the side reduce, SpMM + GEMM on
    the one where it is a launch of its own; the fused projection with
    ops.FUSE_MAX_P = 32, so P = 20 takes its 32-channel kernel."""
    from graph_convolutional_networks_for_text_classification_amd import ops, record
    monkeypatch.setattr(ops, "FACTOR_GC1", path == "factored")
    monkeypatch.setattr(ops, "FUSE_PROJECTION", path != "spmm_gemm")
    monkeypatch.setattr(ops, "DENSE_AX", path == "dense_ax")
    monkeypatch.setattr(ops, "FUSE_MAX_P", 32)
    x_kind = {"dense_ax": "dense", "spmm_gemm": "sparse"}.get(path, "sparse_red")
    ntopic = NTOPIC_NO_TILES if path == "spmm_proj" else NTOPIC
    pb = problem(x_kind, 200, P, ntopic)
    X, A = pb.on_device()
    ref_out, ref_grads = reference(x_kind, 200, P, True, ntopic)
    hashed = {}
    for fuse in (True, False):
        monkeypatch.setattr(ops, "FUSE_BACKWARD", fuse)
        _forget_records(A)
        out, grads = pb.train_step(pb.model())
        _equal(out, ref_out, f"train logits (fuse={fuse})")
        for k in PARAMS:
            _equal(grads[k], ref_grads[k], f"{k} (fuse={fuse})")
        recs = _records(A)
        assert fuse == any(isinstance(r, record.BackwardRecord) for r in recs)
        kinds = {r.kind for r in recs if isinstance(r, record.ForwardRecord)}
        want = {"factored": record.FACTORED, "spmm_gemm": record.SPMM_GEMM, "dense_ax": record.DENSE_AX,
                "spmm_proj": record.SPMM_PROJ}[path]   # (on an adjacency without dense tile blocks)
        assert kinds == {want}, kinds
        hashed[fuse] = pb.train_step(pb.model(dropout_rng="device"))
    assert np.array_equal(hashed[True][0], hashed[False][0])
    assert not np.array_equal(hashed[True][0], ref_out)          # (another mask than the seeded CPU one)
    for k in PARAMS:
        assert np.array_equal(hashed[True][1][k], hashed[False][1][k]), k


# ------------------------------------------------------------------------------ c. frozen parameters

SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(PARAMS, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("trainable", SUBSETS, ids=lambda s: "+".join(s))
@pytest.mark.parametrize("setting", ["sparse_red-8", "sparse-8", "dense-8", "sparse-52"])
def test_frozen_parameters(setting, trainable, monkeypatch):
    """Every non-empty subset of the four parameters left trainable: P = 8 with
    sparse X, twice (backward record, gW1 through X^T's plan: "sparse_red",
    whose plan ends in a tile reduce launch that carries gcn_bwd2's side
    reduce whenever gW1 is wanted, and "sparse", where the side reduce is
    always a launch of its own; test_inputs_are_exact_in_fp32 pins both plans),
    P = 8 with dense X (the dense-AX record, gW1 = (A-hat X)^T gZ1) and P = 52
    (per-op).  Trainable gradients equal float64, frozen ones stay
    None; with nothing trainable in gc1 no BackwardRecord is built and gZ1 is
    never computed (neither gcn_bwd2 nor a MASK_POS GEMM runs)."""
    from graph_convolutional_networks_for_text_classification_amd import ops, record
    x_kind, P = setting.split("-")
    P = int(P)
    pb = problem(x_kind, 200, P)
    X, A = pb.on_device()
    _forget_records(A)
    calls = {"bwd2": 0, "mask_pos": 0}
    real_gemm, real_bwd2 = ops.gemm, ops.gcn_bwd2

    def gemm(*a, **kw):
        calls["mask_pos"] += kw.get("epilogue") == _lib.GEMM_EPI_MASK_POS
        return real_gemm(*a, **kw)

    def gcn_bwd2(*a, **kw):
        calls["bwd2"] += 1
        return real_bwd2(*a, **kw)

    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "gcn_bwd2", gcn_bwd2)
    out, grads = pb.train_step(pb.model(trainable=trainable))
    ref_out, ref_grads = reference(x_kind, 200, P, True)
    _equal(out, ref_out, "train logits")
    for k in PARAMS:
        if k in trainable:
            _equal(grads[k], ref_grads[k], k)
        else:
            assert grads[k] is None, k
    recs = _records(A)
    kinds = {r.kind for r in recs if isinstance(r, record.ForwardRecord)}
    assert kinds == {{"dense-8": record.DENSE_AX, "sparse-52": record.SPMM_GEMM}.get(setting, record.FACTORED)}, kinds
    gc1 = any(k.startswith("gc1.") for k in trainable)
    built = any(isinstance(r, record.BackwardRecord) for r in recs)
    assert built == (gc1 and P <= 32)
    if not gc1:
        assert calls == {"bwd2": 0, "mask_pos": 0}
    elif P > 32:
        assert calls["mask_pos"] == 1
