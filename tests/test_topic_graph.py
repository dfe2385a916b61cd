"""build_topic_graph / topic_similarity on the GPU against the numpy restatement
(tests/topic_graph_ref.py, itself pinned to the reference's A-hat of R8 on the CPU): every
comparison of A-hat is bitwise -- rowptr, colind, and val viewed as uint32."""
import os

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import (GCN, Operand, build_topic_graph, factor,
                                                                       from_theta, sparse, topic_graph,
                                                                       topic_similarity)

import topic_graph_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = topic_graph.DOCS_PER_BLOCK
TD, TT = 0.02, 0.3

_DS = (1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7)
_KS = (1, 3, 50, 64, 65, 128)
# every D at one odd K below and one above a wave's 64 columns, every K at a D that straddles the chunk, the corners
SHAPES = sorted({(D, 3) for D in _DS} | {(D, 65) for D in _DS} | {(C + 1, K) for K in _KS} |
                {(3 * C + 7, K) for K in _KS} | {(D, K) for D in (1, 2) for K in (1, 128)})


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _arrays(g):
    a = g.adj
    return a.rowptr.cpu().numpy(), a.colind.cpu().numpy(), a.val.cpu().numpy()


def _check(g, theta, sim, td=TD, tt=TT):
    """g against the restatement of (theta, sim) as numpy arrays, bitwise; returns the restatement."""
    want = ref.build(theta, sim, td, tt)
    rp, ci, v = _arrays(g)
    D, K = theta.shape
    assert g.adj.shape == (D + K, D + K) and (g.ndoc, g.ntopic) == (D, K)
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and v.dtype == np.float32
    assert np.array_equal(rp, want[0]), "rowptr"
    assert np.array_equal(ci, want[1]), "colind"
    assert np.array_equal(v.view(np.uint32), want[2].view(np.uint32)), "val"
    assert (g.doc_topic_edges, g.topic_topic_edges) == want[3:]
    assert g.adj.nnz == D + K + 2 * (want[3] + want[4])
    return want


def _row(g, r):
    rp, ci, v = _arrays(g)
    return ci[rp[r]:rp[r + 1]].tolist(), v[rp[r]:rp[r + 1]]


@pytest.mark.parametrize("D,K", SHAPES, ids=lambda x: str(x))
def test_shape_table(D, K):
    theta, sim = ref.dirichlet_theta(D, K, seed=1000 * K + D), ref.uniform_sim(K, seed=K)
    _check(build_topic_graph(_dev(theta), topic_sim=_dev(sim), doc_topic_threshold=TD, topic_topic_threshold=TT),
           theta, sim)


def _structure_case():
    D, K = C + 1, 5
    theta = ref.dirichlet_theta(D, K, seed=7)
    theta[:, 1] = 0.0            # topic 1: no document ...
    theta[C - 1] = 0.001         # documents without a kept topic, either side of the chunk's edge
    theta[C] = 0.001
    sim = ref.uniform_sim(K, seed=3)
    sim[1, :] = sim[:, 1] = 0.0  # ... and no topic edge
    return D, K, theta, sim


def test_structure_cases():
    D, K, theta, sim = _structure_case()
    g = build_topic_graph(_dev(theta), topic_sim=_dev(sim))
    _check(g, theta, sim)
    for r in (C - 1, C, D + 1):   # isolated nodes: the diagonal alone, exactly 1.0
        cols, vals = _row(g, r)
        assert cols == [r] and vals.tolist() == [1.0]
    # a topic that keeps every document
    full = theta.copy()
    full[:, 3] = 0.5
    gf = build_topic_graph(_dev(full), topic_sim=_dev(sim))
    _check(gf, full, sim)
    assert _row(gf, D + 3)[0][:D] == list(range(D))
    # no similarities at all
    g0 = build_topic_graph(_dev(theta))
    _check(g0, theta, None)
    assert g0.topic_topic_edges == 0 and g0.features is None
    # an asymmetric sim: only i < j is read, the diagonal never
    low = sim.copy()
    low[np.tril_indices(K)] = 0.99
    g1 = build_topic_graph(_dev(theta), topic_sim=_dev(low))
    for a, b in zip(_arrays(g), _arrays(g1)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    up = sim.copy()
    up[np.triu_indices(K, 1)] = 0.0
    assert build_topic_graph(_dev(theta), topic_sim=_dev(up)).topic_topic_edges == 0


def test_threshold_semantics():
    """Each line fails a kernel that compares in fp32, rounds before it compares, or flips
    >= / >.  (A theta >= thr cannot round BELOW float32(thr), rounding being monotone; the
    case that tells a float64 comparison from one of the rounded weight is a theta just above
    0.02 whose fp32 rounding, float32(0.02) = 0.0199999995..., lies below the threshold.)"""
    D, K = 70, 4
    theta = np.full((D, K), 0.001)
    theta[:, 0] = 0.4
    theta[3, 1] = TD                          # equal: kept
    theta[4, 1] = TD - 1e-12                  # below in float64, float32(theta) == float32(0.02): dropped
    theta[5, 1] = np.nextafter(TD, 1.0)       # above in float64, float32(theta) < 0.02: kept, rounded weight
    theta[6, 2] = np.nextafter(TD, 0.0)       # one ulp below: dropped
    assert np.float32(theta[4, 1]) == np.float32(TD) and np.float64(np.float32(theta[5, 1])) < TD
    sim = np.zeros((K, K))
    sim[0, 1] = TT                            # equal: dropped (strict)
    sim[0, 2] = np.nextafter(TT, 1.0)         # one ulp above: kept
    sim[1, 2] = np.float64(np.float32(TT))    # float32(0.3) > 0.3: kept; an fp32 comparison drops it
    assert sim[1, 2] > TT
    g = build_topic_graph(_dev(theta), topic_sim=_dev(sim))
    _check(g, theta, sim)
    assert _row(g, D + 1)[0] == [3, 5, D + 1, D + 2]
    assert _row(g, D + 2)[0] == [D, D + 1, D + 2]
    assert _row(g, D)[0] == list(range(D)) + [D, D + 2]
    assert (g.doc_topic_edges, g.topic_topic_edges) == (D + 2, 2)
    # the kept weight of document 5 is the ROUNDED theta: its row equals document 3's
    assert np.array_equal(_row(g, 3)[1].view(np.uint32), _row(g, 5)[1].view(np.uint32))
    # fp32 inputs are widened exactly: the same graph as the same values handed over in float64
    t32, s32 = theta.astype(np.float32), sim.astype(np.float32)
    g32 = build_topic_graph(_dev(t32), topic_sim=_dev(s32))
    g64 = build_topic_graph(_dev(t32.astype(np.float64)), topic_sim=_dev(s32.astype(np.float64)))
    _check(g32, t32, s32)
    for a, b in zip(_arrays(g32), _arrays(g64)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert 3 not in _row(g32, D + 1)[0]       # float32(0.02) < 0.02


@pytest.fixture(scope="module")
def r8_built():
    theta, sim, D, K = ref.r8_inputs()
    return build_topic_graph(_dev(theta), topic_sim=_dev(sim), doc_topic_threshold=ref.R8_THRESHOLDS[0],
                             topic_topic_threshold=ref.R8_THRESHOLDS[1]), D, K


def test_r8_is_the_reference_a_hat(r8_built, r8):
    g, D, K = r8_built
    want = sparse.as_csr(r8["adj"].to(DEV))
    assert g.adj.shape == want.shape and (g.doc_topic_edges, g.topic_topic_edges) == (30466, 237)
    assert torch.equal(g.adj.rowptr, want.rowptr) and torch.equal(g.adj.colind, want.colind)
    assert torch.equal(g.adj.val.view(torch.int32), want.val.view(torch.int32))


def test_r8_forward_and_factor_on_the_built_graph(r8_built, r8):
    g, D, K = r8_built
    X = r8["features"].to(DEV)
    torch.manual_seed(50494)
    model = GCN(nfeat=r8["nfeat"], nhid=200, nclass=r8["nclass"], dropout=0.5).to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(model(X, g.adj), model(X, r8["adj"].to(DEV)))
    fac = factor.get(g.adj, Operand(X))
    assert fac is not None and fac.hubs.tolist() == list(range(D, D + K)) and (fac.k0, fac.Kc) == (0, 50)


def test_deterministic_and_strided_theta():
    D, K = 3 * C + 7, 50
    theta, sim = ref.dirichlet_theta(D, K, seed=5), ref.uniform_sim(K, seed=6)
    wide = torch.zeros((D, K + 13), dtype=torch.float64, device=DEV)
    wide[:, 5:5 + K] = _dev(theta)
    view = wide[:, 5:5 + K]
    assert not view.is_contiguous()
    s = _dev(sim)
    first = _arrays(build_topic_graph(view.contiguous(), topic_sim=s))
    for other in (build_topic_graph(view.contiguous(), topic_sim=s), build_topic_graph(view, topic_sim=s),
                  build_topic_graph(view.t().contiguous().t(), topic_sim=s)):
        for a, b in zip(first, _arrays(other)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _check(build_topic_graph(view, topic_sim=s), theta, sim)


def _embedding(K, dim, seed):
    e = np.random.default_rng(seed).standard_normal((K, dim))
    e[K // 2] = 0.0   # one zero row (the only row at K = 1)
    return e


@pytest.mark.parametrize("dim", (1, 7, 100, 7463))
@pytest.mark.parametrize("K", (1, 3, 50, 128))
def test_cosine(K, dim):
    e = _embedding(K, dim, seed=K * 10000 + dim)
    want = ref.cosine(e)
    bound = (dim + 4) * 2.0 ** -52
    for arr in (e, e.astype(np.float32)):
        got = topic_similarity(_dev(arr))
        assert got.dtype == torch.float64 and got.shape == (K, K) and got.device.type == "cuda"
        got = got.cpu().numpy()
        w = want if arr.dtype == np.float64 else ref.cosine(arr)
        err = float(np.abs(got - w).max())
        print(f"K={K} dim={dim} {arr.dtype}: max |S - S_ref| = {err:.3e} = {err / bound:.4f} of (dim + 4) 2^-52")
        assert err <= bound
        assert (got[K // 2] == 0.0).all() and (got[:, K // 2] == 0.0).all()   # the zero row: exactly 0
        assert np.array_equal(got, got.T)


def test_graph_from_embeddings_equals_graph_from_their_similarity():
    D, K, dim = C + 1, 50, 100
    theta = _dev(ref.dirichlet_theta(D, K, seed=2))
    e = _dev(np.abs(_embedding(K, dim, seed=4)))   # (non-negative rows: cosines spread over (0, 1))
    a = build_topic_graph(theta, topic_emb=e)
    b = build_topic_graph(theta, topic_sim=topic_similarity(e))
    assert a.topic_topic_edges == b.topic_topic_edges > 0
    for x, y in zip(_arrays(a), _arrays(b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    _check(a, theta.cpu().numpy(), topic_similarity(e).cpu().numpy())


@pytest.mark.parametrize("dim", (20, 100))
def test_features(dim):
    D, K = C + 1, 50
    theta = ref.dirichlet_theta(D, K, seed=9)
    e = _embedding(K, dim, seed=8).astype(np.float32)
    g = build_topic_graph(_dev(theta), topic_emb=_dev(e))
    X = g.features
    nfeat = max(K, dim)
    assert X.is_sparse and X.dtype == torch.float32 and tuple(X.shape) == (D + K, nfeat) and X is g.features
    idx, vals = X._indices().cpu().numpy(), X._values().cpu().numpy()
    assert (vals != 0).all()                                           # no explicit zeros
    key = idx[0].astype(np.int64) * nfeat + idx[1]
    assert (np.diff(key) > 0).all()                                    # row-major, no duplicates
    dense = X.to_dense().cpu().numpy()
    xd = from_theta(_dev(theta), TD)[0].cpu().numpy()
    assert np.array_equal(dense[:D, :K].view(np.uint32), xd.view(np.uint32)) and not dense[:D, K:].any()
    e64 = e.astype(np.float64)
    n = np.sqrt((e64 * e64).sum(1, keepdims=True))
    want = e64 / np.where(n == 0, 1.0, n)
    got = dense[D:, :dim].astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= ulp).all() and not dense[D:, dim:].any() and not dense[D + K // 2].any()
    assert np.count_nonzero(dense) == vals.size


def test_python_refusals():
    theta = _dev(ref.dirichlet_theta(10, 4, seed=0))
    sim = _dev(ref.uniform_sim(4, seed=0))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        build_topic_graph(theta.cpu())
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        build_topic_graph(theta, topic_sim=sim.cpu())
    with pytest.raises(ValueError):
        build_topic_graph(theta, topic_sim=sim, topic_emb=sim)
    for bad in (sim[:3], sim[:, :3], sim.to(torch.float16), sim[0]):
        with pytest.raises(RuntimeError):
            build_topic_graph(theta, topic_sim=bad)
    for bad in (theta.to(torch.float16), theta[0], theta.to(torch.int64)):
        with pytest.raises(RuntimeError):
            build_topic_graph(bad)
    with pytest.raises(RuntimeError):
        build_topic_graph(theta, topic_emb=_dev(np.ones((5, 8))))
    with pytest.raises(RuntimeError, match="unsupported"):
        build_topic_graph(_dev(np.full((4, 129), 1.0 / 129)))
    for kw in (dict(doc_topic_threshold=0.0), dict(doc_topic_threshold=-1.0), dict(topic_topic_threshold=0.0)):
        with pytest.raises(ValueError):
            build_topic_graph(theta, topic_sim=sim, **kw)
