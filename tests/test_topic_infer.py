"""TopicInferencer on the GPU (csrc/lda_estep.hip) against the float64 numpy restatement tests/lda_ref.py,
itself pinned on the CPU (test_lda_ref.py) to the reference's theta and to sklearn.  Iteration counts must be
EQUAL for every document (test_lda_ref.py shows every document far from the stop rule's edge), theta within
lda_cases.bound; rows, scorer operands and replays are compared bit for bit."""
import types

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import (GCN, DocumentScorer, TopicInferencer, datasets,
                                                                       doc_term, from_theta, inductive)

import lda_cases
import lda_ref
from lda_gpu import DEV, bits as _bits, dev as _dev

pytestmark = pytest.mark.gpu
T, W = lda_cases.T, lda_cases.W


def _docs(c, dtype=np.float64):
    return _dev(c["indptr"]), _dev(c["indices"]), _dev(c["counts"].astype(dtype))


def _inferencer(c):
    return TopicInferencer(_dev(c["beta"]), c["alpha"], c["tol"], c["max_iter"])


def _compare(what, theta, iters, ref, extra=0.0):
    """theta / iters of the device against (theta, gamma, iters, margin) of the restatement."""
    theta, iters = theta.cpu().numpy(), iters.cpu().numpy()
    assert theta.dtype == np.float64 and iters.dtype == np.int32 and theta.shape == ref[0].shape
    differ = np.flatnonzero(iters != ref[2])
    assert differ.size == 0, f"{what}: documents {differ.tolist()} ran {iters[differ]} updates, not {ref[2][differ]}"
    err = np.abs(theta - ref[0]).max(1)
    bound = lda_cases.bound(ref[2]) + extra
    worst = int((err / bound).argmax())
    print(f"{what}: worst document {worst} ({ref[2][worst]} updates): max_k |theta - theta_ref| = {err[worst]:.3e} = "
          f"{err[worst] / bound[worst]:.4f} of its bound")
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, f"{what}: documents {bad.tolist()} after {ref[2][bad]} updates miss the bound by {err[bad] / bound[bad]}"
    return float((err / bound).max())


@pytest.mark.parametrize("name", lda_cases.NAMES)
def test_case_table(name):
    c = lda_cases.table()[name]
    inf = _inferencer(c)
    theta, iters = inf(*_docs(c), return_iterations=True)
    assert theta.device.type == "cuda" and tuple(theta.shape) == (len(c["indptr"]) - 1, c["K"])
    _compare(name, theta, iters, lda_cases.reference(name))
    if c["max_iter"] == 0:
        assert torch.equal(theta, torch.full_like(theta, 1.0 / c["K"])) and not iters.any()
    # integer counts are widened exactly: the same bits as float64 counts
    for dt in (np.int32, np.int64):
        assert torch.equal(_bits(inf(*_docs(c, dt))), _bits(theta)), dt


@pytest.fixture(scope="module")
def golden():
    return lda_ref.load_golden()


def _sklearn_like(z):
    return types.SimpleNamespace(exp_dirichlet_component_=z["exp_dirichlet_component_"],
                                 doc_topic_prior_=float(z["doc_topic_prior_"]),
                                 mean_change_tol=float(z["mean_change_tol"]),
                                 max_doc_update_iter=int(z["max_doc_update_iter"]))


def test_fixture_against_restatement_and_reference(golden):
    z = golden
    inf = TopicInferencer.from_sklearn(_sklearn_like(z), DEV)
    assert (inf.K, inf.V) == z["components_"].shape
    theta, iters = inf(_dev(z["indptr"]), _dev(z["indices"]), _dev(z["counts"]), return_iterations=True)   # int64 counts
    ref = lda_cases.golden_reference()
    _compare("R8 fixture against lda_ref", theta, iters, ref)
    # against the reference's own theta: the same bound plus the 1e-13 the restatement is held to
    _compare("R8 fixture against the reference's theta", theta, iters, (z["theta"],) + tuple(ref[1:]), extra=1e-13)
    assert np.array_equal(theta.cpu().numpy() >= 0.02, z["theta"] >= 0.02)


def test_doc_term_feeds_the_same_launch(golden):
    sp = pytest.importorskip("scipy.sparse")
    z = golden
    X = sp.csr_matrix((z["counts"], z["indices"], z["indptr"]), shape=(256, z["components_"].shape[1]))
    inf = TopicInferencer.from_sklearn(_sklearn_like(z), DEV)
    ip, ix, c = doc_term(X, DEV)
    assert (ip.dtype, ix.dtype, c.dtype) == (torch.int32, torch.int32, torch.float64) and c.device.type == "cuda"
    assert torch.equal(_bits(inf(ip, ix, c)), _bits(inf(_dev(z["indptr"]), _dev(z["indices"]), _dev(z["counts"]))))


def _batch(c, order):
    """The documents ``order`` of case c as a batch of their own."""
    ip, ix, ct = c["indptr"], c["indices"], c["counts"]
    parts = [np.arange(ip[d], ip[d + 1]) for d in order]
    sel = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    indptr = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int32)
    return _dev(indptr), _dev(ix[sel.astype(np.int64)]), _dev(ct[sel.astype(np.int64)])


@pytest.mark.parametrize("name", ["K50-lengths", "K128-lengths"])
def test_a_row_does_not_depend_on_the_batch(name):
    """The same document alone, in every position of other batch sizes, beside long and empty neighbours."""
    c = lda_cases.table()[name]
    inf = _inferencer(c)
    B = len(c["indptr"]) - 1
    whole = _bits(inf(*_docs(c)))
    lengths = np.diff(c["indptr"])
    empty, longest = int(lengths.argmin()), int(lengths.argmax())
    orders = [list(range(B))[::-1], [longest] + list(range(B)) + [empty], [empty, empty] + list(range(B)) * 2,
              list(range(B)) + [longest] * (3 * W + 1)]
    orders += [[d] for d in range(B)]
    for order in orders:
        got = _bits(inf(*_batch(c, order)))
        assert torch.equal(got, whole[torch.tensor(order, device=DEV)]), order
    assert torch.equal(_bits(inf(*_docs(c))), whole)   # and the same launch twice


@pytest.mark.parametrize("name", ["K3-lengths", "K50-lengths", "K65-lengths", "B%d" % (3 * W + 7), "cap0"])
def test_scorer_operands_are_from_theta_of_the_same_theta(name):
    c = lda_cases.table()[name]
    inf = _inferencer(c)
    docs = _docs(c)
    theta = inf(*docs)
    for thr in (0.02, 1.0 / c["K"]):
        x, a = inf.scorer_operands(*docs, thr)
        wx, wa = from_theta(theta, thr)
        assert x.dtype == a.dtype == torch.float32 and x.shape == a.shape == theta.shape
        assert torch.equal(_bits(x), _bits(wx)) and torch.equal(_bits(a), _bits(wa))
        for t in (x, a):   # rows the scorer reads in place
            assert t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0
            assert inductive._rows16(t, "operand", c["K"]).data_ptr() == t.data_ptr()


def test_text_to_labels_through_the_scorer():
    """scorer_operands -> DocumentScorer.predict gives the labels of inf(...) -> from_theta -> predict."""
    K = 16
    g = datasets.doc_topic_graph(ndoc=600, ntopic=K, nclass=4, seed=1)
    torch.manual_seed(5)
    model = GCN(nfeat=g["nfeat"], nhid=32, nclass=4, dropout=0.5).to(DEV).eval()
    scorer = DocumentScorer(model, g["features"].to(DEV), g["adj"].to(DEV))
    assert scorer.Kc == K and len(scorer.hubs) == K
    c = lda_cases.table()["B%d" % (3 * W + 7)]
    inf = _inferencer(c)
    docs = _docs(c)
    x, a = inf.scorer_operands(*docs, 0.02)
    labels = scorer.predict(x, a)
    assert torch.equal(labels, scorer.predict(*from_theta(inf(*docs), 0.02)))
    assert torch.equal(scorer(x, a), scorer(*from_theta(inf(*docs), 0.02)))


def _lambda_case():
    """lambda in every branch of psi: <= 1e-6 (small-x), (1e-6, 6) (the shift loop), large."""
    rng = np.random.default_rng(77)
    K, V = 5, 1000
    lam = rng.gamma(0.3, 1.0, (K, V)) + 0.01
    lam[0, ::7] = 1e-7
    lam[1, ::5] = 1e-6
    lam[1, 1::5] = np.nextafter(1e-6, 1.0)
    lam[2, ::3] = rng.uniform(6.0, 5000.0, lam[2, ::3].shape)
    lam[3] = rng.uniform(0.01, 6.0, V)      # (below ~2e-3 the result is denormal or 0: no relative bound there)
    lam[4, 3] = 1e5
    return lam


def test_from_components():
    lam = _lambda_case()
    K, V = lam.shape
    want = lda_ref.exp_dirichlet(lam)
    inf = TopicInferencer.from_components(_dev(lam), 0.2)
    got = inf.exp_topic_word.cpu().numpy()
    assert got.shape == (K, V)
    # 8 ulp relative for psi's few operations and exp / log, plus what the serial row sum's V roundings
    # move psi(row sum) by: an absolute V 2^-53 in the exponent, so relative in the result
    bound = 8 * 2.0 ** -52 + V * 2.0 ** -53
    assert (want[0, ::7] == 0).all() and np.array_equal(got == 0, want == 0)   # exp(-1e6): exactly 0
    rel = np.abs(got - want) / np.where(want == 0, 1.0, want)
    print(f"from_components: max relative error {rel.max():.3e} = {rel.max() / bound:.4f} of 8 * 2^-52 + V * 2^-53")
    assert (rel <= bound).all()
    # and the model's own matrix, transposed only: bit for bit
    plain = TopicInferencer(_dev(want), 0.2)
    assert np.array_equal(plain.exp_topic_word.cpu().numpy(), want)
    # an in-place change of the model rebuilds the table (derived.py's rule)
    src = _dev(want)
    held = TopicInferencer(src, 0.2)
    src.mul_(0.5)
    assert np.array_equal(held.exp_topic_word.cpu().numpy(), want * 0.5)


@pytest.mark.parametrize("name", ["K50-lengths", "K128-lengths", "cap0"])
def test_gamma_normalises_to_theta(name):
    c = lda_cases.table()[name]
    inf = _inferencer(c)
    docs = _docs(c)
    theta, gamma = inf(*docs), inf.gamma(*docs)
    ref = lda_cases.reference(name)
    assert np.allclose(gamma.cpu().numpy(), ref[1], rtol=1e-9, atol=0)   # (it IS gamma; theta carries the precision claim)
    # the kernel's sum over topics ascends (numpy's and torch's sum(1) are pairwise / tree sums)
    total = torch.zeros(gamma.shape[0], dtype=torch.float64, device=DEV)
    for k in range(gamma.shape[1]):
        total = total + gamma[:, k]
    assert torch.equal(_bits(gamma / total[:, None]), _bits(theta))
    # two orders of summing K positive terms differ by at most 2 (K - 1) 2^-53 relative; the quotient adds one rounding
    assert float((gamma / gamma.sum(1, keepdim=True) - theta).abs().max()) <= c["K"] * 2.0 ** -52


def test_captured_calls_replay_the_eager_bits():
    c = lda_cases.table()["K50-lengths"]
    inf = _inferencer(c)
    docs = _docs(c)
    theta, iters = inf(*docs, return_iterations=True)   # (also loads the kernel before the capture)
    x, a = inf.scorer_operands(*docs, 0.02)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                            # a single chain on one stream
        t2, i2 = inf(*docs, return_iterations=True)
        x2, a2 = inf.scorer_operands(*docs, 0.02)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(t2), _bits(theta)) and torch.equal(i2, iters)
    assert torch.equal(_bits(x2), _bits(x)) and torch.equal(_bits(a2), _bits(a))
    del g


def test_python_refusals():
    c = lda_cases.table()["B1"]
    inf = _inferencer(c)
    ip, ix, ct = _docs(c)
    with pytest.raises(RuntimeError, match="float32 E-step"):
        inf(ip, ix, ct.to(torch.float32))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        inf(ip.cpu(), ix, ct)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        TopicInferencer(torch.from_numpy(c["beta"]), 0.1)
    for bad in ((ip.to(torch.int64), ix, ct), (ip, ix.to(torch.int64), ct), (ip, ix, ct.to(torch.float16)),
                (ip, ix[:-1], ct), (ip[:1], ix, ct)):
        with pytest.raises(RuntimeError):
            inf(*bad)
    with pytest.raises(RuntimeError):
        TopicInferencer(_dev(c["beta"]).to(torch.float32), 0.1)
    with pytest.raises(RuntimeError):
        TopicInferencer(_dev(c["beta"]), 0.1, max_doc_update_iter=10001)
    with pytest.raises(RuntimeError, match="unsupported"):
        TopicInferencer(_dev(np.full((129, 10), 0.1)), 0.1)
