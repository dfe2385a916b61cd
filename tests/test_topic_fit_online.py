"""The online topic-model fit on the GPU (csrc/lda_estep.hip: gcnk_lda_mstep_online_f64, and the minibatch loop
of fit_topics(learning_method="online") and OnlineTopics.partial_fit) against the float64 numpy restatement
tests/lda_ref.py, itself pinned on the CPU (test_lda_ref.py) to the reference's online fit and to
sklearn.  Expected values never come from the code under test.

  online M-step  on the restatement's own inputs, lambda BIT FOR BIT the serial loop's: every operation is a
                 correctly rounded multiply or add in a fixed order; guard columns untouched.
  rho = 1        one minibatch of all the documents at learning_decay = 0 is bit for bit the batch fit.
  whole fit      on the R8 fixture's runs a and b: update counts equal in all EM iterations, lambda within
                 16 max(d_ref, d_perm) of the recorded components_, n_batch_iter equal.
  OnlineTopics   run c (two partial_fit calls) within the same bound; from_fit + partial_fit bit for bit the
                 longer online fit; the inferencer.
  determinism    the host draw, a second run, a hipGraph replay, and a minibatch alone or inside a larger matrix.
"""
import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import (OnlineTopics, TopicInferencer, _lib, fit_topics,
                                                                      topic_fit)

import lda_online_cases
import lda_ref
from lda_gpu import DEV, GUARD, bits as _bits, dev as _dev, mstep_online as _mstep_online

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", lda_online_cases.NAMES)
def test_online_mstep_is_bit_for_bit_the_serial_loop(name):
    c = lda_online_cases.table()[name]
    want = lda_online_cases.reference(name)
    out = _mstep_online(c).cpu().numpy()
    got, guard = np.ascontiguousarray(out[:, :c["V"]]), out[:, c["V"]:]
    off = np.argwhere(got.view(np.int64) != want.view(np.int64))
    print(f"{name}: {len(off)} of {got.size} entries differ from the serial loop (the demand is 0: bit for bit)")
    assert off.size == 0, f"{name}: {len(off)} entries differ, first (k, w) = {off[0].tolist()}: {got[tuple(off[0])]!r} != {want[tuple(off[0])]!r}"
    assert guard.shape[1] == c["pad"] and np.all(guard == GUARD)
    if c["rho"] == 1.0:   # lambda * +0: nothing of the old lambda is left
        again = dict(c, lam=c["lam"] * 3.0)
        assert np.array_equal(_mstep_online(again).cpu().numpy()[:, :c["V"]].view(np.int64), want.view(np.int64))


@pytest.fixture(scope="module")
def golden():
    return lda_ref.load_fit_golden(), lda_ref.load_online_golden()


@pytest.fixture(scope="module")
def docs(golden):
    z = golden[0]
    return _dev(z["indptr"]), _dev(z["indices"]), _dev(z["counts"])


def _fit(z, docs, init=True, max_iter=3, **kw):
    return fit_topics(*docs, int(z["V"]), num_topics=z["components_"].shape[0], max_iter=max_iter,
                      random_state=int(z["random_state"]), mean_change_tol=float(z["mean_change_tol"]),
                      max_doc_update_iter=int(z["max_doc_update_iter"]),
                      init=(_dev(z["lambda0"]), _dev(z["gamma0"][:max_iter])) if init else None, **kw)


@pytest.fixture(scope="module")
def fitted(golden, docs):
    """key -> the online fit of fixture run a (batch_size 128) and b (64), from the stored draws."""
    return {key: _fit(golden[0], docs, return_iterations=True, learning_method="online", batch_size=bs)
            for key, bs in (("a", 128), ("b", 64))}


def test_rho_one_in_one_minibatch_is_the_batch_fit_bit_for_bit(golden, docs):
    z = golden[0]
    batch = _fit(z, docs, return_iterations=True)
    online = _fit(z, docs, return_iterations=True, learning_method="online", learning_decay=0.0, batch_size=200)
    assert torch.equal(online.iterations, batch.iterations)
    off = torch.nonzero(_bits(online.components) != _bits(batch.components))
    assert off.numel() == 0, f"{len(off)} entries differ, first (k, w) = {off[0].tolist()}"
    assert torch.equal(_bits(online.exp_topic_word), _bits(batch.exp_topic_word))
    assert torch.equal(_bits(online.topic_word_distribution), _bits(batch.topic_word_distribution))
    assert online.n_batch_iter == batch.n_batch_iter == 4      # sklearn counts one M-step an EM iteration for both
    larger = _fit(z, docs, learning_method="online", learning_decay=0.0, batch_size=1000)   # (one minibatch as well)
    assert torch.equal(_bits(larger.components), _bits(batch.components))


@pytest.mark.parametrize("key", ["a", "b"])
def test_whole_online_fit_against_the_reference(golden, fitted, key):
    (z, o), fit = golden, fitted[key]
    K, V = z["components_"].shape
    want = o[f"{key}_components_"]
    assert fit.components.device.type == "cuda" and tuple(fit.components.shape) == (K, V)
    its = fit.iterations.cpu().numpy()
    assert its.dtype == np.int32 and its.shape == (3, 200)
    differ = np.argwhere(its != o[f"{key}_iterations"])
    assert differ.size == 0, f"(EM iteration, document) {differ.tolist()} ran {its[its != o[f'{key}_iterations']]} updates"
    assert fit.n_batch_iter == int(o[f"{key}_n_batch_iter_"]) and fit.n_iter == 3
    lam = fit.components.cpu().numpy()
    bound = 16.0 * max(float(o[f"{key}_d_ref"]), float(o[f"{key}_d_perm"]))
    d = lda_ref.max_rel(lam, want)
    print(f"online fit {key}: max relative |lambda - recorded components_| = {d:.3e} = {d / bound:.4f} of "
          f"16 max(d_ref, d_perm) = {bound:.3e}")
    assert d <= bound
    tw = fit.topic_word_distribution.cpu().numpy()
    assert np.abs(tw.sum(1) - 1).max() <= 1e-12
    # test_whole_fit_against_the_reference's two bounds: lambda_kw / sum_w lambda_kw, the numerator within `bound`,
    # the sum of V positive terms within `bound` and its own V roundings in whatever order, one division;
    want_tw = o["a_topic_word_distribution"] if key == "a" else want / want.sum(axis=1, keepdims=True)
    assert lda_ref.max_rel(tw, want_tw) <= 2 * bound + (V + 1) * 2.0 ** -52
    # and the last table is exp_dirichlet of the fitted lambda
    assert lda_ref.max_rel(fit.exp_topic_word.cpu().numpy(), lda_ref.exp_dirichlet(lam)) <= 8 * 2.0 ** -52 + V * 2.0 ** -53


def _online_topics(z, o, **kw):
    return OnlineTopics(int(z["V"]), num_topics=8, total_samples=int(o["c_total_samples"]),
                        batch_size=int(o["c_batch_size"]), random_state=int(z["random_state"]),
                        mean_change_tol=float(z["mean_change_tol"]), max_doc_update_iter=int(z["max_doc_update_iter"]), **kw)


def _first(docs, n, z):
    hi = int(z["indptr"][n])
    return docs[0][:n + 1], docs[1][:hi], docs[2][:hi]


def test_two_partial_fit_calls_against_sklearn(golden, docs):
    z, o = golden
    second = int(o["c_second"])
    g0 = _dev(o["c_gamma0"])
    ot = _online_topics(z, o, init_components=_dev(z["lambda0"]))
    assert ot.n_batch_iter == 1 and ot.partial_fit(*docs, gamma0=g0[:200], return_iterations=True) is ot
    its = [ot.iterations.cpu().numpy()]
    assert ot.n_batch_iter == 5
    ot.partial_fit(*_first(docs, second, z), gamma0=g0[200:], return_iterations=True)
    its.append(ot.iterations.cpu().numpy())
    assert ot.n_batch_iter == int(o["c_n_batch_iter_"])
    assert np.array_equal(np.concatenate(its), o["c_iterations"])
    lam = ot.components.cpu().numpy()
    bound = 16.0 * max(float(o["c_d_ref"]), float(o["c_d_perm"]))
    d = lda_ref.max_rel(lam, o["c_components_"])
    print(f"two partial_fit calls: max relative |lambda - sklearn's components_| = {d:.3e} = {d / bound:.4f} of "
          f"16 max(d_ref, d_perm) = {bound:.3e}")
    assert d <= bound
    V = int(z["V"])
    assert lda_ref.max_rel(ot.exp_topic_word.cpu().numpy(), lda_ref.exp_dirichlet(lam)) <= 8 * 2.0 ** -52 + V * 2.0 ** -53
    assert float((ot.topic_word_distribution.sum(1) - 1).abs().max()) <= 1e-12
    # the host draws: lambda0, then a (B, K) gamma0 per call from the same RandomState
    drawn = _online_topics(z, o, device=DEV)
    drawn.partial_fit(*docs).partial_fit(*_first(docs, second, z))
    assert drawn.iterations is None and drawn.n_batch_iter == ot.n_batch_iter
    assert torch.equal(_bits(drawn.components), _bits(ot.components))
    assert torch.equal(_bits(drawn.exp_topic_word), _bits(ot.exp_topic_word))


def test_from_fit_then_partial_fit_is_the_longer_online_fit(golden, docs):
    z = golden[0]
    kw = dict(learning_method="online", batch_size=64)
    two = _fit(z, docs, max_iter=2, return_iterations=True, **kw)
    one = _fit(z, docs, max_iter=1, **kw)
    assert (one.n_batch_iter, two.n_batch_iter) == (5, 9)
    ot = OnlineTopics.from_fit(one, total_samples=200, batch_size=64)
    kept = one.components.clone()
    ot.partial_fit(*docs, gamma0=_dev(z["gamma0"][1]), return_iterations=True)
    assert torch.equal(_bits(one.components), _bits(kept))          # the fit's own lambda is left alone
    assert ot.n_batch_iter == two.n_batch_iter and torch.equal(ot.iterations, two.iterations[1])
    assert torch.equal(_bits(ot.components), _bits(two.components))
    assert torch.equal(_bits(ot.exp_topic_word), _bits(two.exp_topic_word))
    assert torch.equal(_bits(ot.topic_word_distribution), _bits(two.topic_word_distribution))
    assert (ot.doc_topic_prior, ot.topic_word_prior) == (two.doc_topic_prior, two.topic_word_prior)
    # from a BATCH fit too: n_batch_iter goes on from 1 + its EM iterations
    batch = _fit(z, docs, max_iter=1)
    assert OnlineTopics.from_fit(batch, total_samples=200).partial_fit(*docs).n_batch_iter == 2 + 2


def test_inferencer_is_from_components_of_the_current_lambda(golden, docs):
    z, o = golden
    ot = _online_topics(z, o, init_components=_dev(z["lambda0"])).partial_fit(*docs, gamma0=_dev(o["c_gamma0"][:200]))
    inf = ot.inferencer()
    other = TopicInferencer.from_components(ot.components.clone(), ot.doc_topic_prior, ot.mean_change_tol,
                                            ot.max_doc_update_iter)
    theta = inf(*docs)
    assert tuple(theta.shape) == (200, 8) and torch.equal(_bits(theta), _bits(other(*docs)))
    assert torch.equal(_bits(inf.exp_topic_word), _bits(ot.exp_topic_word))
    ot.partial_fit(*_first(docs, 70, z), gamma0=_dev(o["c_gamma0"][200:]))    # the model moves on, the inferencer stays
    assert torch.equal(_bits(inf(*docs)), _bits(theta))
    assert not torch.equal(_bits(ot.inferencer()(*docs)), _bits(theta))


def test_host_draw_second_run_and_replay_are_bit_for_bit(golden, docs, fitted):
    z, fit = golden[0], fitted["b"]
    kw = dict(learning_method="online", batch_size=64)
    drawn = _fit(z, docs, init=False, **kw)                    # RandomState(42) on the host, uploaded
    assert drawn.iterations is None
    assert torch.equal(_bits(drawn.components), _bits(fit.components))
    again = _fit(z, docs, return_iterations=True, **kw)
    assert torch.equal(_bits(again.components), _bits(fit.components)) and torch.equal(again.iterations, fit.iterations)
    assert torch.equal(_bits(again.topic_word_distribution), _bits(fit.topic_word_distribution))
    init = (_dev(z["lambda0"]), _dev(z["gamma0"]))
    args = dict(num_topics=8, max_iter=3, mean_change_tol=float(z["mean_change_tol"]),
                max_doc_update_iter=int(z["max_doc_update_iter"]), init=init, return_iterations=True, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # a single chain on one stream
        cap = fit_topics(*docs, int(z["V"]), **args)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(cap.components), _bits(fit.components)) and torch.equal(cap.iterations, fit.iterations)
    assert torch.equal(_bits(cap.topic_word_distribution), _bits(fit.topic_word_distribution))
    assert torch.equal(_bits(cap.exp_topic_word), _bits(fit.exp_topic_word)) and cap.n_batch_iter == fit.n_batch_iter
    assert torch.equal(_bits(init[0]), _bits(_dev(z["lambda0"])))   # lambda0 is not worked on in place
    del g


def _one_minibatch(indptr, indices, counts, b0, b1, lam0, gamma0, z, rho, doc_ratio):
    """exp_dirichlet -> fit E-step on rows [b0, b1) -> online M-step of that minibatch, by the entry points: the
    new lambda.  gamma0 is [B x K] of the matrix given."""
    K, V = lam0.shape
    B, nnz = indptr.numel() - 1, indices.numel()
    lib, stream = _lib.load(), _lib.stream(torch.device(DEV))
    ix = topic_fit.word_index(indptr, indices, V)
    table = torch.zeros((V, K), dtype=torch.float64, device=DEV)
    lam = lam0.clone()
    etheta = torch.full((B, K), float("nan"), dtype=torch.float64, device=DEV)
    ratio = torch.full((nnz,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.gcnk_lda_exp_dirichlet_f64(lam.data_ptr(), V, K, V, table.data_ptr(), K, stream), "exp_dirichlet")
    _lib.check(lib.gcnk_lda_estep_fit_f64(
        indptr[b0:].data_ptr(), indices.data_ptr(), counts.data_ptr(), 2, b1 - b0, V, K, table.data_ptr(), K,
        float(z["doc_topic_prior_"]), float(z["mean_change_tol"]), int(z["max_doc_update_iter"]), gamma0[b0:].data_ptr(), K,
        nnz, ratio.data_ptr(), etheta[b0:].data_ptr(), K, None, 0, None, stream), "estep_fit")
    _lib.check(lib.gcnk_lda_mstep_online_f64(
        ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), nnz, b0, b1, ratio.data_ptr(), etheta.data_ptr(), K, B,
        V, K, table.data_ptr(), K, float(z["topic_word_prior_"]), rho, doc_ratio, lam.data_ptr(), V, stream), "mstep_online")
    return lam, etheta, ratio


def test_a_minibatch_does_not_depend_on_the_rows_outside_it(golden, docs):
    """Rows [64, 128) of the 200 as one minibatch, and the same 64 documents as a matrix of their own."""
    z = golden[0]
    assert docs[2].dtype == torch.int64 and z["components_"].shape[0] % 2 == 0
    lam0, g0 = _dev(z["lambda0"]), _dev(z["gamma0"][0])
    rho, doc_ratio = lda_ref.rho_of(10.0, 1, 0.7), 200.0 / 64
    inside, etheta, ratio = _one_minibatch(*docs, 64, 128, lam0, g0, z, rho, doc_ratio)
    lo, hi = int(z["indptr"][64]), int(z["indptr"][128])
    assert not torch.isnan(etheta[64:128]).any() and torch.isnan(etheta[:64]).all() and torch.isnan(etheta[128:]).all()
    assert not torch.isnan(ratio[lo:hi]).any() and torch.isnan(ratio[:lo]).all() and torch.isnan(ratio[hi:]).all()
    own = ((docs[0][64:129] - lo).contiguous(), docs[1][lo:hi].contiguous(), docs[2][lo:hi].contiguous())
    alone, _, _ = _one_minibatch(*own, 0, 64, lam0, g0[64:128].contiguous(), z, rho, doc_ratio)
    assert not torch.isnan(inside).any() and not torch.equal(_bits(inside), _bits(lam0))
    off = torch.nonzero(_bits(inside) != _bits(alone))
    assert off.numel() == 0, f"{len(off)} entries differ, first (k, w) = {off[0].tolist()}"
    # and by the public route: one partial_fit of those 64 documents at total_samples = 200
    ot = OnlineTopics(int(z["V"]), num_topics=8, total_samples=200, batch_size=64, init_components=lam0,
                      mean_change_tol=float(z["mean_change_tol"]), max_doc_update_iter=int(z["max_doc_update_iter"]))
    assert torch.equal(_bits(ot.partial_fit(*own, gamma0=g0[64:128]).components), _bits(inside))


def test_online_fit_of_documents_without_a_word_is_the_blend_of_lambda0_and_the_prior():
    """No stored nonzero at all: S = 0 in every minibatch, so lambda is the closed-form blend of lambda0 and eta,
    the same operations in the same order, bit for bit; every document stops where the restatement does."""
    B, V, K, eta = 3, 7, 5, 0.3
    ip = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    ix = torch.zeros(0, dtype=torch.int32, device=DEV)
    ct = torch.zeros(0, dtype=torch.float64, device=DEV)
    fit = fit_topics(ip, ix, ct, V, num_topics=K, max_iter=2, random_state=3, topic_word_prior=eta, return_iterations=True,
                     learning_method="online", batch_size=2)
    lam0, g0s = lda_ref.draws(3, K, V, B, 2)
    lam, n = lam0.copy(), 1
    for _ in range(2):
        for b0, b1 in ((0, 2), (2, 3)):
            rho = np.float64(np.power(10.0 + n, -0.7))
            beta = lda_ref.exp_dirichlet(lam)
            v = rho * (np.float64(eta) + np.float64(3.0 / (b1 - b0)) * (np.zeros((K, V)) * beta))
            lam = lam * (np.float64(1.0) - rho) + v
            n += 1
    assert fit.n_batch_iter == n == 5
    assert np.array_equal(fit.components.cpu().numpy().view(np.int64), lam.view(np.int64))
    want, iters, _, _ = lda_ref.fit_online(np.zeros(B + 1, np.int32), np.zeros(0, np.int32), np.zeros(0), lam0, g0s,
                                                  1.0 / K, eta, batch_size=2)
    assert np.array_equal(want.view(np.int64), lam.view(np.int64))
    assert np.array_equal(fit.iterations.cpu().numpy(), iters)
    assert float((fit.topic_word_distribution.sum(1) - 1).abs().max()) <= 1e-12
