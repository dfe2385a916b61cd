"""TopicBound, fit.bound and evaluate_every on the GPU (csrc/lda_estep.hip: gcnk_lda_bound_{docs,topics,finish}_f64)
against the float64 numpy restatement tests/lda_bound_ref.py, itself pinned on the CPU (test_lda_bound_ref.py) to
sklearn's own bound, score and perplexity of the reference's model.  Expected values never come from the code
under test.

  rule        a value is near when |x - y| <= 16 max(d_ref, d_perm, d_fn) 2^-52 A, A the sum of its absolute addends
              and the d's the fixture's recorded distances (test_topic_fit.py's rule and factor), element by element
              for the partials; a perplexity exp(-bound / count) carries the bound's allowance over the count.
  fixture     parts(), bound, score, perplexity, fit.bound against the restatement and sklearn's recorded values.
  stop rule   fit_topics(evaluate_every=2) stops at sklearn's n_iter_ with the restatement's perplexities.
  determinism bitwise: a second run, a document alone / first / last / in a row range, the count kinds.
"""
import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import (OnlineTopics, TopicBound, _lib, fit_topics,
                                                                      topic_bound)

import lda_bound_cases
import lda_bound_ref as R
import lda_fit_cases
from lda_gpu import DEV, GUARD, bits as _bits, dev as _dev

pytestmark = pytest.mark.gpu

_worst = {"parts": 0.0, "total": 0.0}


def _docs(c, prefix=""):
    return _dev(c[prefix + "indptr"]), _dev(c[prefix + "indices"]), _dev(c[prefix + "counts"])


def _near(what, got, ref, parts=None):
    """``got`` = (doc_bound, topic_bound) and / or a [3] result on the host against a restatement's evaluate()."""
    f_parts, f_total = lda_bound_cases.factors()
    if parts is not None:
        d = max(R.distance(parts[0], ref["doc"], ref["A_doc"]), R.distance(parts[1], ref["topic"], ref["A_topic"]))
        _worst["parts"] = max(_worst["parts"], d / f_parts)
        print(f"{what}: partials {d:.3f} x 2^-52 A = {d / f_parts:.4f} of the bound {f_parts:.1f}; worst so far {_worst['parts']:.4f}")
        assert d <= f_parts, (what, d, f_parts)
    if got is not None:
        bound, count, perp = (float(v) for v in got)
        d = R.distance(bound, ref["bound"], ref["A"])
        _worst["total"] = max(_worst["total"], d / f_total)
        print(f"{what}: bound {bound!r} at {d:.3f} x 2^-52 A = {d / f_total:.4f} of the bound {f_total:.1f}; worst so far {_worst['total']:.4f}")
        assert d <= f_total, (what, bound, ref["bound"], d, f_total)
        assert count == ref["count"]
        assert abs(perp - ref["perplexity"]) <= _perplexity_slack(ref) * ref["perplexity"], (what, perp, ref["perplexity"])


def _perplexity_slack(ref, count=None):
    """The relative allowance of exp(-bound / count): the bound's own over the count, and four roundings of the
    exponent for the division and the exp."""
    count = ref["count"] if count is None else count
    return lda_bound_cases.factors()[1] * R.ULP * ref["A"] / count + 4 * R.ULP * max(1.0, abs(ref["bound"]) / count)


def _scorer(c):
    return TopicBound(_dev(c["lam"]), c["alpha"], c["eta"])


@pytest.mark.parametrize("name", lda_bound_cases.NAMES)
def test_case_table(name):
    c, ref = lda_bound_cases.table()[name], lda_bound_cases.reference(name)
    tb, docs, gamma = _scorer(c), _docs(c), _dev(c["gamma"])
    doc, topic = tb.parts(*docs, gamma)
    assert doc.dtype == topic.dtype == torch.float64 and tuple(doc.shape) == (len(c["indptr"]) - 1,) and tuple(topic.shape) == (c["K"],)
    out = topic_bound.finish(doc, topic, docs[0], docs[2], 1.0)
    _near(name, out.cpu().numpy(), ref, (doc.cpu().numpy(), topic.cpu().numpy()))
    b = tb.bound(*docs, gamma)
    assert b.dim() == 0 and b.dtype == torch.float64 and torch.equal(_bits(b), _bits(out[0]))


@pytest.fixture(scope="module")
def z():
    return lda_bound_cases.golden()


@pytest.fixture(scope="module")
def scorer(z):
    return TopicBound(_dev(z["components_"]), float(z["doc_topic_prior_"]), float(z["topic_word_prior_"]),
                      float(z["mean_change_tol"]), int(z["max_doc_update_iter"]))


@pytest.mark.parametrize("which", ["train", "held"])
def test_fixture_parts_score_and_perplexity(z, scorer, which):
    docs = _docs(z, which + "_")
    ref = lda_bound_cases.golden_reference(which)
    doc, topic = scorer.parts(*docs)
    score, perp = scorer.score(*docs), scorer.perplexity(*docs)
    assert score.dim() == 0 and perp.dim() == 0 and score.device.type == "cuda"
    _near(which, (float(score), ref["count"], float(perp)), ref, (doc.cpu().numpy(), topic.cpu().numpy()))
    # ... and sklearn's own recorded numbers, under the same allowance
    f_total = lda_bound_cases.factors()[1]
    d = R.distance(float(score), float(z[f"{which}_score"]), ref["A"])
    print(f"{which}: score {float(score)!r} against sklearn's {float(z[f'{which}_score'])!r}: {d / f_total:.4f} of the bound")
    assert d <= f_total
    assert abs(float(perp) - float(z[f"{which}_perplexity"])) <= _perplexity_slack(ref) * float(z[f"{which}_perplexity"])


def test_fixture_bound_of_a_given_gamma_and_sub_sampling(z, scorer):
    docs, gamma = _docs(z, "held_"), _dev(z["held_gamma"])
    args = (z["held_indptr"], z["held_indices"], z["held_counts"], z["held_gamma"], z["components_"],
            float(z["doc_topic_prior_"]), float(z["topic_word_prior_"]))
    ref = R.evaluate(*args)
    b = scorer.bound(*docs, gamma)
    _near("held, sklearn's gamma", (float(b), ref["count"], ref["perplexity"]), ref)
    assert R.distance(float(b), float(z["held_score"]), ref["A"]) <= lda_bound_cases.factors()[1]
    sub = R.evaluate(*args, doc_ratio=1000.0 / 60)
    got = scorer._evaluate(*docs, gamma, True, 1000).cpu().numpy()
    _near("held, sub-sampled", got, sub)
    assert torch.equal(_bits(scorer.bound(*docs, gamma, sub_sampling=True, total_samples=1000)), _bits(_dev(got[:1])[0]))


def _fit(z, **kw):
    docs = _docs(z, "train_")
    kw.setdefault("max_iter", 3)
    return fit_topics(*docs, int(z["V"]), num_topics=8, mean_change_tol=float(z["mean_change_tol"]),
                      max_doc_update_iter=int(z["max_doc_update_iter"]),
                      init=(_dev(z["lambda0"]), _dev(z["gamma0"][:kw["max_iter"]])), **kw), docs


def test_fit_bound_is_sklearns_bound_(z):
    fit, docs = _fit(z, compute_bound=True)
    plain, _ = _fit(z)
    assert plain.bound is None and plain.perplexities == [] and plain.n_iter == 3 and plain.n_batch_iter == 4
    assert torch.equal(_bits(plain.components), _bits(fit.components))      # the closing evaluation moves nothing
    assert fit.bound.dim() == 0 and fit.bound.dtype == torch.float64 and fit.n_iter == 3 and fit.perplexities == []
    lam = lda_fit_cases.golden_fit()[0]                                     # the restatement's fit of the same draws
    ref = R.score(z["train_indptr"], z["train_indices"], z["train_counts"], lam, float(z["doc_topic_prior_"]),
                  float(z["topic_word_prior_"]), float(z["mean_change_tol"]), int(z["max_doc_update_iter"]))
    got = float(fit.bound)
    slack = _perplexity_slack(ref)
    print(f"fit.bound {got!r}: the restatement {ref['perplexity']!r}, sklearn's bound_ {float(z['bound_'])!r}; "
          f"{abs(got - ref['perplexity']) / (slack * ref['perplexity']):.4f} and "
          f"{abs(got - float(z['bound_'])) / (slack * float(z['bound_'])):.4f} of the allowance")
    assert abs(got - ref["perplexity"]) <= slack * ref["perplexity"]
    assert abs(got - float(z["bound_"])) <= slack * float(z["bound_"])
    assert torch.equal(_bits(fit.scorer().perplexity(*docs)), _bits(fit.bound))


@pytest.mark.parametrize("method", ["batch", "online"])
def test_evaluate_every_stops_where_sklearn_stops(z, method):
    want_n, want = int(z[f"ee_{method}_n_iter"]), z[f"ee_{method}_perplexities"]
    fit, docs = _fit(z, max_iter=12, evaluate_every=2, perp_tol=float(z[f"ee_{method}_perp_tol"]), learning_method=method)
    assert fit.n_iter == want_n and fit.n_batch_iter == int(z[f"ee_{method}_n_batch_iter"])
    assert len(fit.perplexities) == len(want) and all(isinstance(p, float) for p in fit.perplexities)
    train = lda_bound_cases.golden_reference("train")            # A and the count of these documents' bound
    slack = _perplexity_slack(train)
    frac = [abs(p - w) / (slack * w) for p, w in zip(fit.perplexities, want)]
    print(f"{method}: perplexities {fit.perplexities} at {[round(f, 4) for f in frac]} of the allowance")
    assert max(frac) <= 1.0
    closing = float(z[f"ee_{method}_bound_"])
    assert abs(float(fit.bound) - closing) <= slack * closing and float(fit.bound) == fit.perplexities[-1]
    # the evaluations move nothing: the same EM iterations without them give the same lambda, bit for bit
    plain, _ = _fit(z, max_iter=want_n + 1, learning_method=method)
    assert torch.equal(_bits(plain.components), _bits(fit.components)) and plain.n_batch_iter == fit.n_batch_iter


def test_evaluate_every_that_never_stops_and_its_refusal_in_a_capture(z, monkeypatch):
    fit, docs = _fit(z, max_iter=3, evaluate_every=1, perp_tol=0.0)
    assert fit.n_iter == 3 and len(fit.perplexities) == 3 and float(fit.bound) == fit.perplexities[-1]
    plain, _ = _fit(z)
    assert torch.equal(_bits(plain.components), _bits(fit.components))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        _fit(z, evaluate_every=1)


def test_compute_bound_is_captured_and_replayed(z):
    fit, docs = _fit(z, compute_bound=True)
    init = (_dev(z["lambda0"]), _dev(z["gamma0"][:3]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # a single chain on one stream, no host read
        cap = fit_topics(*docs, int(z["V"]), num_topics=8, max_iter=3, mean_change_tol=float(z["mean_change_tol"]),
                         max_doc_update_iter=int(z["max_doc_update_iter"]), init=init, compute_bound=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(cap.components), _bits(fit.components)) and torch.equal(_bits(cap.bound), _bits(fit.bound))
    del g


def test_second_run_and_batch_independence_are_bitwise():
    c = lda_bound_cases.table()["K65-lengths"]
    tb, gamma = _scorer(c), c["gamma"]
    B = len(c["indptr"]) - 1
    whole_doc, whole_topic = tb.parts(*_docs(c), _dev(gamma))
    again_doc, again_topic = _scorer(c).parts(*_docs(c), _dev(gamma))
    assert torch.equal(_bits(again_doc), _bits(whole_doc)) and torch.equal(_bits(again_topic), _bits(whole_topic))
    longest = int(np.diff(c["indptr"]).argmax())
    orders = [[d] for d in range(B)] + [list(range(B))[::-1], [longest] + list(range(B)), list(range(B)) + [0, longest] * 2]
    for order in orders:
        sel = [np.arange(c["indptr"][d], c["indptr"][d + 1]) for d in order]
        flat = np.concatenate(sel).astype(np.int64)
        indptr = np.concatenate([[0], np.cumsum([s.size for s in sel])]).astype(np.int32)
        if flat.size == 0:
            continue    # (a batch without any word is test_documents_without_a_word's)
        doc, topic = tb.parts(_dev(indptr), _dev(c["indices"][flat]), _dev(c["counts"][flat]), _dev(gamma[order]))
        assert torch.equal(_bits(doc), _bits(whole_doc[torch.tensor(order, device=DEV)])), order
        assert torch.equal(_bits(topic), _bits(whole_topic))          # the topic term does not see the documents
    # a row range of the whole matrix: indptr advanced, the whole indices and counts
    ip, ix, ct = _docs(c)
    doc, _ = tb.parts(ip[2:5], ix, ct, _dev(gamma)[2:4])
    assert torch.equal(_bits(doc), _bits(whole_doc[2:4]))
    out = topic_bound.finish(doc, whole_topic, ip[2:5], ct, 1.0).cpu().numpy()
    lo, hi = int(c["indptr"][2]), int(c["indptr"][4])
    assert out[1] == R.dealt_sum(c["counts"][lo:hi], R.FINISH_THREADS)


def test_documents_without_a_word():
    """No stored nonzero at all: every document is its Dirichlet term, the count 0 and the perplexity exp(-(x / 0))."""
    c = lda_bound_cases.table()["B3"]
    tb = _scorer(c)
    B = 3
    ip = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    ix, ct = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV)
    doc, topic = tb.parts(ip, ix, ct, _dev(c["gamma"]))
    ref = R.evaluate(np.zeros(B + 1, np.int32), np.zeros(0, np.int32), np.zeros(0), c["gamma"], c["lam"], c["alpha"], c["eta"])
    assert R.distance(doc.cpu().numpy(), ref["doc"], ref["A_doc"]) <= lda_bound_cases.factors()[0]
    # ... and the same document's term in a batch that has words: its own words alone decide it
    whole, _ = tb.parts(*_docs(c), _dev(c["gamma"]))
    assert torch.equal(_bits(whole[1]), _bits(doc[1]))               # (document 1 of B3 has no word)
    out = topic_bound.finish(doc, topic, ip, torch.zeros(1, dtype=torch.float64, device=DEV), 1.0).cpu().numpy()
    assert out[1] == 0.0 and R.distance(out[0], ref["bound"], ref["A"]) <= lda_bound_cases.factors()[1]


def test_count_kinds_leading_dimensions_and_guards():
    c = lda_bound_cases.table()["B3"]
    K, V, B = c["K"], c["V"], 3
    ip, ix, ct = _docs(c)
    tb = _scorer(c)
    gamma = _dev(c["gamma"])
    doc, topic = tb.parts(ip, ix, ct, gamma)
    want = topic_bound.finish(doc, topic, ip, ct, 1.0)
    for dtype in (torch.int32, torch.int64):
        d2, _ = tb.parts(ip, ix, ct.to(dtype), gamma)
        assert torch.equal(_bits(d2), _bits(doc))
        assert torch.equal(_bits(topic_bound.finish(d2, topic, ip, ct.to(dtype), 1.0)), _bits(want))
    # leading dimensions above K and V: a padded gamma and a padded lambda (views, not copies)
    wide_gamma = torch.full((B, K + 3), float("nan"), dtype=torch.float64, device=DEV)
    wide_gamma[:, :K] = gamma
    wide_lam = torch.full((K, V + 5), float("nan"), dtype=torch.float64, device=DEV)
    wide_lam[:, :V] = _dev(c["lam"])
    padded = TopicBound(wide_lam[:, :V], c["alpha"], c["eta"])
    assert padded.components.data_ptr() == wide_lam.data_ptr() and padded.components.stride(0) == V + 5
    d3, t3 = padded.parts(ip, ix, ct, wide_gamma[:, :K])
    assert torch.equal(_bits(d3), _bits(doc)) and torch.equal(_bits(t3), _bits(topic))
    # the entry points write doc_bound[B], topic_bound[K] and out[3] and nothing behind them
    lib, stream = _lib.load(), _lib.stream(torch.device(DEV))
    table = tb.inferencer._table().t
    g_doc = torch.full((B + 2,), GUARD, dtype=torch.float64, device=DEV)
    g_topic = torch.full((K + 2,), GUARD, dtype=torch.float64, device=DEV)
    g_out = torch.full((5,), GUARD, dtype=torch.float64, device=DEV)
    _lib.check(lib.gcnk_lda_bound_docs_f64(ip.data_ptr(), ix.data_ptr(), ct.data_ptr(), 0, B, V, K, table.data_ptr(),
                                           table.stride(0), gamma.data_ptr(), K, c["alpha"], g_doc.data_ptr(), stream), "docs")
    lam = tb.components
    _lib.check(lib.gcnk_lda_bound_topics_f64(lam.data_ptr(), lam.stride(0), K, V, c["eta"], g_topic.data_ptr(), stream), "topics")
    _lib.check(lib.gcnk_lda_bound_finish_f64(g_doc.data_ptr(), B, g_topic.data_ptr(), K, ip.data_ptr(), ct.data_ptr(), 0,
                                             1.0, g_out.data_ptr(), stream), "finish")
    assert torch.equal(_bits(g_doc[:B]), _bits(doc)) and torch.equal(_bits(g_topic[:K]), _bits(topic))
    assert torch.equal(_bits(g_out[:3]), _bits(want))
    assert all(float(t[n:].min()) == GUARD == float(t[n:].max()) for t, n in ((g_doc, B), (g_topic, K), (g_out, 3)))


def test_topic_term_is_cached_under_the_derived_rule(z):
    lam = _dev(z["components_"])
    tb = TopicBound(lam, 0.125, 0.125)
    first = tb.topic_bound()
    assert tb.topic_bound() is first
    before = first.clone()
    lam.mul_(1.5)                                            # an in-place change: rebuilt on the next use
    second = tb.topic_bound()
    assert second is not first and not torch.equal(second, before)
    assert torch.equal(_bits(second), _bits(topic_bound.topic_terms(lam, 0.125)))


def test_constructors_scorers_and_refusals(z, scorer):
    docs = _docs(z, "held_")
    lda = type("Lda", (), dict(components_=z["components_"], doc_topic_prior_=float(z["doc_topic_prior_"]),
                               topic_word_prior_=float(z["topic_word_prior_"]), mean_change_tol=float(z["mean_change_tol"]),
                               max_doc_update_iter=int(z["max_doc_update_iter"])))()
    assert torch.equal(_bits(TopicBound.from_sklearn(lda, DEV).score(*docs)), _bits(scorer.score(*docs)))
    ot = OnlineTopics(int(z["V"]), num_topics=8, total_samples=260, init_components=_dev(z["components_"]), device=DEV)
    sc = ot.scorer()
    assert sc.components.data_ptr() != ot.components.data_ptr() and torch.equal(sc.components, ot.components)
    before = sc.perplexity(*docs)
    assert torch.equal(_bits(before), _bits(scorer.perplexity(*docs)))
    ot.partial_fit(*docs)
    assert torch.equal(_bits(sc.perplexity(*docs)), _bits(before))      # a copy: the model moved, the scorer did not
    assert float(ot.scorer().perplexity(*docs)) < float(before)         # ... and the documents it saw fit better now
    gamma = _dev(z["held_gamma"])
    for bad in (gamma[:, :-1], gamma[:-1], gamma.to(torch.float32), gamma.cpu(), None):
        with pytest.raises(RuntimeError):
            scorer.bound(*docs, bad)
    with pytest.raises(RuntimeError, match="total_samples"):
        scorer.perplexity(*docs, sub_sampling=True)
    with pytest.raises(RuntimeError, match="float32 E-step"):
        scorer.score(docs[0], docs[1], docs[2].to(torch.float32))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        scorer.score(docs[0].cpu(), docs[1], docs[2])
    with pytest.raises(RuntimeError):
        TopicBound(_dev(z["components_"]).to(torch.float32), 0.125, 0.125)
