"""Generate tests/golden/lda_bound_r8_small.npz by running the REFERENCE's topic model and sklearn's own
bound, score and perplexity on it.

Test infrastructure only, CPU only.  Imports ``TopicModel`` from ``$GCN_REFERENCE`` (default
``/root/reference``) at run time; nothing of the reference is copied: the file holds numbers.

  topic_model.py:74-131    TopicModel(num_topics=8, max_iter=3).fit(first 200 R8 clean-corpus documents)

Stored: the training documents' and 60 held-out documents' (200..259) document-term matrices as the reference's
CountVectorizer gives them, the reference's components_ and priors; sklearn's bound_, score and perplexity of the
training documents, score and perplexity of the held-out ones with their gamma (_unnormalized_transform); and,
from the draws of RandomState(42) in sklearn's order (lambda0, gamma0 [12 x 200 x 8]), sklearn fits with
evaluate_every=2, max_iter=12 by both learning methods: perp_tol, n_iter_, bound_, n_batch_iter_ and the
perplexities tests/lda_bound_ref.py's restatement of that loop evaluates.  perp_tol is the geometric mean of two
consecutive |change of the perplexity|, so that the stop falls between two evaluations and is no rounding
matter (asserted: every change is at least 1e-6 of the perplexity away from it).

Distances, each |x - y| / (2^-52 A) with A the sum of the absolute addends (lda_bound_ref.py), a scalar for the
bound (``*_total``) and the maximum over documents and topics for the partials (``*_parts``):
  d_ref   the restatement against sklearn (the partials against the same formulas evaluated with sklearn's own
          _dirichlet_expectation_2d, scipy's logsumexp and gammaln and numpy's sums);
  d_perm  against the restatement with the vocabulary renumbered and every document's words reordered, the
          maximum over 8 seeds;
  d_fn    against the restatement with math.lgamma and a hand-written max-shift logsumexp in scipy's place: what
          two independent correct libraries differ by, which is what the device's lgamma / log / exp are.

Usage:  python tests/golden/make_lda_bound_golden.py
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GCN_REFERENCE", "/root/reference")
NTOPIC, MAX_ITER, NFIT, NHELD, SEED = 8, 3, 200, 60, 42
EVERY, EE_MAX_ITER, NSEEDS = 2, 12, 8


def check_perp_tol(perps, perp_tol, max_iter=EE_MAX_ITER, every=EVERY):
    """The stop that ``perp_tol`` gives on the evaluated perplexities falls after the first evaluation and before
    max_iter, and no change is within 1e-6 of the perplexity of it -> the n_iter_ it stops at."""
    import numpy as np
    perps = np.asarray(perps, np.float64)
    change = np.abs(np.diff(perps))
    assert change.size >= 1 and change[-1] < perp_tol and (change[:-1] >= perp_tol).all(), (change, perp_tol)
    assert (np.abs(change - perp_tol) >= 1e-6 * perps[1:]).all(), (change, perp_tol)
    n_iter = every * len(perps) - 1      # (the stopping iteration is not counted)
    assert every < n_iter + 1 < max_iter, n_iter
    return n_iter


def sklearn_parts(X, gamma, lam, alpha, eta):
    """doc_d and topic_k by _approx_bound's formulas in sklearn's own arithmetic."""
    import numpy as np
    from scipy.special import gammaln, logsumexp
    from sklearn.decomposition._online_lda_fast import _dirichlet_expectation_2d
    el_theta, el_beta = _dirichlet_expectation_2d(gamma), _dirichlet_expectation_2d(lam)
    K, V = lam.shape
    doc = np.zeros(X.shape[0])
    for d in range(X.shape[0]):
        ids, cnts = X.indices[X.indptr[d]:X.indptr[d + 1]], X.data[X.indptr[d]:X.indptr[d + 1]]
        doc[d] = np.dot(cnts, logsumexp(el_theta[d, :, None] + el_beta[:, ids], axis=0)) if len(ids) else 0.0
        doc[d] += np.sum((alpha - gamma[d]) * el_theta[d]) + np.sum(gammaln(gamma[d]) - gammaln(alpha))
        doc[d] += gammaln(alpha * K) - gammaln(np.sum(gamma[d]))
    topic = np.sum((eta - lam) * el_beta, axis=1) + np.sum(gammaln(lam) - gammaln(eta), axis=1)
    topic += gammaln(eta * V) - gammaln(np.sum(lam, axis=1))
    return doc, topic


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    import lda_bound_ref as R
    import lda_ref
    from sklearn.base import clone
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet), contextlib.redirect_stderr(quiet):
        import topic_model
        docs = topic_model.load_documents_from_file(os.path.join(REF, "data", "text_dataset", "clean_corpus", "R8.txt"))
        tm = topic_model.TopicModel(num_topics=NTOPIC, max_iter=MAX_ITER, random_state=SEED)
        tm.fit(docs[:NFIT])
    X = tm.vectorizer.transform(docs[:NFIT]).tocsr()
    H = tm.vectorizer.transform(docs[NFIT:NFIT + NHELD]).tocsr()
    assert X.has_sorted_indices and X.dtype == np.int64 and H.dtype == np.int64
    lda = tm.lda_model
    B, V = X.shape
    lam = lda.components_.astype(np.float64)
    alpha, eta = float(lda.doc_topic_prior_), float(lda.topic_word_prior_)
    tol, cap = float(lda.mean_change_tol), int(lda.max_doc_update_iter)
    csr = lambda M: (M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.int64))   # noqa: E731
    train, held = csr(X), csr(H)

    out = dict(V=np.int64(V), components_=lam, doc_topic_prior_=np.float64(alpha), topic_word_prior_=np.float64(eta),
               mean_change_tol=np.float64(tol), max_doc_update_iter=np.int64(cap), random_state=np.int64(SEED),
               bound_=np.float64(lda.bound_))
    d = {"d_ref_parts": 0.0, "d_ref_total": 0.0, "d_perm_parts": 0.0, "d_perm_total": 0.0, "d_fn_parts": 0.0,
         "d_fn_total": 0.0}

    def worse(key, parts, total):
        d[key + "_parts"], d[key + "_total"] = max(d[key + "_parts"], parts), max(d[key + "_total"], total)

    for name, M, arrays in (("train", X, train), ("held", H, held)):
        gamma = lda._unnormalized_transform(M.astype(np.float64))    # (its callers validate X to float64)
        sk_score, sk_perp = float(lda.score(M)), float(lda.perplexity(M))
        ours = R.evaluate(*arrays, gamma, lam, alpha, eta)
        sk_doc, sk_topic = sklearn_parts(M, gamma, lam, alpha, eta)
        worse("d_ref", max(R.distance(ours["doc"], sk_doc, ours["A_doc"]), R.distance(ours["topic"], sk_topic, ours["A_topic"])),
              R.distance(ours["bound"], sk_score, ours["A"]))
        # the restatement's own gamma (its E-step) against sklearn's: the score as a user calls it
        own = R.score(*arrays, lam, alpha, eta, tol, cap)
        worse("d_ref", 0.0, R.distance(own["bound"], sk_score, own["A"]))
        worse("d_fn", *R.distances(ours, R.evaluate(*arrays, gamma, lam, alpha, eta, fn=R.LIBM)))
        for seed in range(NSEEDS):
            ix, ct, lam2 = R.relabelled(*arrays, lam, seed)
            other = R.evaluate(arrays[0], ix, ct, gamma, lam2, alpha, eta)
            worse("d_perm", *R.distances(ours, other))
        for k, a in zip(("indptr", "indices", "counts"), arrays):
            out[f"{name}_{k}"] = a
        out[f"{name}_score"], out[f"{name}_perplexity"] = np.float64(sk_score), np.float64(sk_perp)
        out[f"{name}_A"] = np.float64(ours["A"])
        if name == "held":
            out["held_gamma"] = gamma
    assert abs(float(lda.bound_) - float(out["train_perplexity"])) <= 1e-9 * float(lda.bound_)

    lam0, g0s = lda_ref.draws(SEED, NTOPIC, V, B, EE_MAX_ITER)
    out["lambda0"], out["gamma0"] = lam0, g0s
    for method in ("batch", "online"):
        _, _, perps, _, _ = R.evaluate_every(*train, lam0, g0s, alpha, eta, EVERY, 0.0, method, tol=tol, cap=cap)
        change = np.abs(np.diff(perps))
        assert len(perps) == EE_MAX_ITER // EVERY and (np.diff(change) < 0).all(), (method, perps)
        j = 1                                              # between the second and the third change
        perp_tol = float(np.sqrt(change[j] * change[j + 1]))
        _, n_iter, seq, closing, n_batch = R.evaluate_every(*train, lam0, g0s, alpha, eta, EVERY, perp_tol, method,
                                                            tol=tol, cap=cap)
        assert check_perp_tol(seq, perp_tol) == n_iter and np.array_equal(seq, perps[:len(seq)])
        sk = clone(lda).set_params(max_iter=EE_MAX_ITER, evaluate_every=EVERY, perp_tol=perp_tol, verbose=0,
                                   learning_method=method).fit(X)
        assert sk.n_iter_ == n_iter and sk.n_batch_iter_ == n_batch, (method, sk.n_iter_, n_iter, sk.n_batch_iter_)
        assert abs(sk.bound_ - closing) <= 1e-9 * closing, (method, sk.bound_, closing)
        out[f"ee_{method}_perp_tol"], out[f"ee_{method}_n_iter"] = np.float64(perp_tol), np.int64(sk.n_iter_)
        out[f"ee_{method}_bound_"], out[f"ee_{method}_n_batch_iter"] = np.float64(sk.bound_), np.int64(sk.n_batch_iter_)
        out[f"ee_{method}_perplexities"] = seq
        print(f"{method}: perplexities {perps.tolist()} perp_tol {perp_tol:.6g} -> n_iter_ {sk.n_iter_} bound_ {sk.bound_!r}")

    out.update({k: np.float64(v) for k, v in d.items()})
    path = os.path.join(HERE, "lda_bound_r8_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: B={B} held={H.shape[0]} V={V} bound_={float(lda.bound_)!r} train score {float(out['train_score'])!r} "
          f"held score {float(out['held_score'])!r} perplexity {float(out['held_perplexity'])!r} A={float(out['train_A']):.3e}\n"
          + " ".join(f"{k}={v:.3f}" for k, v in d.items()) + f" ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
