"""Generate tests/golden/lda_online_r8_small.npz by running the REFERENCE's topic model fit with
learning_method='online', and sklearn's online fit and partial_fit on the same matrix.

Test infrastructure only, CPU only.  Imports ``TopicModel`` from ``$GCN_REFERENCE`` (default
``/root/reference``) at run time; nothing of the reference is copied: the file holds numbers.

The documents are lda_fit_r8_small.npz's (the first 200 R8 clean-corpus documents, K = 8, seed 42); the
document-term matrix, lambda0 and the gamma0 stream are read from that file and not stored twice (the reference's
own vectoriser is asserted to give the same matrix).  Three runs, keys prefixed a_, b_, c_:

  a  topic_model.py:74-131   TopicModel(num_topics=8, max_iter=3, learning_method='online').fit(documents)
                             (sklearn's default batch_size 128: minibatches of 128 and 72)
  b  sklearn directly        LatentDirichletAllocation(8, learning_method='online', batch_size=64, max_iter=3,
                             random_state=42).fit(X)   (minibatches 64, 64, 64, 8)
  c  sklearn's partial_fit   (..., total_samples=1000, batch_size=64): partial_fit(X); partial_fit(X[:70])

For each: components_ [8 x V] float64 and n_batch_iter_; the update counts of tests/lda_ref.py's
restatement (int32 [3 x 200] for a and b, [270] for c: the two calls one after the other) and its smallest stop
margin; and two measured distances of the restatement's lambda (max relative):
  d_ref   to components_;
  d_perm  to the restatement run with every document's words randomly permuted (a pure reorder of sums).
a_topic_word_distribution is the reference's row-normalised lambda; c_gamma0 [270 x 8] is RandomState(42)'s stream
after lambda0: the (200, 8) draw of the first call, then the (70, 8) draw of the second.

Usage:  python tests/golden/make_lda_online_golden.py
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GCN_REFERENCE", "/root/reference")
NTOPIC, MAX_ITER, NFIT, SEED = 8, 3, 200, 42
C_TOTAL, C_BATCH, C_SECOND = 1000, 64, 70


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # (lda_cases imports the package)
    import numpy as np
    import scipy.sparse as sp
    from sklearn.decomposition import LatentDirichletAllocation
    import lda_cases
    import lda_ref as lda_fit_ref
    import lda_ref as ref
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet), contextlib.redirect_stderr(quiet):
        import topic_model
        docs = topic_model.load_documents_from_file(os.path.join(REF, "data", "text_dataset", "clean_corpus", "R8.txt"))
        tm = topic_model.TopicModel(num_topics=NTOPIC, max_iter=MAX_ITER, random_state=SEED, learning_method="online")
        tm.fit(docs[:NFIT])
    z = lda_fit_ref.load_fit_golden()
    X = tm.vectorizer.transform(docs[:NFIT]).tocsr()
    indptr, indices, counts = z["indptr"], z["indices"], z["counts"]
    assert X.has_sorted_indices and np.array_equal(X.indptr, indptr) and np.array_equal(X.indices, indices)
    assert np.array_equal(X.data, counts), "the batch fixture holds another matrix"
    B, V = X.shape
    lda_a = tm.lda_model
    alpha, eta = float(lda_a.doc_topic_prior_), float(lda_a.topic_word_prior_)
    tol, cap = float(lda_a.mean_change_tol), int(lda_a.max_doc_update_iter)
    assert (alpha, eta, tol, cap) == (float(z["doc_topic_prior_"]), float(z["topic_word_prior_"]),
                                      float(z["mean_change_tol"]), int(z["max_doc_update_iter"]))
    assert lda_a.batch_size == 128 and lda_a.learning_decay == 0.7 and lda_a.learning_offset == 10.0
    lam0, g0s = z["lambda0"], z["gamma0"]
    pi, pc = lda_fit_ref.permuted(indptr, indices, counts)

    with contextlib.redirect_stdout(quiet), contextlib.redirect_stderr(quiet):
        lda_b = LatentDirichletAllocation(n_components=NTOPIC, random_state=SEED, max_iter=MAX_ITER,
                                          learning_method="online", batch_size=64).fit(X)
        lda_c = LatentDirichletAllocation(n_components=NTOPIC, random_state=SEED, learning_method="online",
                                          batch_size=C_BATCH, total_samples=C_TOTAL)
        lda_c.partial_fit(X)
        lda_c.partial_fit(X[:C_SECOND])

    out, report = {}, []

    def record(key, lda, run):
        lam, iters, margin, n = run(indices, counts)
        lam_p, iters_p, _, _ = run(pi, pc)
        assert np.array_equal(iters, iters_p), f"{key}: a reorder changed an update count: the fixture would not be a fair test"
        assert margin >= lda_cases.MIN_MARGIN, (key, margin)
        assert n == lda.n_batch_iter_, (key, n, lda.n_batch_iter_)
        d_ref, d_perm = lda_fit_ref.max_rel(lam, lda.components_), lda_fit_ref.max_rel(lam, lam_p)
        out.update({f"{key}_components_": lda.components_.astype(np.float64), f"{key}_n_batch_iter_": np.int64(n),
                    f"{key}_iterations": iters.astype(np.int32), f"{key}_stop_margin": np.float64(margin),
                    f"{key}_d_ref": np.float64(d_ref), f"{key}_d_perm": np.float64(d_perm)})
        report.append(f"  {key}: n_batch_iter_={n} d_ref={d_ref:.3e} d_perm={d_perm:.3e} margin={margin:.3e} "
                      f"documents at the cap {int((iters == cap).sum())}")

    def fit_of(batch_size):
        return lambda ix, ct: ref.fit_online(indptr, ix, ct, lam0, g0s, alpha, eta, batch_size, 0.7, 10.0, tol, cap)

    rs = np.random.RandomState(SEED)
    assert np.array_equal(rs.gamma(100.0, 0.01, (NTOPIC, V)), lam0)
    c_gamma0 = np.concatenate([rs.gamma(100.0, 0.01, (B, NTOPIC)), rs.gamma(100.0, 0.01, (C_SECOND, NTOPIC))])
    hi = int(indptr[C_SECOND])

    def two_calls(ix, ct):
        lam, i1, m1, n = ref.partial_fit(indptr, ix, ct, lam0, c_gamma0[:B], alpha, eta, C_TOTAL, 1, C_BATCH, 0.7, 10.0,
                                         tol, cap)
        lam, i2, m2, n = ref.partial_fit(indptr[:C_SECOND + 1], ix[:hi], ct[:hi], lam, c_gamma0[B:], alpha, eta, C_TOTAL,
                                         n, C_BATCH, 0.7, 10.0, tol, cap)
        return lam, np.concatenate([i1, i2]), min(m1, m2), n

    record("a", lda_a, fit_of(128))
    record("b", lda_b, fit_of(64))
    record("c", lda_c, two_calls)
    out["a_topic_word_distribution"] = tm.topic_word_distribution
    out["c_gamma0"] = c_gamma0
    out["c_total_samples"], out["c_batch_size"], out["c_second"] = np.int64(C_TOTAL), np.int64(C_BATCH), np.int64(C_SECOND)
    path = os.path.join(HERE, "lda_online_r8_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: B={B} V={V} nnz={X.nnz} ({os.path.getsize(path)} bytes)")
    print("\n".join(report))


if __name__ == "__main__":
    main()
