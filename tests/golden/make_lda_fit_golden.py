"""Generate tests/golden/lda_fit_r8_small.npz by running the REFERENCE's topic model fit.

Test infrastructure only, CPU only.  Imports ``TopicModel`` from ``$GCN_REFERENCE`` (default
``/root/reference``) at run time; nothing of the reference is copied: the file holds numbers.

  topic_model.py:74-131    TopicModel(num_topics=8, max_iter=3).fit(first 200 R8 clean-corpus documents)

Stored: the document-term matrix the reference's CountVectorizer gives (indptr / indices int32, counts
int64, V), the reference's components_ (lambda, [8 x V] float64) and its row-normalised
topic_word_distribution, doc_topic_prior_, topic_word_prior_, mean_change_tol, max_doc_update_iter,
random_state; lambda0 and the three gamma0 draws of RandomState(42) in sklearn's order; the update counts
of tests/lda_ref.py's restatement per EM iteration (int32 [3 x 200]) and its smallest stop margin; and
two measured distances of the restatement's lambda (max relative):
  d_ref   to the reference's components_;
  d_perm  to the restatement run with every document's words randomly permuted (a pure reorder of sums).

Usage:  python tests/golden/make_lda_fit_golden.py
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GCN_REFERENCE", "/root/reference")
NTOPIC, MAX_ITER, NFIT, SEED = 8, 3, 200, 42


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    import lda_ref as lda_fit_ref
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet), contextlib.redirect_stderr(quiet):
        import topic_model
        docs = topic_model.load_documents_from_file(os.path.join(REF, "data", "text_dataset", "clean_corpus", "R8.txt"))
        tm = topic_model.TopicModel(num_topics=NTOPIC, max_iter=MAX_ITER, random_state=SEED)
        tm.fit(docs[:NFIT])
    X = tm.vectorizer.transform(docs[:NFIT]).tocsr()
    assert X.has_sorted_indices and X.dtype == np.int64
    lda = tm.lda_model
    B, V = X.shape
    indptr, indices, counts = X.indptr.astype(np.int32), X.indices.astype(np.int32), X.data.astype(np.int64)
    alpha, eta = float(lda.doc_topic_prior_), float(lda.topic_word_prior_)
    tol, cap = float(lda.mean_change_tol), int(lda.max_doc_update_iter)
    lam0, g0s = lda_fit_ref.draws(SEED, NTOPIC, V, B, MAX_ITER)
    lam, iters, margin = lda_fit_ref.fit(indptr, indices, counts, lam0, g0s, alpha, eta, tol, cap)
    pi, pc = lda_fit_ref.permuted(indptr, indices, counts)
    lam_p, iters_p, _ = lda_fit_ref.fit(indptr, pi, pc, lam0, g0s, alpha, eta, tol, cap)
    assert np.array_equal(iters, iters_p), "a reorder changed an update count: the fixture would not be a fair test"
    d_ref = lda_fit_ref.max_rel(lam, lda.components_)
    d_perm = lda_fit_ref.max_rel(lam, lam_p)
    out = os.path.join(HERE, "lda_fit_r8_small.npz")
    np.savez_compressed(
        out, indptr=indptr, indices=indices, counts=counts, V=np.int64(V),
        components_=lda.components_.astype(np.float64), topic_word_distribution=tm.topic_word_distribution,
        doc_topic_prior_=np.float64(alpha), topic_word_prior_=np.float64(eta), mean_change_tol=np.float64(tol),
        max_doc_update_iter=np.int64(cap), random_state=np.int64(SEED), lambda0=lam0, gamma0=g0s,
        iterations=iters, stop_margin=np.float64(margin), d_ref=np.float64(d_ref), d_perm=np.float64(d_perm))
    print(f"wrote {out}: B={B} V={V} nnz={X.nnz} d_ref={d_ref:.3e} d_perm={d_perm:.3e} margin={margin:.3e} "
          f"cap reached in EM iterations {[int(i) for i in np.flatnonzero((iters == cap).any(1))]} "
          f"({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
