"""Generate tests/golden/lda_r8_small.npz by running the REFERENCE's topic model.

Test infrastructure only, CPU only.  Imports ``TopicModel`` from ``$GCN_REFERENCE`` (default
``/root/reference``) at run time; nothing of the reference is copied: the file holds numbers.

  topic_model.py:74-131    TopicModel(num_topics=16, max_iter=5).fit(first 600 R8 clean-corpus documents)
  topic_model.py:133-164   get_document_topic_distribution(documents 600 .. 855)  -> theta

Stored: components_ (lambda, [16 x V] float64), exp_dirichlet_component_, doc_topic_prior_,
mean_change_tol, max_doc_update_iter, the 256 held-out documents as the CSR the reference's
CountVectorizer gives (indptr / indices int32, counts int64) and the reference's theta.

Usage:  python tests/golden/make_lda_golden.py
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GCN_REFERENCE", "/root/reference")
NTOPIC, MAX_ITER, NFIT, NHELD = 16, 5, 600, 256


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import numpy as np
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet), contextlib.redirect_stderr(quiet):
        import topic_model
        docs = topic_model.load_documents_from_file(os.path.join(REF, "data", "text_dataset", "clean_corpus", "R8.txt"))
        tm = topic_model.TopicModel(num_topics=NTOPIC, max_iter=MAX_ITER)
        tm.fit(docs[:NFIT])
        held = docs[NFIT:NFIT + NHELD]
        theta = tm.get_document_topic_distribution(held)
    X = tm.vectorizer.transform(held).tocsr()
    X.sort_indices()
    lda = tm.lda_model
    assert X.dtype == np.int64 and theta.dtype == np.float64 and theta.shape == (NHELD, NTOPIC)
    out = os.path.join(HERE, "lda_r8_small.npz")
    np.savez_compressed(
        out, components_=lda.components_.astype(np.float64), exp_dirichlet_component_=lda.exp_dirichlet_component_,
        doc_topic_prior_=np.float64(lda.doc_topic_prior_), mean_change_tol=np.float64(lda.mean_change_tol),
        max_doc_update_iter=np.int64(lda.max_doc_update_iter), indptr=X.indptr.astype(np.int32),
        indices=X.indices.astype(np.int32), counts=X.data.astype(np.int64), theta=theta)
    print(f"wrote {out}: V={X.shape[1]} nnz={X.nnz} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
