"""Generate tests/golden/text_r8_small.npz by running the REFERENCE's vectoriser: sklearn's CountVectorizer as
topic_model.py:93-102 configures it, fitted by TopicModel.fit, and its transform (topic_model.py:159).

Test infrastructure only, CPU only.  Imports ``TopicModel`` from ``$GCN_REFERENCE`` (default
``/root/reference``) at run time; nothing of the reference is copied: the file holds the corpus' first documents
as bytes and numbers.

Stored: the first 300 documents of the R8 clean corpus as a UTF-8 byte blob with offsets (``text_bytes``,
``text_offsets``), the vocabulary the reference's vectoriser fits on the first 200 as a blob with offsets in id
order (``vocab_bytes``, ``vocab_offsets``), and ``vectorizer.transform`` of all 300 (``indptr``, ``indices``,
``data`` as sklearn gives them: int32, int32, int64, indices ascending in a row).  The last 100 documents are unseen
text: they hold words the vocabulary lacks.  tests/text_ref.py's restatement is asserted equal before the file is
written.

Usage:  python tests/golden/make_text_golden.py
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GCN_REFERENCE", "/root/reference")
NFIT, NDOC = 200, 300


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    import text_ref as R
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet), contextlib.redirect_stderr(quiet):
        import topic_model
        docs = topic_model.load_documents_from_file(os.path.join(REF, "data", "text_dataset", "clean_corpus", "R8.txt"))
        tm = topic_model.TopicModel(num_topics=2, max_iter=1, random_state=0)
        tm.fit(docs[:NFIT])
    vec = tm.vectorizer
    assert vec.token_pattern == r"\S+" and vec.lowercase is False and vec.ngram_range == (1, 1) and not vec.binary
    texts = [d if isinstance(d, str) else " ".join(d) for d in docs[:NDOC]]
    X = vec.transform(texts).tocsr()
    assert X.has_sorted_indices and X.shape[0] == NDOC
    words = [None] * len(vec.vocabulary_)
    for w, i in vec.vocabulary_.items():
        words[int(i)] = w
    assert all(w is not None for w in words) and list(vec.get_feature_names_out()) == words

    data, offsets = R.encode(texts)
    ours = R.count(data, offsets, R.vocabulary_of(words))
    assert np.array_equal(ours[0], X.indptr) and np.array_equal(ours[1], X.indices) and np.array_equal(ours[2], X.data)
    unseen = sum(tok not in R.vocabulary_of(words) for d in range(NFIT, NDOC)
                 for tok in R.tokens(data[offsets[d]:offsets[d + 1]]))
    assert unseen > 0
    enc = [w.encode("utf-8") for w in words]
    out = dict(text_bytes=np.frombuffer(data, np.uint8), text_offsets=offsets,
               vocab_bytes=np.frombuffer(b"".join(enc), np.uint8),
               vocab_offsets=np.concatenate([[0], np.cumsum([len(b) for b in enc])]).astype(np.int64),
               indptr=X.indptr.astype(np.int32), indices=X.indices.astype(np.int32), data=X.data.astype(np.int64))
    path = os.path.join(HERE, "text_r8_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {NDOC} documents, {len(data)} bytes, V={len(words)}, nnz={X.nnz}, "
          f"{int(X.data.sum())} counted tokens, {unseen} tokens of the last {NDOC - NFIT} outside the vocabulary "
          f"({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
