"""The variational bound's entry points without a GPU: gcnk_lda_bound_{docs,topics,finish}_f64 declared in
include/gcnk_lda.h (which include/gcnk.h includes), exported and bound within ABI 13, every refusal before any
HIP call with its reason in gcnk_last_error, the public names, and the Python refusals that need no device."""
import ctypes

import pytest
import torch

import gcn_amd
from graph_convolutional_networks_for_text_classification_amd import TopicBound, _lib, fit_topics, topic_bound, topic_fit

import abi_bound
import lda_abi
from lda_abi import PTR, _even_K, _K, _V, kernels_source

DOCS, TOPICS, FINISH = "gcnk_lda_bound_docs_f64", "gcnk_lda_bound_topics_f64", "gcnk_lda_bound_finish_f64"
NAMES = {"gcnk_lda_bound_topic_chunk": 0, DOCS: 14, TOPICS: 7, FINISH: 10}   # argument counts, the stream included
# entry point -> its operands in the declaration's order as (keyword, default), lda_abi.ENTRY's form
ENTRY = {
    DOCS: (("indptr", PTR), ("indices", PTR), ("counts", PTR), ("kind", 0), ("B", 8), ("V", 100), ("K", 16),
           ("table", PTR), ("ldt", _even_K), ("gamma", PTR), ("ldg", _K), ("alpha", 0.1), ("doc_bound", PTR)),
    TOPICS: (("lam", PTR), ("ldl", _V), ("K", 16), ("V", 100), ("eta", 0.1), ("topic_bound", PTR)),
    FINISH: (("doc_bound", PTR), ("B", 8), ("topic_bound", PTR), ("K", 16), ("indptr", PTR), ("counts", PTR), ("kind", 0),
             ("doc_ratio", 1.0), ("out", PTR)),
}


def call(name, **kw):
    return lda_abi.call(name, ENTRY, **kw)


def _ids(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


def test_symbols_declared_exported_and_bound():
    text = abi_bound.header("gcnk_lda.h")[0]
    assert '#include "gcnk_lda.h"' in abi_bound.header("gcnk.h")[1]        # a C caller of gcnk.h sees them
    assert set(NAMES) <= abi_bound.declared_names("gcnk_lda.h")   # (test_lda_abi.py: the four files' are all of it)
    lda_abi.assert_declared_exported_bound({k: v for k, v in NAMES.items() if v == 0}, ENTRY, ctypes.c_int32)
    lda_abi.assert_declared_exported_bound({k: v for k, v in NAMES.items() if v != 0}, ENTRY, ctypes.c_int)
    assert "within ABI 13" in text and "_approx_bound" in text
    kernels = kernels_source()
    assert all(name in kernels for name in NAMES)


def test_constants_and_public_names():
    lib = _lib.load()
    assert lib.gcnk_lda_bound_topic_chunk() == topic_bound.TOPIC_CHUNK == 256
    assert gcn_amd.TopicBound is TopicBound is topic_bound.TopicBound and gcn_amd.topic_bound is topic_bound
    assert {"TopicBound", "topic_bound"} <= set(gcn_amd.__all__)
    assert callable(topic_fit.TopicFit.scorer) and callable(topic_fit.OnlineTopics.scorer)
    assert {"bound", "perplexities"} <= set(topic_fit.TopicFit.__slots__)
    # what the fit still does not restate: n_jobs and float32 input alone
    rest = topic_fit.__doc__[topic_fit.__doc__.index("Still not restated"):]
    assert "n_jobs" in rest and "float32" in rest
    assert "bound_" not in rest and "evaluate_every" not in rest and "perplexity" not in rest
    assert "underflow" in topic_bound.__doc__            # the limit of the shifted logsumexp is documented


@pytest.mark.parametrize("kw", [dict(B=0), dict(K=0), dict(K=-1), dict(V=0), dict(indptr=None), dict(indices=None),
                                dict(counts=None), dict(table=None), dict(table=PTR + 8), dict(ldt=15), dict(ldt=17),
                                dict(kind=3), dict(kind=-1), dict(gamma=None), dict(doc_bound=None), dict(ldg=15)],
                         ids=_ids)
def test_docs_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = call(DOCS, **kw)
    assert rc == _lib.EARG and DOCS in msg


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=-1), dict(V=0), dict(lam=None), dict(topic_bound=None), dict(ldl=99)],
                         ids=_ids)
def test_topics_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = call(TOPICS, **kw)
    assert rc == _lib.EARG and TOPICS in msg


@pytest.mark.parametrize("kw", [dict(B=0), dict(K=0), dict(doc_bound=None), dict(topic_bound=None), dict(indptr=None),
                                dict(counts=None), dict(out=None), dict(kind=3), dict(kind=-1), dict(doc_ratio=0.0),
                                dict(doc_ratio=-1.0), dict(doc_ratio=float("inf")), dict(doc_ratio=float("nan"))],
                         ids=_ids)
def test_finish_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = call(FINISH, **kw)
    assert rc == _lib.EARG and FINISH in msg


def test_unsupported_sizes_are_refused_before_any_hip_call():
    for who in (DOCS, TOPICS, FINISH):
        rc, msg = call(who, K=129)
        assert rc == _lib.EUNSUP and who in msg and "128" in msg
    rc, msg = call(DOCS, K=128, V=1 << 21)      # 2^21 rows of 1 KiB: past the buffer resource's 32-bit offsets
    assert rc == _lib.EUNSUP and DOCS in msg and "32-bit" in msg


def test_python_refusals_that_need_no_device():
    lam = torch.ones((4, 10), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm GPU"):      # never a host fallback
        TopicBound(lam, 0.25, 0.25)
    with pytest.raises(RuntimeError, match="float64"):
        TopicBound.from_sklearn(type("Lda", (), dict(components_=lam.to(torch.float32).numpy(), doc_topic_prior_=0.25,
                                                     topic_word_prior_=0.25, mean_change_tol=1e-3,
                                                     max_doc_update_iter=100))(), "cpu")
    for bad in (None, 0.0, -3.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="total_samples"):
            topic_bound.doc_ratio_of("TopicBound", 5, True, bad)
    assert topic_bound.doc_ratio_of("TopicBound", 5, False, None) == 1.0
    assert topic_bound.doc_ratio_of("TopicBound", 5, True, 40) == 8.0
    ip, ix = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([1, 5], dtype=torch.int32)
    ct = torch.ones(2, dtype=torch.float64)
    for bad in (-0.1, float("nan")):
        with pytest.raises(RuntimeError, match="perp_tol"):
            fit_topics(ip, ix, ct, 10, num_topics=4, evaluate_every=1, perp_tol=bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        fit_topics(ip, ix, ct, 10, num_topics=4, evaluate_every=1, compute_bound=True)
