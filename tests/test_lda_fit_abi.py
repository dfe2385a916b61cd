"""The LDA fit's entry points without a GPU: gcnk_lda_estep_fit_f64 and gcnk_lda_mstep_f64 declared, exported
and bound within ABI 13, every refusal of both before any HIP call with its reason in gcnk_last_error, and
the public names."""
import pytest
import torch

import gcn_amd
from graph_convolutional_networks_for_text_classification_amd import TopicFit, _lib, fit_topics, topic_fit, topic_infer

from lda_abi import PTR, assert_declared_exported_bound, call, header, kernels_source

NAMES = {"gcnk_lda_words_per_block": 0, "gcnk_lda_estep_fit_f64": 22, "gcnk_lda_mstep_f64": 16}
ESTEP, MSTEP = "gcnk_lda_estep_fit_f64", "gcnk_lda_mstep_f64"


def _estep(**kw):
    return call(ESTEP, **kw)


def _mstep(**kw):
    return call(MSTEP, **kw)


def test_symbols_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    assert len(_lib.SIGNATURES["gcnk_lda_estep_f64"][1]) == 22   # the transform's entry point keeps its signature
    assert "topic_model.py:74-131" in header()[0]
    kernels = kernels_source()
    assert MSTEP in kernels and ESTEP in kernels


def test_constants_and_public_names():
    lib = _lib.load()
    assert lib.gcnk_lda_words_per_block() == topic_fit.WORDS_PER_BLOCK >= 1
    assert gcn_amd.fit_topics is fit_topics is topic_fit.fit_topics and gcn_amd.TopicFit is TopicFit
    assert gcn_amd.topic_fit is topic_fit
    assert {"fit_topics", "TopicFit", "topic_fit"} <= set(gcn_amd.__all__)
    for what in ("bound_", "online", "evaluate_every", "n_jobs", "float32"):   # what the fit does not restate
        assert what in topic_fit.__doc__


@pytest.mark.parametrize("kw", [dict(B=0), dict(K=0), dict(K=-1), dict(V=0), dict(indptr=None), dict(indices=None),
                                dict(counts=None), dict(table=None), dict(table=PTR + 8), dict(ldt=15), dict(ldt=17),
                                dict(kind=3), dict(kind=-1), dict(max_iter=-1), dict(max_iter=10001),
                                dict(gamma0=None), dict(ratio=None), dict(etheta=None), dict(ldg0=15), dict(lde=15),
                                dict(gamma=PTR, ldg=15), dict(nnz=-1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_estep_fit_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = _estep(**kw)
    assert rc == _lib.EARG and ESTEP in msg


@pytest.mark.parametrize("kw", [dict(B=0), dict(K=0), dict(V=0), dict(wptr=None), dict(pos=None), dict(doc=None),
                                dict(ratio=None), dict(etheta=None), dict(lam=None), dict(table=None),
                                dict(table=PTR + 8), dict(ldt=15), dict(ldt=17), dict(lde=15), dict(ldl=99),
                                dict(nnz=-1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_mstep_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = _mstep(**kw)
    assert rc == _lib.EARG and MSTEP in msg


def test_unsupported_sizes_are_refused_before_any_hip_call():
    for call, who in ((_estep, ESTEP), (_mstep, MSTEP)):
        rc, msg = call(K=129)
        assert rc == _lib.EUNSUP and who in msg and "128" in msg
        rc, msg = call(K=128, V=1 << 21)      # 2^21 rows of 1 KiB: past the buffer resource's 32-bit offsets
        assert rc == _lib.EUNSUP and who in msg and "32-bit" in msg
        rc, msg = call(nnz=1 << 28)           # 2^28 ratios of 8 bytes, the same limit
        assert rc == _lib.EUNSUP and who in msg and "32-bit" in msg
    rc, msg = _mstep(B=1 << 24, lde=16)       # an etheta of 2^24 rows of 128 bytes
    assert rc == _lib.EUNSUP and MSTEP in msg and "32-bit" in msg


def test_python_refusals_that_need_no_device():
    ip, ix = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([1, 5], dtype=torch.int32)
    ct = torch.ones(2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="num_topics=129"):
        fit_topics(ip, ix, ct, 10, num_topics=129)
    with pytest.raises(RuntimeError, match="num_topics=0"):
        fit_topics(ip, ix, ct, 10, num_topics=0)
    with pytest.raises(RuntimeError, match="max_iter >= 1"):
        fit_topics(ip, ix, ct, 10, num_topics=4, max_iter=0)
    with pytest.raises(RuntimeError, match="V >= 1"):
        fit_topics(ip, ix, ct, 0, num_topics=4)
    with pytest.raises(RuntimeError, match="max_doc_update_iter"):
        fit_topics(ip, ix, ct, 10, num_topics=4, max_doc_update_iter=topic_infer.MAX_UPDATE_ITER + 1)
    with pytest.raises(RuntimeError, match="float32 E-step"):
        fit_topics(ip, ix, ct.to(torch.float32), 10, num_topics=4)
    with pytest.raises(RuntimeError, match="ROCm GPU"):     # never a host fallback
        fit_topics(ip, ix, ct, 10, num_topics=4)
