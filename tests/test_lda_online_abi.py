"""The online M-step's entry point without a GPU: gcnk_lda_mstep_online_f64 declared, exported and bound within
ABI 13, every refusal before any HIP call with its reason in gcnk_last_error, the public names, and the Python
refusals of the online method."""
import math

import pytest
import torch

import gcn_amd
from graph_convolutional_networks_for_text_classification_amd import OnlineTopics, TopicFit, _lib, fit_topics, topic_fit

from lda_abi import PTR, assert_declared_exported_bound, call, header, kernels_source

ONLINE = "gcnk_lda_mstep_online_f64"
NARGS = 20      # the declaration in include/gcnk_lda.h, counted: 19 operands and the stream


def _online(**kw):
    return call(ONLINE, **kw)


def test_symbol_declared_exported_and_bound():
    assert_declared_exported_bound({ONLINE: NARGS})
    assert "_em_step(batch_update=False)" in header()[0]
    kernels = kernels_source()
    assert ONLINE in kernels
    # one summation chain, which both M-step kernels instantiate
    assert kernels.count("void mstep_chain(") == 1 and kernels.count("mstep_chain<kTwo>(") == 2


def test_public_names_and_docstring():
    assert gcn_amd.OnlineTopics is OnlineTopics is topic_fit.OnlineTopics and gcn_amd.fit_topics is fit_topics
    assert {"OnlineTopics", "fit_topics", "TopicFit", "topic_fit"} <= set(gcn_amd.__all__)
    assert "n_batch_iter" in TopicFit.__slots__
    for what in ("bound_", "online", "evaluate_every", "n_jobs", "float32", "partial_fit", "out of scope"):
        assert what in topic_fit.__doc__


@pytest.mark.parametrize("kw", [dict(B=0), dict(K=0), dict(V=0), dict(wptr=None), dict(pos=None), dict(doc=None),
                                dict(ratio=None), dict(etheta=None), dict(lam=None), dict(table=None),
                                dict(table=PTR + 8), dict(ldt=15), dict(ldt=17), dict(lde=15), dict(ldl=99),
                                dict(nnz=-1), dict(doc_lo=-1), dict(doc_hi=9), dict(doc_lo=6, doc_hi=6),
                                dict(doc_lo=7, doc_hi=6), dict(rho=0.0), dict(rho=-0.5), dict(rho=1.0000000000000002),
                                dict(rho=math.nan), dict(rho=math.inf), dict(doc_ratio=0.0), dict(doc_ratio=-1.0),
                                dict(doc_ratio=math.nan), dict(doc_ratio=math.inf)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_online_mstep_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = _online(**kw)
    assert rc == _lib.EARG and ONLINE in msg


def test_unsupported_sizes_are_refused_before_any_hip_call():
    rc, msg = _online(K=129)
    assert rc == _lib.EUNSUP and ONLINE in msg and "128" in msg
    rc, msg = _online(K=128, V=1 << 21)      # 2^21 rows of 1 KiB: past the buffer resource's 32-bit offsets
    assert rc == _lib.EUNSUP and ONLINE in msg and "32-bit" in msg
    rc, msg = _online(nnz=1 << 28)           # 2^28 ratios of 8 bytes, the same limit
    assert rc == _lib.EUNSUP and ONLINE in msg and "32-bit" in msg
    rc, msg = _online(B=1 << 24, lde=16)     # an etheta of 2^24 rows of 128 bytes
    assert rc == _lib.EUNSUP and ONLINE in msg and "32-bit" in msg


def test_python_refusals_that_need_no_device():
    ip, ix = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([1, 5], dtype=torch.int32)
    ct = torch.ones(2, dtype=torch.float64)
    kw = dict(num_topics=4, learning_method="online")
    with pytest.raises(RuntimeError, match="learning_method"):
        fit_topics(ip, ix, ct, 10, num_topics=4, learning_method="minibatch")
    with pytest.raises(RuntimeError, match="batch_size"):
        fit_topics(ip, ix, ct, 10, batch_size=0, **kw)
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(RuntimeError, match="learning_decay"):
            fit_topics(ip, ix, ct, 10, learning_decay=bad, **kw)
    for bad in (0.5, 0.0, math.nan):
        with pytest.raises(RuntimeError, match="learning_offset"):
            fit_topics(ip, ix, ct, 10, learning_offset=bad, **kw)
    with pytest.raises(RuntimeError, match="ROCm GPU"):     # never a host fallback
        fit_topics(ip, ix, ct, 10, **kw)
    with pytest.raises(RuntimeError, match="batch_size"):
        OnlineTopics(10, num_topics=4, batch_size=0)
    with pytest.raises(RuntimeError, match="learning_decay"):
        OnlineTopics(10, num_topics=4, learning_decay=2.0)
    with pytest.raises(RuntimeError, match="learning_offset"):
        OnlineTopics(10, num_topics=4, learning_offset=0.0)
    with pytest.raises(RuntimeError, match="total_samples"):
        OnlineTopics(10, num_topics=4, total_samples=0)
    with pytest.raises(RuntimeError, match="num_topics=129"):
        OnlineTopics(10, num_topics=129)
    with pytest.raises(RuntimeError, match="V >= 1"):
        OnlineTopics(0, num_topics=4)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        OnlineTopics(10, num_topics=4, device="cpu")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        OnlineTopics(10, num_topics=4, init_components=torch.ones((4, 10), dtype=torch.float64))
