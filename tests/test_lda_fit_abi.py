"""The LDA fit's entry points without a GPU: gcnk_lda_estep_fit_f64 and gcnk_lda_mstep_f64 declared, exported
and bound within ABI 13, every refusal of both before any HIP call with its reason in gcnk_last_error, and
the public names."""
import os
import re

import pytest
import torch

import gcn_amd
from graph_convolutional_networks_for_text_classification_amd import TopicFit, _lib, fit_topics, topic_fit, topic_infer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gcnk_lda_words_per_block": 0, "gcnk_lda_estep_fit_f64": 22, "gcnk_lda_mstep_f64": 16}
PTR = 0x10000   # an aligned address that no refused call dereferences
ESTEP, MSTEP = "gcnk_lda_estep_fit_f64", "gcnk_lda_mstep_f64"


def _estep(indptr=PTR, indices=PTR, counts=PTR, kind=0, B=8, V=100, K=16, table=PTR, ldt=None, alpha=0.1, tol=1e-3,
           max_iter=100, gamma0=PTR, ldg0=None, nnz=50, ratio=PTR, etheta=PTR, lde=None, gamma=None, ldg=0, iters=None):
    lib = _lib.load()
    kp = (K + 1) // 2 * 2
    rc = lib.gcnk_lda_estep_fit_f64(indptr, indices, counts, kind, B, V, K, table, kp if ldt is None else ldt, alpha,
                                    tol, max_iter, gamma0, K if ldg0 is None else ldg0, nnz, ratio, etheta,
                                    K if lde is None else lde, gamma, ldg, iters, None)
    return rc, lib.gcnk_last_error().decode()


def _mstep(wptr=PTR, pos=PTR, doc=PTR, nnz=50, ratio=PTR, etheta=PTR, lde=None, B=8, V=100, K=16, table=PTR, ldt=None,
           eta=0.1, lam=PTR, ldl=None):
    lib = _lib.load()
    kp = (K + 1) // 2 * 2
    rc = lib.gcnk_lda_mstep_f64(wptr, pos, doc, nnz, ratio, etheta, K if lde is None else lde, B, V, K, table,
                                kp if ldt is None else ldt, eta, lam, V if ldl is None else ldl, None)
    return rc, lib.gcnk_last_error().decode()


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "gcnk.h")) as f:
        text = f.read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, nargs in NAMES.items():
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert name in _lib.NEWER_THAN_SOME_VARIANTS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0]
    assert len(_lib.SIGNATURES["gcnk_lda_estep_f64"][1]) == 22   # the transform's entry point keeps its signature
    assert lib.gcnk_abi_version() == _lib.ABI_VERSION == 13
    assert "topic_model.py:74-131" in text
    with open(os.path.join(ROOT, "graph-convolutional-networks-for-text-classification_amd", "csrc", "Makefile")) as f:
        assert "lda_estep.hip" in f.read()
    with open(os.path.join(ROOT, "graph-convolutional-networks-for-text-classification_amd", "csrc", "lda_estep.hip")) as f:
        kernels = f.read()
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
