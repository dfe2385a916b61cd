"""gcnk_lda_* without a GPU: declared, exported and bound within ABI 13, and every refusal -- of the entry
points and of the Python layer -- before any HIP call, with its reason in gcnk_last_error."""
import numpy as np
import pytest
import torch

import gcn_amd
from graph_convolutional_networks_for_text_classification_amd import TopicInferencer, _lib, doc_term, topic_infer

import abi_bound
import lda_abi
from lda_abi import PTR, assert_declared_exported_bound, call, header, kernels_source

NAMES = {"gcnk_lda_max_topics": 0, "gcnk_lda_tile_words": 0, "gcnk_lda_docs_per_block": 0,
         "gcnk_lda_exp_dirichlet_f64": 7, "gcnk_lda_table_from_exp_f64": 7, "gcnk_lda_estep_f64": 22}
ESTEP = "gcnk_lda_estep_f64"


def _estep(**kw):
    return call(ESTEP, **kw)


def test_symbols_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES)
    text = header()[0]
    assert "topic_model.py:133-164" in text and "gcnk_lda_" in text.split("#define GCNK_ABI_VERSION")[0]
    assert ESTEP in kernels_source()


def test_gcnk_lda_h_declares_the_four_files_names_and_nothing_else():
    assert abi_bound.declared_names("gcnk_lda.h") == lda_abi.all_names() and len(lda_abi.all_names()) == 14


def test_constants_and_public_names():
    lib = _lib.load()
    assert lib.gcnk_lda_max_topics() == topic_infer.MAX_TOPICS == lib.gcnk_topic_graph_max_topics() == 128
    assert lib.gcnk_lda_tile_words() == topic_infer.TILE_WORDS >= 64
    assert lib.gcnk_lda_docs_per_block() == topic_infer.DOCS_PER_BLOCK >= 1
    assert gcn_amd.TopicInferencer is TopicInferencer and gcn_amd.doc_term is doc_term


@pytest.mark.parametrize("kw", [dict(B=0), dict(K=0), dict(K=-1), dict(V=0), dict(indptr=None), dict(indices=None),
                                dict(counts=None), dict(table=None), dict(table=PTR + 8), dict(ldt=15), dict(ldt=17),
                                dict(kind=3), dict(kind=-1), dict(max_iter=-1), dict(max_iter=10001),
                                dict(theta=None), dict(theta=None, x=PTR), dict(theta=None, a=PTR), dict(ldth=15),
                                dict(x=PTR, a=PTR, ldx=15), dict(x=PTR, a=PTR, lda=15), dict(gamma=PTR, ldth=3)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_bad_arguments_are_refused_before_any_hip_call(kw):
    rc, msg = _estep(**kw)
    assert rc == _lib.EARG and ESTEP in msg


def test_unsupported_sizes_are_refused_before_any_hip_call():
    rc, msg = _estep(K=129)
    assert rc == _lib.EUNSUP and ESTEP in msg and "128" in msg
    rc, msg = _estep(K=128, V=1 << 21)   # 2^21 rows of 1 KiB: past the buffer resource's 32-bit offsets
    assert rc == _lib.EUNSUP and "32-bit" in msg


@pytest.mark.parametrize("fn", ["gcnk_lda_exp_dirichlet_f64", "gcnk_lda_table_from_exp_f64"])
def test_table_builders_refuse(fn):
    for kw, want in ((dict(src=None), _lib.EARG), (dict(ld=99), _lib.EARG), (dict(K=0), _lib.EARG),
                     (dict(K=129, ldt=130), _lib.EUNSUP), (dict(V=0), _lib.EARG), (dict(table=None), _lib.EARG),
                     (dict(ldt=15), _lib.EARG), (dict(ldt=17), _lib.EARG), (dict(table=PTR + 8), _lib.EARG)):
        rc, msg = call(fn, **kw)
        assert rc == want and fn in msg, kw


def test_python_refusals_that_need_no_device():
    beta = torch.full((4, 30), 0.1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        TopicInferencer(beta, 0.25)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        TopicInferencer.from_components(beta, 0.25)
    ip, ix = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([1, 5], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="float32 E-step"):
        topic_infer.check_documents(ip, ix, torch.ones(2, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        topic_infer.check_documents(ip, ix, torch.ones(2, dtype=torch.float64))


def test_doc_term_on_the_host():
    sp = pytest.importorskip("scipy.sparse")
    X = sp.csr_matrix(np.array([[0, 2, 0, 1], [0, 0, 0, 0], [3, 0, 0, 0]], np.int64))
    ip, ix, c = doc_term(X, "cpu")
    assert (ip.dtype, ix.dtype, c.dtype) == (torch.int32, torch.int32, torch.float64)
    assert ip.tolist() == [0, 2, 2, 3] and ix.tolist() == [1, 3, 0] and c.tolist() == [2.0, 1.0, 3.0]
    with pytest.raises(RuntimeError, match="float32 E-step"):
        doc_term(X.astype(np.float32), "cpu")
    with pytest.raises(RuntimeError):
        doc_term(np.zeros((2, 2)), "cpu")
