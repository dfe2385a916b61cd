"""gcnk_topic_graph_* / gcnk_topic_cosine_f64 without a GPU: declared, exported and bound,
every refusal before any HIP call with its reason in gcnk_last_error, and the definition the
kernels implement (tests/topic_graph_ref.py) pinned to the reference's own A-hat of R8."""
import ctypes
import os

import numpy as np
import pytest

import gcn_amd
from graph_convolutional_networks_for_text_classification_amd import _lib, factor, topic_graph

import topic_graph_ref as ref
from abi_bound import assert_declared_exported_bound, declared_names, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gcnk_topic_graph_chunk": 0, "gcnk_topic_graph_max_topics": 0, "gcnk_topic_graph_nnz_bound": 3,
         "gcnk_topic_graph_workspace_bytes": 2, "gcnk_topic_graph_build": 18, "gcnk_topic_cosine_f64": 8}
PTR = 0x10000   # an aligned address that no refused call dereferences
BUILD = "gcnk_topic_graph_build"


def _build(theta=PTR, theta_f32=0, ldt=None, sim=PTR, sim_f32=0, lds=None, D=300, K=50, thr_doc=0.02, thr_top=0.3,
           rowptr=PTR, colind=PTR, val=PTR, capacity=None, edges=PTR, workspace=PTR, workspace_bytes=1 << 40):
    lib = _lib.load()
    if capacity is None:
        capacity = max(int(lib.gcnk_topic_graph_nnz_bound(D, K, int(sim is not None))), 0)
    rc = lib.gcnk_topic_graph_build(theta, theta_f32, K if ldt is None else ldt, sim, sim_f32,
                                    K if lds is None else lds, D, K, thr_doc, thr_top, rowptr, colind, val, capacity,
                                    edges, workspace, workspace_bytes, None)
    return rc, lib.gcnk_last_error().decode()


def test_symbols_declared_exported_and_bound():
    assert_declared_exported_bound(NAMES, header="gcnk_topic_graph.h")
    assert declared_names("gcnk_topic_graph.h") == set(NAMES) and len(NAMES) == 6   # these and nothing else
    text = header()[0]
    assert "build_graph.py:99-133" in text and "gcnk_topic_graph_" in text.split("#define GCNK_ABI_VERSION")[0]
    with open(os.path.join(ROOT, "graph-convolutional-networks-for-text-classification_amd", "csrc", "Makefile")) as f:
        assert "topic_graph.hip" in f.read()


def test_constants_and_public_names():
    lib = _lib.load()
    assert lib.gcnk_topic_graph_chunk() == topic_graph.DOCS_PER_BLOCK and topic_graph.DOCS_PER_BLOCK % 64 == 0
    assert lib.gcnk_topic_graph_max_topics() == topic_graph.MAX_TOPICS >= factor.MAX_HUBS == 128
    assert gcn_amd.build_topic_graph is topic_graph.build_topic_graph
    assert gcn_amd.topic_similarity is topic_graph.topic_similarity


@pytest.mark.parametrize("kw", [dict(D=0), dict(D=-3), dict(K=0), dict(thr_doc=0.0), dict(thr_doc=-0.02),
                                dict(thr_top=0.0), dict(thr_top=float("nan")), dict(theta=None), dict(rowptr=None),
                                dict(colind=None), dict(val=None), dict(workspace=None), dict(ldt=49), dict(lds=49),
                                dict(theta_f32=2), dict(capacity=100), dict(workspace_bytes=64)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_bad_arguments_are_refused_before_any_hip_call(kw):
    rc, msg = _build(**kw)
    assert rc == _lib.EARG and BUILD in msg


def test_unsupported_sizes_are_refused_before_any_hip_call():
    rc, msg = _build(K=129)
    assert rc == _lib.EUNSUP and BUILD in msg and "128" in msg
    # N + (N + 2 D K + K (K - 1)) must stay below 2^31: D = 2^23 at K = 128 passes it
    rc, msg = _build(D=1 << 23, K=128)
    assert rc == _lib.EUNSUP and "int32" in msg
    lib = _lib.load()
    assert lib.gcnk_topic_graph_nnz_bound(1 << 23, 128, 1) == _lib.EUNSUP
    assert lib.gcnk_topic_graph_nnz_bound(300, 129, 0) == _lib.EUNSUP
    assert lib.gcnk_topic_graph_nnz_bound(0, 50, 0) == _lib.EARG
    assert lib.gcnk_topic_graph_workspace_bytes(300, 129) == _lib.EUNSUP
    assert lib.gcnk_topic_graph_workspace_bytes(0, 5) == _lib.EARG
    # the null sim is no refusal by itself: its leading dimension is then not looked at
    assert _build(sim=None, lds=0, workspace_bytes=64)[1].count("workspace") == 1


def test_nnz_bound_counts_every_possible_entry():
    lib = _lib.load()
    assert lib.gcnk_topic_graph_nnz_bound(7674, 50, 1) == 7724 + 2 * 7674 * 50 + 50 * 49
    assert lib.gcnk_topic_graph_nnz_bound(7674, 50, 0) == 7724 + 2 * 7674 * 50
    assert lib.gcnk_topic_graph_nnz_bound(1, 1, 1) == 2 + 2


def test_workspace_query_is_monotone():
    lib = _lib.load()
    c = topic_graph.DOCS_PER_BLOCK
    sizes = [1, 2, 63, 64, 65, c - 1, c, c + 1, 3 * c + 7, 7674, 18846, 100000]
    for K in (1, 3, 50, 64, 65, 128):
        got = [lib.gcnk_topic_graph_workspace_bytes(D, K) for D in sizes]
        assert all(g > 0 for g in got) and got == sorted(got), (K, got)
    for D in sizes:
        got = [lib.gcnk_topic_graph_workspace_bytes(D, K) for K in range(1, 129)]
        assert got == sorted(got), D


@pytest.mark.parametrize("kw", [dict(K=0), dict(dim=0), dict(emb=None), dict(sim=None), dict(lde=99), dict(lds=49),
                                dict(f32=3)], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_cosine_refusals(kw):
    a = dict(emb=PTR, f32=0, lde=100, K=50, dim=100, sim=PTR, lds=50)
    a.update(kw)
    lib = _lib.load()
    rc = lib.gcnk_topic_cosine_f64(a["emb"], a["f32"], a["lde"], a["K"], a["dim"], a["sim"], a["lds"], None)
    assert rc == _lib.EARG and "gcnk_topic_cosine_f64" in lib.gcnk_last_error().decode()


def test_python_refusals_that_need_no_device():
    import torch
    theta = torch.full((4, 3), 1.0 / 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        topic_graph.build_topic_graph(theta)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        topic_graph.topic_similarity(torch.ones(3, 5))
    for bad in (dict(doc_topic_threshold=0.0), dict(topic_topic_threshold=-0.3)):
        with pytest.raises(ValueError, match="> 0"):
            topic_graph.build_topic_graph(theta, **bad)
    with pytest.raises(ValueError, match="not both"):
        topic_graph.build_topic_graph(theta, topic_sim=torch.eye(3), topic_emb=torch.ones(3, 5))


def test_restatement_reproduces_the_reference_a_hat_of_r8():
    """R8's kept theta entries and topic-block similarities (the raw A the reference built),
    through the rule "theta >= 0.02, sim > 0.3, sym_normalize": the golden A-hat, bit for bit."""
    theta, sim, D, K = ref.r8_inputs()
    rp, ci, v, ndt, ntt = ref.build(theta, sim, *ref.R8_THRESHOLDS)
    grp, gci, gv = ref.r8_golden()
    assert (ndt, ntt, ci.size) == (30466, 237, 69130)
    assert np.array_equal(rp, grp) and np.array_equal(ci, gci)
    assert np.array_equal(v.view(np.uint32), gv.view(np.uint32))


def test_restatement_edge_rules():
    """>= against > , float64 comparison, the ignored lower triangle, isolated nodes."""
    thr = 0.02
    theta = np.array([[thr, 0.5, 0.0], [np.nextafter(thr, 0), 0.3, 0.0], [0.0, 0.0, 0.0]])
    sim = np.array([[9.0, 0.3, 0.31], [0.9, 9.0, 0.2], [0.9, 0.9, 9.0]])
    rp, ci, v, ndt, ntt = ref.build(theta, sim, thr, 0.3)
    D = 3
    rows = [ci[rp[r]:rp[r + 1]].tolist() for r in range(6)]
    assert rows[0] == [0, D, D + 1] and rows[1] == [1, D + 1] and rows[2] == [2]
    assert rows[D] == [0, D, D + 2] and rows[D + 1] == [0, 1, D + 1] and rows[D + 2] == [D, D + 2]
    assert (ndt, ntt) == (3, 1) and v[rp[2]] == np.float32(1.0)
    # float32 inputs widen exactly: float32(0.02) < 0.02 is dropped, as the same value in float64 is
    t32 = np.array([[0.02, 0.5]], np.float32)
    a, b = ref.build(t32, None, thr, 0.3), ref.build(t32.astype(np.float64), None, thr, 0.3)
    assert a[3] == b[3] == 1 and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
