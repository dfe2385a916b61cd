"""gcnk_score_docs_f32 without a GPU: the symbol is declared, exported and bound,
its refusals come before any launch, and the definition it implements
(tests/score_ref.py, float64) is the reference's forward on R8's documents."""
import ctypes
import os
import re

import numpy as np
import pytest

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

import score_ref
from abi_bound import assert_declared_exported_bound, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gcnk_score_docs_f32"
PTR = 0x10000   # a 16-byte aligned address that no refused call dereferences


def _call(B=40, F=200, Kc=50, H=50, P=8, k0=0, x=PTR, ldx=None, a=PTR, lda=None, W1=PTR, ldw1=None, S=PTR, lds=None,
          W2=PTR, ldw2=None, S2=PTR, lds2=None, dh=PTR, b1=None, b2=None, out=PTR, ldo=None, labels=None):
    r4 = lambda n: (n + 3) // 4 * 4
    lib = _lib.load()
    rc = lib.gcnk_score_docs_f32(
        B, F, Kc, H, P, k0, x, r4(Kc) if ldx is None else ldx, a, r4(H) if lda is None else lda,
        W1, F if ldw1 is None else ldw1, S, F if lds is None else lds, W2, P if ldw2 is None else ldw2,
        S2, P if lds2 is None else lds2, dh, b1, b2, out, P if ldo is None else ldo, labels, None)
    return rc, lib.gcnk_last_error().decode()


def test_symbol_declared_exported_and_bound():
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header()[1])
    assert_declared_exported_bound({NAME: 25}, restype=ctypes.c_int)


@pytest.mark.parametrize("kw", [dict(H=129), dict(Kc=129), dict(P=33), dict(F=6), dict(F=260), dict(x=PTR + 4),
                                dict(ldx=50), dict(lda=54), dict(W1=PTR + 8), dict(S=PTR + 4), dict(ldw1=202)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_unsupported_shapes_are_refused_before_any_launch(kw):
    rc, msg = _call(**kw)
    assert rc == _lib.EUNSUP and NAME in msg


@pytest.mark.parametrize("kw", [dict(ldx=49), dict(lda=49), dict(ldw1=199), dict(lds=196), dict(ldw2=7), dict(lds2=7),
                                dict(ldo=7), dict(out=None), dict(x=None), dict(dh=None), dict(S2=None), dict(B=-1),
                                dict(F=0), dict(k0=-1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_bad_arguments_are_refused_before_any_launch(kw):
    rc, msg = _call(**kw)
    assert rc == _lib.EARG and NAME in msg


def test_empty_batch_succeeds_without_a_device():
    assert _call(B=0)[0] == _lib.OK
    assert _call(B=0, labels=PTR)[0] == _lib.OK


def test_label_rule_of_the_restatement():
    nan = float("nan")
    out = np.array([[1.0, 3.0, 3.0], [nan, 5.0, nan], [0.0, nan, 9.0], [-1.0, -1.0, -2.0]])
    assert score_ref.labels(out).tolist() == [1, 0, 1, 0]


def _r8_float64():
    import scipy.sparse as ssp
    z = np.load(os.path.join(ROOT, "tests", "golden", "r8_graph.npz"), allow_pickle=False)
    N, nfeat, ndoc, ntopic, nclass = (int(v) for v in z["shape"])
    A = ssp.csr_matrix((z["adj_val"].astype(np.float64), (z["adj_row"], z["adj_col"])), shape=(N, N))
    X = ssp.vstack([ssp.hstack([ssp.csr_matrix(z["x_doc"].astype(np.float64)),
                                ssp.csr_matrix((ndoc, nfeat - ntopic))]),
                    ssp.csr_matrix(z["x_topic"].astype(np.float64))]).tocsr()
    return A, X, z["x_doc"], ndoc, ntopic, nfeat, nclass


@pytest.fixture(scope="module")
def r8_f64():
    return _r8_float64()


@pytest.mark.parametrize("seed", [50494, 99346, 0])
def test_definition_reproduces_the_golden_logits_on_r8(r8_f64, golden_logits, seed):
    """Every R8 document scored "as new" by the float64 restatement -- x = its X
    row, a recovered from A-hat, W / b the reference's init for the seed, the
    held state from the math -- is its row of the reference's eval logits within
    the 1e-4 the project allows for them: the definition is the reference's."""
    A, X, x_doc, ndoc, ntopic, nfeat, nclass = r8_f64
    hubs = np.arange(ndoc, ndoc + ntopic)
    W1, b1, W2, b2 = score_ref.reference_init(seed, nfeat, 200, nclass)
    S_T, S2_T = score_ref.held_state(A, X, hubs, W1, b1, W2)
    a, dh = score_ref.recovered_edges(A, np.arange(ndoc), hubs)
    assert (a >= 0).all() and np.count_nonzero(a) == A[:ndoc][:, hubs].nnz
    out = score_ref.score(x_doc, a, W1, S_T, W2, S2_T, dh, b1, b2)
    gold = golden_logits[f"eval_{seed}"][:ndoc]
    err = float(np.abs(out - gold).max())
    print(f"seed {seed}: max |restatement - golden| = {err:.3e}")
    assert err <= 1e-4
    # and the coefficients are A-hat's own entries again (to the ulp that recovering a in fp32 costs)
    c_self, c = score_ref.coefficients(a, dh)
    sub = np.asarray(A[:ndoc][:, hubs].todense())
    print(f"coefficients: {np.mean(c_self.astype(np.float64) == A.diagonal()[:ndoc]):.4f} of c_self, "
          f"{np.mean(c.astype(np.float64) == sub):.4f} of c equal A-hat's fp32 entries")
    assert np.abs(c.astype(np.float64) - sub).max() <= 2e-7 and np.abs(c_self - A.diagonal()[:ndoc]).max() <= 2e-7


@pytest.mark.parametrize("shape", score_ref.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_kernel_test_seeds_leave_few_near_ties(shape):
    """The seeds of tests/test_score_docs.py: by the float64 reference alone at
    most 1 % of a case's rows lie within twice the tolerance of a tie, with
    either bias present or absent (labels are compared on all the other rows)."""
    c = score_ref.make_case(shape)
    for b1 in (True, False):
        for b2 in (True, False):
            ref = score_ref.case_ref(c, b1, b2)
            near = int((score_ref.top2_gap(ref) <= 2 * score_ref.atol_of(ref)).sum())
            assert near <= shape[0] // 100, (b1, b2, near)


def test_route_covers_every_operand_column_the_kernel_reads():
    """gcnk_score_docs_route over every (Kc, H) in range, at F and P of each
    instantiation: the operand-row columns the kernel writes cover what its
    MFMA k-loop (0 .. roundup4(Kc + H)) and its hub sum (Kc .. Kc + 16 KHQ) read
    and fit the row stride; the staged chunk is a positive multiple of 4 rows;
    the launch fits 160 KiB of LDS."""
    lib = _lib.load()
    out = (ctypes.c_int64 * 8)()
    beyond = 0
    for F, P in ((4, 1), (128, 16), (192, 17), (256, 32)):
        for Kc in range(1, 129):
            for H in range(1, 129):
                assert lib.gcnk_score_docs_route(F, Kc, H, P, out) == _lib.OK, (F, P, Kc, H)
                ntq, np_, khq, ch, kpa, wd, lds, per = out[:]
                kp = (Kc + H + 3) // 4 * 4
                assert (ntq, np_, khq) == (2 if F <= 128 else 3 if F <= 192 else 4, 1 if P <= 16 else 2,
                                           4 if H <= 64 else 8)
                assert H <= 16 * khq and wd >= kp and wd >= Kc + 16 * khq and wd <= kpa and kpa % 64 == 4
                assert ch >= 4 and ch % 4 == 0 and ch <= kp and lds <= 160 * 1024 and per == 1
                beyond += kp > Kc + 16 * khq
    assert beyond > 0     # (shapes whose k-loop reads past the hub sum's columns exist: they are why wd is reported)
    assert lib.gcnk_score_docs_route(256, 128, 128, 32, out) == _lib.OK and out[3] == 96   # three chunks of 256 rows
    for bad in ((6, 50, 50, 8), (260, 50, 50, 8), (200, 129, 50, 8), (200, 50, 129, 8), (200, 50, 50, 33)):
        assert lib.gcnk_score_docs_route(*bad, out) == _lib.EUNSUP
    assert lib.gcnk_score_docs_route(200, 0, 50, 8, out) == _lib.EARG
    assert lib.gcnk_score_docs_route(200, 50, 50, 8, None) == _lib.EARG
