"""The batch-EM restatement (tests/lda_ref.py) pinned on the CPU to the reference's own fit of 200 R8
documents (tests/golden/lda_fit_r8_small.npz), and the conditions that make the GPU tests' demands fair:
every document far from the stop rule's edge in every EM iteration, and sklearn's random stream reproduced."""
import numpy as np
import pytest

import lda_fit_cases
import lda_ref

MIN_MARGIN = lda_fit_cases.MIN_MARGIN


@pytest.fixture(scope="module")
def golden():
    return lda_ref.load_fit_golden()


def test_fixture_holds_what_the_generator_documents(golden):
    z = golden
    K, V = z["components_"].shape
    assert (K, V) == (8, 1200) == z["lambda0"].shape == z["topic_word_distribution"].shape and int(z["V"]) == V
    assert z["indptr"].shape == (201,) and z["indptr"][-1] == z["indices"].size == z["counts"].size == 7296
    assert z["gamma0"].shape == (3, 200, K) and z["iterations"].shape == (3, 200)
    assert z["components_"].dtype == z["lambda0"].dtype == z["gamma0"].dtype == np.float64
    assert z["counts"].dtype == np.int64 and z["iterations"].dtype == np.int32
    assert 0 <= z["indices"].min() and z["indices"].max() < V
    for d in range(200):   # a document's word ids are distinct and ascend
        assert np.all(np.diff(z["indices"][z["indptr"][d]:z["indptr"][d + 1]]) > 0)
    assert float(z["doc_topic_prior_"]) == float(z["topic_word_prior_"]) == 1.0 / K
    assert float(z["mean_change_tol"]) == 1e-3 and int(z["max_doc_update_iter"]) == 100
    tw = z["components_"] / z["components_"].sum(axis=1, keepdims=True)
    assert np.array_equal(tw, z["topic_word_distribution"])


def test_restatement_against_the_reference_lambda(golden):
    z = golden
    lam, iters, margin = lda_fit_cases.golden_fit()
    d_ref = lda_ref.max_rel(lam, z["components_"])
    print(f"max relative |lambda_restatement - lambda_reference| = {d_ref:.3e} (stored {float(z['d_ref']):.3e}); "
          f"d_perm stored {float(z['d_perm']):.3e}; smallest stop margin {margin:.3e}")
    assert d_ref == float(z["d_ref"]) and d_ref < 1e-12
    assert np.array_equal(iters, z["iterations"])
    # the cap is reached in EM iterations 0 and 1, not in 2
    cap = int(z["max_doc_update_iter"])
    assert (iters == cap).any(1).tolist() == [True, True, False]


def test_no_document_stops_near_the_tolerance(golden):
    """Equal update counts are a fair demand only while no mean change comes within 1e-6 (relative) of the
    tolerance, at any update of any EM iteration."""
    margin = lda_fit_cases.golden_fit()[2]
    assert margin == float(golden["stop_margin"]) and margin >= MIN_MARGIN
    assert margin > 1e-4   # (1.9e-4 on this fixture)


def test_a_reorder_of_every_documents_words_moves_lambda_by_d_perm(golden):
    z = golden
    pi, pc = lda_ref.permuted(z["indptr"], z["indices"], z["counts"])
    assert not np.array_equal(pi, z["indices"])
    lam_p, iters_p, _ = lda_ref.fit(z["indptr"], pi, pc, z["lambda0"], z["gamma0"], float(z["doc_topic_prior_"]),
                                        float(z["topic_word_prior_"]), float(z["mean_change_tol"]),
                                        int(z["max_doc_update_iter"]))
    lam, iters, _ = lda_fit_cases.golden_fit()
    assert np.array_equal(iters_p, iters)
    assert lda_ref.max_rel(lam, lam_p) == float(z["d_perm"]) < 1e-12


def test_random_state_reproduces_the_stored_draws(golden):
    z = golden
    K, V = z["lambda0"].shape
    lam0, g0s = lda_ref.draws(int(z["random_state"]), K, V, 200, 3)
    assert np.array_equal(lam0, z["lambda0"]) and np.array_equal(g0s, z["gamma0"])


def test_one_big_draw_equals_successive_draws():
    rs = np.random.RandomState(7)
    rs.gamma(100.0, 0.01, (5, 33))
    one = rs.gamma(100.0, 0.01, (4, 21, 5))
    rs = np.random.RandomState(7)
    rs.gamma(100.0, 0.01, (5, 33))
    for it in range(4):
        assert np.array_equal(rs.gamma(100.0, 0.01, (21, 5)), one[it])


def test_restatement_against_sklearn(golden):
    pytest.importorskip("sklearn")
    from sklearn.decomposition import LatentDirichletAllocation
    import scipy.sparse as sp
    z = golden
    K, V = z["components_"].shape
    X = sp.csr_matrix((z["counts"], z["indices"], z["indptr"]), shape=(200, V))
    lda = LatentDirichletAllocation(n_components=K, random_state=int(z["random_state"]), max_iter=3,
                                    learning_method="batch").fit(X)
    lam = lda_fit_cases.golden_fit()[0]
    assert lda_ref.max_rel(lam, lda.components_) < 1e-11


@pytest.mark.parametrize("name", lda_fit_cases.ESTEP_NAMES)
def test_estep_case_stop_margins(name):
    c = lda_fit_cases.estep_table()[name]
    gamma, etheta, ratio, iters, margin = lda_fit_cases.estep_reference(name)
    assert margin.min() >= MIN_MARGIN, (name, int(margin.argmin()), float(margin.min()))
    assert np.all(iters <= c["max_iter"]) and np.isfinite(gamma).all() and np.isfinite(etheta).all()
    assert np.isfinite(ratio).all() and ratio.shape == c["indices"].shape
    if c["max_iter"] == 0:
        assert np.all(iters == 0) and np.array_equal(gamma, c["gamma0"])
    if ratio.size:
        assert ratio.min() > 0


def test_case_tables_cover_what_they_say():
    t = lda_fit_cases.estep_table()
    assert {c["K"] for c in t.values()} >= {1, 3, 16, 50, 64, 65, 128}
    assert {int(n) for c in t.values() for n in np.diff(c["indptr"])} >= {0, 1, 63, 64, 65, 199}
    assert {len(c["indptr"]) - 1 for c in t.values()} >= {1, 2, 3, 13}
    assert {c["max_iter"] for c in t.values()} >= {0, 1, 3, 100}
    e = t["edge-ids-unsorted"]
    assert 0 in e["indices"] and e["V"] - 1 in e["indices"]
    assert t["counts-thousand"]["counts"].max() == 1000 and t["counts-ones"]["counts"].max() == 1
    m = lda_fit_cases.mstep_table()
    assert {c["K"] for c in m.values()} >= {1, 3, 16, 50, 64, 65, 128} and {c["V"] for c in m.values()} >= {1, 2, 65}
    for name in ("K50", "chains", "V2"):
        c = m[name]
        df = np.bincount(c["indices"], minlength=c["V"])
        assert df.max() == c["B"] and c["B"] in (13, 300)            # a word in every document
    assert np.bincount(m["K50"]["indices"], minlength=65)[5] == 0     # a word in none
    assert tuple(np.bincount(m["chains"]["indices"], minlength=len(lda_fit_cases.CHAINS))) == lda_fit_cases.CHAINS
    assert 0 in np.diff(m["empty-documents"]["indptr"]) and m["empty-corpus"]["indices"].size == 0


def test_mstep_restatement_is_the_outer_product_accumulate():
    """lda_ref.mstep against sklearn's own statement: sstats[:, ids] += np.outer(etheta_d, r_d), document
    by document, then eta + sstats * beta."""
    c = lda_fit_cases.mstep_table()["K16"]
    S = np.zeros((c["K"], c["V"]))
    for d in range(c["B"]):
        lo, hi = c["indptr"][d], c["indptr"][d + 1]
        S[:, c["indices"][lo:hi]] += np.outer(c["etheta"][d], c["ratio"][lo:hi])
    want = c["eta"] + S * c["beta"]
    assert np.array_equal(lda_fit_cases.mstep_reference("K16"), want)
    assert np.all(lda_fit_cases.mstep_reference("K16")[:, 5] == c["eta"])
