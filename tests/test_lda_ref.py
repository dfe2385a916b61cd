"""The E-step restatement (tests/lda_ref.py) pinned on the CPU: against the reference's own theta of 256
held-out R8 documents (tests/golden/lda_r8_small.npz), against sklearn where it is installed, and the two
conditions that make the GPU tests' demands fair -- every document far from the stop rule's edge, no theta at
the 0.02 threshold."""
import numpy as np
import pytest

import lda_cases
import lda_ref

BOUND = 1e-13


@pytest.fixture(scope="module")
def golden():
    return lda_ref.load_golden()


def test_fixture_holds_what_the_generator_documents(golden):
    z = golden
    K, V = z["components_"].shape
    assert (K, V) == (16, 2418) and z["exp_dirichlet_component_"].shape == (K, V)
    assert z["theta"].shape == (256, K) and z["indptr"].shape == (257,) and z["indptr"][-1] == z["indices"].size
    assert z["components_"].dtype == z["theta"].dtype == np.float64 and z["counts"].dtype == np.int64
    assert 0 <= z["indices"].min() and z["indices"].max() < V


def test_restatement_against_the_reference_theta(golden):
    theta, gamma, iters, margin = lda_cases.golden_reference()
    err = float(np.abs(theta - golden["theta"]).max())
    print(f"max |theta_ref - theta_reference| = {err:.3e}; iterations {iters.min()} .. {iters.max()}, "
          f"median {np.median(iters):.0f}")
    assert err <= BOUND
    assert iters.max() == int(golden["max_doc_update_iter"])   # one document reaches the cap
    assert np.array_equal(theta >= 0.02, golden["theta"] >= 0.02)


def test_restatement_against_sklearn(golden):
    pytest.importorskip("sklearn")
    from sklearn.decomposition import LatentDirichletAllocation
    import scipy.sparse as sp
    z = golden
    K, V = z["components_"].shape
    lda = LatentDirichletAllocation(n_components=K)
    lda.components_ = z["components_"]
    lda.exp_dirichlet_component_ = z["exp_dirichlet_component_"]
    lda.doc_topic_prior_ = float(z["doc_topic_prior_"])
    lda.n_features_in_ = V
    X = sp.csr_matrix((z["counts"], z["indices"], z["indptr"]), shape=(256, V))
    want = lda.transform(X)
    theta = lda_cases.golden_reference()[0]
    assert float(np.abs(theta - want).max()) <= BOUND
    # the model matrix as well: _dirichlet_expectation_2d, then exp
    assert np.array_equal(lda_ref.exp_dirichlet(z["components_"]), z["exp_dirichlet_component_"])


def test_psi_is_as103_not_the_accurate_digamma():
    x = np.array([1e-7, 1e-6, 1.0000001e-6, 0.02, 0.5, 1.0, 5.999999, 6.0, 50.0, 1e5])
    got = lda_ref.psi(x)
    assert got[0] == -lda_ref.EULER - 1.0 / 1e-7 and got[1] == -lda_ref.EULER - 1.0 / 1e-6
    assert abs(got[5] + lda_ref.EULER) < 1e-8 and got[5] != -lda_ref.EULER   # psi(1) to AS 103's 1e-9, not exactly
    assert np.isnan(lda_ref.psi(np.nan)[0])
    assert np.all(np.diff(got[2:]) > 0)


def test_fixture_stop_margin_and_threshold_distance(golden):
    margin = lda_cases.golden_reference()[3]
    print(f"smallest stop margin of the fixture: {margin.min():.3e}")
    assert margin.min() >= lda_cases.MIN_MARGIN
    assert float(np.abs(golden["theta"] - 0.02).min()) > 1e-9


@pytest.mark.parametrize("name", lda_cases.NAMES)
def test_case_stop_margins(name):
    """Equal iteration counts are a fair demand of the GPU only for documents whose mean change stays away
    from the tolerance: every document of every case must, or the case is re-seeded in lda_cases.py."""
    c = lda_cases.table()[name]
    theta, gamma, iters, margin = lda_cases.reference(name)
    assert margin.min() >= lda_cases.MIN_MARGIN, (name, int(margin.argmin()), float(margin.min()))
    assert np.all(iters <= c["max_iter"]) and np.isfinite(theta).all()
    assert np.abs(theta.sum(1) - 1).max() < 1e-14
    if c["max_iter"] == 0:
        assert np.all(iters == 0) and np.array_equal(theta, np.full_like(theta, 1.0 / c["K"]))
    if name == "never-converges":
        assert np.all(iters == c["max_iter"])


def test_case_table_covers_what_it_says():
    t = lda_cases.table()
    T, W = lda_cases.T, lda_cases.W
    assert {c["K"] for c in t.values()} >= {1, 3, 16, 50, 64, 65, 128}
    lengths = {int(n) for c in t.values() for n in np.diff(c["indptr"])}
    assert lengths >= {0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7}
    assert {len(c["indptr"]) - 1 for c in t.values()} >= {1, W, W + 1, 3 * W + 7}
    assert {c["max_iter"] for c in t.values()} >= {0, 1, 100}
    e = t["edge-ids-unsorted"]
    assert 0 in e["indices"] and e["V"] - 1 in e["indices"] and np.any(np.diff(e["indices"][:12]) < 0)
    assert t["counts-thousand"]["counts"].max() == 1000 and t["counts-ones"]["counts"].max() == 1
