"""The online-EM restatement (tests/lda_ref.py) pinned on the CPU to the reference's own online fit of 200
R8 documents and to sklearn's online fit and partial_fit (tests/golden/lda_online_r8_small.npz), and the
conditions that make the GPU tests' demands fair: every document far from the stop rule's edge in every
minibatch, sklearn's random stream reproduced slice by slice, and the case table holding what it says."""
import functools

import numpy as np
import pytest

import lda_fit_cases
import lda_ref
import lda_online_cases

MIN_MARGIN = lda_fit_cases.MIN_MARGIN
RUNS = {"a": 128, "b": 64}     # fit runs: key -> batch_size


@pytest.fixture(scope="module")
def golden():
    return lda_ref.load_fit_golden(), lda_ref.load_online_golden()


@functools.lru_cache(maxsize=None)
def _restated(key):
    """The restatement's run of fixture run `key`: (lambda, iterations, margin, n_batch_iter)."""
    z, o = lda_ref.load_fit_golden(), lda_ref.load_online_golden()
    alpha, eta = float(z["doc_topic_prior_"]), float(z["topic_word_prior_"])
    tol, cap = float(z["mean_change_tol"]), int(z["max_doc_update_iter"])
    docs = (z["indptr"], z["indices"], z["counts"])
    if key in RUNS:
        return lda_ref.fit_online(*docs, z["lambda0"], z["gamma0"], alpha, eta, RUNS[key], 0.7, 10.0, tol, cap)
    total, bs, second = int(o["c_total_samples"]), int(o["c_batch_size"]), int(o["c_second"])
    hi = int(z["indptr"][second])
    lam, i1, m1, n = lda_ref.partial_fit(*docs, z["lambda0"], o["c_gamma0"][:200], alpha, eta, total, 1, bs, 0.7,
                                                10.0, tol, cap)
    lam, i2, m2, n = lda_ref.partial_fit(z["indptr"][:second + 1], z["indices"][:hi], z["counts"][:hi], lam,
                                                o["c_gamma0"][200:], alpha, eta, total, n, bs, 0.7, 10.0, tol, cap)
    return lam, np.concatenate([i1, i2]), min(m1, m2), n


def test_fixture_holds_what_the_generator_documents(golden):
    z, o = golden
    K, V = z["components_"].shape
    for key in "abc":
        assert o[f"{key}_components_"].shape == (K, V) and o[f"{key}_components_"].dtype == np.float64
        assert o[f"{key}_iterations"].dtype == np.int32
        assert o[f"{key}_iterations"].shape == ((3, 200) if key in RUNS else (270,))
        assert 0 < float(o[f"{key}_d_ref"]) < 1e-11 and 0 < float(o[f"{key}_d_perm"]) < 1e-11
    # sklearn's n_batch_iter_: 1 + the minibatches walked
    assert int(o["a_n_batch_iter_"]) == 1 + 3 * 2 and int(o["b_n_batch_iter_"]) == 1 + 3 * 4
    assert int(o["c_n_batch_iter_"]) == 1 + 4 + 2
    assert (int(o["c_total_samples"]), int(o["c_batch_size"]), int(o["c_second"])) == (1000, 64, 70)
    tw = o["a_components_"] / o["a_components_"].sum(axis=1, keepdims=True)
    assert np.array_equal(tw, o["a_topic_word_distribution"])
    assert not np.array_equal(o["a_components_"], z["components_"])      # the online fit is another model


@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_restatement_against_the_recorded_components(golden, key):
    z, o = golden
    lam, iters, margin, n = _restated(key)
    d_ref = lda_ref.max_rel(lam, o[f"{key}_components_"])
    print(f"{key}: max relative |lambda_restatement - components_| = {d_ref:.3e} (stored {float(o[f'{key}_d_ref']):.3e}); "
          f"d_perm stored {float(o[f'{key}_d_perm']):.3e}; smallest stop margin {margin:.3e}; n_batch_iter_ {n}")
    assert d_ref == float(o[f"{key}_d_ref"])
    assert np.array_equal(iters, o[f"{key}_iterations"])
    assert n == int(o[f"{key}_n_batch_iter_"])
    # equal update counts are a fair demand only while no mean change comes within 1e-6 (relative) of the tolerance
    assert margin == float(o[f"{key}_stop_margin"]) and margin >= MIN_MARGIN


def test_restatement_against_sklearn(golden):
    pytest.importorskip("sklearn")
    from sklearn.decomposition import LatentDirichletAllocation
    import scipy.sparse as sp
    z, o = golden
    K, V = z["components_"].shape
    X = sp.csr_matrix((z["counts"], z["indices"], z["indptr"]), shape=(200, V))
    lda = LatentDirichletAllocation(n_components=K, random_state=int(z["random_state"]), max_iter=3,
                                    learning_method="online", batch_size=64).fit(X)
    lam, _, _, n = _restated("b")
    assert lda_ref.max_rel(lam, lda.components_) < 1e-11 and n == lda.n_batch_iter_


def test_gamma0_slices_are_sklearns_stream(golden):
    """sklearn draws a (slice size, K) gamma0 per minibatch; the slices [it, b0:b1] of ONE (max_iter, B, K) draw
    are those draws, and so are the rows of one (B, K) draw per partial_fit."""
    z, o = golden
    K, V = z["lambda0"].shape
    for bs in (64, 128, 7):
        rs = np.random.RandomState(int(z["random_state"]))
        assert np.array_equal(rs.gamma(100.0, 0.01, (K, V)), z["lambda0"])
        for it in range(3):
            for b0, b1 in lda_ref.batches(200, bs):
                assert np.array_equal(rs.gamma(100.0, 0.01, (b1 - b0, K)), z["gamma0"][it, b0:b1])
    rs = np.random.RandomState(int(z["random_state"]))
    rs.gamma(100.0, 0.01, (K, V))
    for n, off in ((200, 0), (70, 200)):
        for b0, b1 in lda_ref.batches(n, 64):
            assert np.array_equal(rs.gamma(100.0, 0.01, (b1 - b0, K)), o["c_gamma0"][off + b0:off + b1])
    assert lda_ref.batches(200, 64) == [(0, 64), (64, 128), (128, 192), (192, 200)]
    assert lda_ref.batches(200, 200) == [(0, 200)] and lda_ref.batches(3, 7) == [(0, 3)]


@pytest.mark.parametrize("name", ["K16", "K65", "chains-K50", "empty-documents", "empty-corpus"])
def test_rho_one_in_one_minibatch_is_the_batch_mstep_bit_for_bit(name):
    c = lda_fit_cases.mstep_table()[name]
    lam = np.random.default_rng(11).gamma(100.0, 0.01, (c["K"], c["V"]))
    got = lda_ref.mstep_online(c["indptr"], c["indices"], c["ratio"], c["etheta"], c["beta"], lam, c["eta"], 1.0, 1.0,
                                      0, c["B"])
    want = lda_fit_cases.mstep_reference(name)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("name", ["range-start", "rho2-ratio1", "empty-documents"])
def test_mstep_restatement_is_sklearns_dense_update(name):
    """lda_ref.mstep_online against sklearn's own statement on dense arrays: sstats[:, ids] +=
    np.outer(etheta_d, r_d) over the minibatch's documents, sstats *= beta, components *= 1 - rho,
    components += rho * (eta + doc_ratio * sstats)."""
    c = lda_online_cases.table()[name]
    S = np.zeros((c["K"], c["V"]))
    for d in range(c["doc_lo"], c["doc_hi"]):
        lo, hi = c["indptr"][d], c["indptr"][d + 1]
        S[:, c["indices"][lo:hi]] += np.outer(c["etheta"][d], c["ratio"][lo:hi])
    S *= c["beta"]
    want = c["lam"].copy()
    rho = np.float64(c["rho"])
    want *= 1 - rho
    want += rho * (c["eta"] + c["doc_ratio"] * S)
    assert np.array_equal(lda_online_cases.reference(name).view(np.int64), want.view(np.int64))


def test_case_table_covers_what_it_says():
    t = lda_online_cases.table()
    assert {c["K"] for c in t.values()} >= {1, 50, 64, 65, 128}
    assert {(c["rho"], c["doc_ratio"]) for c in t.values()} >= {(r, q) for r in lda_online_cases.RHOS
                                                                for q in lda_online_cases.DOC_RATIOS}
    assert lda_online_cases.RHOS[0] == 1.0 and 0.17 < lda_online_cases.RHOS[1] < 0.18
    assert lda_online_cases.RHOS[2] == np.power(10.0 + 10 ** 6, -1.0) and lda_online_cases.DOC_RATIOS == (1.0, 1e6 / 7)
    assert {c["pad"] for c in t.values()} == {0, 3}
    assert any(c["V"] % 4 for c in t.values())
    for K in lda_online_cases.KS:
        c = t[f"sub-ranges-K{K}"]
        lo, hi, B = c["doc_lo"], c["doc_hi"], c["B"]
        doc_of = np.repeat(np.arange(B), np.diff(c["indptr"]))
        seen = set()
        for w in range(c["V"] - 2):
            d = doc_of[c["indices"] == w]
            seen.add((min(int((d < lo).sum()), 2), int(((lo <= d) & (d < hi)).sum()), min(int((d >= hi).sum()), 2)))
        assert seen == {(b, n, a) for b in (0, 1, 2) for n in lda_online_cases.IN_RANGE for a in (0, 1, 2)}
        assert not (c["indices"] == c["V"] - 2).any()                    # a word no document holds
        assert np.isnan(c["etheta"][:lo]).all() and np.isnan(c["etheta"][hi:]).all()
        assert np.isfinite(c["etheta"][lo:hi]).all() and np.isfinite(lda_online_cases.reference(c["name"])).all()
    assert (t["range-start"]["doc_lo"], t["range-end"]["doc_hi"]) == (0, t["range-end"]["B"])
    assert t["range-one-document"]["doc_hi"] - t["range-one-document"]["doc_lo"] == 1
    assert 0 in np.diff(t["empty-documents"]["indptr"]) and t["empty-corpus"]["indices"].size == 0
    for c in t.values():
        assert np.isfinite(lda_online_cases.reference(c["name"])).all(), c["name"]
