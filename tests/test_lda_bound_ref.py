"""tests/lda_bound_ref.py, the float64 restatement of sklearn's variational bound, pinned on the CPU to the numbers
sklearn itself gave on the reference's model (tests/golden/lda_bound_r8_small.npz, make_lda_bound_golden.py), and
the generator's own assertions on the committed file.  The GPU tests (test_topic_bound.py) compare the kernels with
this restatement."""
import importlib.util
import os

import numpy as np
import pytest

import lda_bound_cases
import lda_bound_ref as R
import lda_ref


def _generator():
    spec = importlib.util.spec_from_file_location("make_lda_bound_golden",
                                                  os.path.join(lda_ref.GOLDEN_DIR, "make_lda_bound_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def z():
    return lda_bound_cases.golden()


def test_fixture_is_the_one_the_issue_measured(z):
    assert z["components_"].shape == (8, int(z["V"])) and len(z["train_indptr"]) == 201 and len(z["held_indptr"]) == 61
    fit = lda_ref.load_fit_golden()                       # the same reference fit as the fit fixture's
    assert np.array_equal(fit["components_"], z["components_"]) and np.array_equal(fit["indices"], z["train_indices"])
    assert float(z["train_score"]) == pytest.approx(-72238.66528440802, rel=1e-14)
    assert float(z["bound_"]) == pytest.approx(506.74506281987357, rel=1e-13) == pytest.approx(float(z["train_perplexity"]), rel=1e-12)
    assert 3.4e5 < float(z["train_A"]) < 3.6e5
    for k in ("ref", "perm", "fn"):
        assert 0 < float(z[f"d_{k}_total"]) < 8 and 0 < float(z[f"d_{k}_parts"]) < 32   # a few roundings, no more


@pytest.mark.parametrize("which", ["train", "held"])
def test_restatement_reproduces_sklearns_score_and_perplexity(z, which):
    own = lda_bound_cases.golden_reference(which)          # at the restatement's own gamma
    d = R.distance(own["bound"], float(z[f"{which}_score"]), own["A"])
    print(f"{which}: score {own['bound']!r} against sklearn's {float(z[f'{which}_score'])!r}: {d:.3f} (stored d_ref {float(z['d_ref_total']):.3f})")
    assert d <= float(z["d_ref_total"])
    count = float(z[f"{which}_counts"].sum())
    assert own["count"] == count
    # exp(-bound / count): the bound's distance over the count, relative, and the division's and exp's roundings
    rel = float(z["d_ref_total"]) * R.ULP * own["A"] / count + 4 * R.ULP * max(1.0, abs(own["bound"]) / count)
    assert abs(own["perplexity"] - float(z[f"{which}_perplexity"])) <= rel * float(z[f"{which}_perplexity"])


def test_bound_of_a_given_gamma_and_sub_sampling(z):
    held = (z["held_indptr"], z["held_indices"], z["held_counts"])
    alpha, eta = float(z["doc_topic_prior_"]), float(z["topic_word_prior_"])
    e = R.evaluate(*held, z["held_gamma"], z["components_"], alpha, eta)
    assert R.distance(e["bound"], float(z["held_score"]), e["A"]) <= float(z["d_ref_total"])
    sub = R.evaluate(*held, z["held_gamma"], z["components_"], alpha, eta, doc_ratio=1000.0 / 60)
    docs = R.dealt_sum(e["doc"], R.FINISH_THREADS)
    assert sub["bound"] == (1000.0 / 60) * docs + (e["bound"] - docs) and sub["count"] == e["count"]
    assert sub["perplexity"] == float(np.exp(-1.0 * (sub["bound"] / (e["count"] * (1000.0 / 60)))))


@pytest.mark.parametrize("method", ["batch", "online"])
def test_generators_assertions_hold_on_the_committed_file(z, method):
    gen = _generator()
    seq, perp_tol = z[f"ee_{method}_perplexities"], float(z[f"ee_{method}_perp_tol"])
    assert gen.check_perp_tol(seq, perp_tol) == int(z[f"ee_{method}_n_iter"]) == 7
    assert abs(float(z[f"ee_{method}_bound_"]) - seq[-1]) <= 1e-9 * seq[-1]      # the closing value is the last evaluated
    assert int(z[f"ee_{method}_n_batch_iter"]) == 1 + 8 * (1 if method == "batch" else 2)
    assert z["gamma0"].shape == (gen.EE_MAX_ITER, 200, 8) and z["lambda0"].shape == z["components_"].shape
    lam0, g0s = lda_ref.draws(int(z["random_state"]), 8, int(z["V"]), 200, gen.EE_MAX_ITER)
    assert np.array_equal(lam0, z["lambda0"]) and np.array_equal(g0s, z["gamma0"])


def test_trees_and_orders():
    v = np.arange(1.0, 65.0)
    assert R.wave_tree(v) == v.sum() and R.wave_tree(v[:5]) == 15.0 and R.wave_tree([]) == 0.0
    big = np.array([1e16, 1.0, -1e16, 1.0])                # adjacent pairs: (1e16 + 1) + (-1e16 + 1) = 0
    assert R.wave_tree(big) == 0.0 and float(lda_ref.seq_sum(big)) == 1.0
    x = np.random.default_rng(0).standard_normal(700)
    per_thread = np.array([float(lda_ref.seq_sum(x[t::256])) for t in range(256)])
    waves = [R.wave_tree(per_thread[i:i + 64]) for i in range(0, 256, 64)]
    assert R.dealt_sum(x, 256) == ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert R.distance(1.0, 1.0, 0.0) == 0.0 and R.distance(1.0, 2.0, 0.0) == np.inf


@pytest.mark.parametrize("name", lda_bound_cases.NAMES)
def test_case_table_is_well_conditioned(name):
    """Every synthetic case is finite, and another pair of correct library functions lands within the fixture's
    factor of it: the factor is a fair bound for a correct implementation at these shapes too."""
    c, ref = lda_bound_cases.table()[name], lda_bound_cases.reference(name)
    assert np.isfinite(ref["doc"]).all() and np.isfinite(ref["topic"]).all() and np.isfinite(ref["perplexity"])
    other = R.evaluate(c["indptr"], c["indices"], c["counts"], c["gamma"], c["lam"], c["alpha"], c["eta"], fn=R.LIBM)
    parts, total = R.distances(ref, other)
    f_parts, f_total = lda_bound_cases.factors()
    print(f"{name}: math.lgamma / shift logsumexp at {parts:.3f} (partials) and {total:.3f} (bound) of 2^-52 A")
    assert parts <= f_parts and total <= f_total
