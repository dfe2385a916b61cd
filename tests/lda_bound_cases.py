"""The case table of the variational bound's launches (csrc/lda_estep.hip, gcnk_lda_bound_*_f64): seeded synthetic
models (lambda), documents and gamma at the smallest shapes where the kernels can go wrong, with
tests/lda_bound_ref.py's evaluation of each, computed once.

  K in {1, 2, 7, 64, 65, 128} (one topic; below, at and above a wave's 64 lanes; the maximum), each with documents
    of {0, 1, 63, 64, 65, 129} distinct words (empty; a full tile and both neighbours; three tiles) over V = 300
    words (the topic kernel's chunk of 256 and a partial second one);
  B in {1, 3} (3: an odd tail workgroup of one document);  V in {1, 5, 256, 257};
  counts of 1 and of 1,000;  gamma rows exactly alpha (what the E-step gives a document without a word) beside
    ordinary ones;  lambda from eta = 1/128 up to 1e4 in one row.
gamma is alpha + a Gamma(2, 3) draw: the bound takes any gamma, the E-step's or not.
"""
import functools

import numpy as np

import lda_bound_ref
import lda_cases

KS = (1, 2, 7, 64, 65, 128)
LENGTHS = (0, 1, 63, 64, 65, 129)
CHUNK = lda_bound_ref.TOPIC_CHUNK


def _case(name, K, V, lengths, seed, counts="several", alpha=None, eta=None, lam=None, prior_rows=()):
    rng = np.random.default_rng(seed)
    alpha = 1.0 / K if alpha is None else alpha
    eta = 1.0 / K if eta is None else eta
    if lam is None:
        lam = eta + rng.gamma(0.3, 1.0, (K, V))
    indptr, indices, data = lda_cases._docs(rng, V, lengths, counts)
    gamma = alpha + rng.gamma(2.0, 3.0, (len(lengths), K))
    gamma[list(prior_rows)] = alpha
    return dict(name=name, K=K, V=V, alpha=alpha, eta=eta, lam=lam, indptr=indptr, indices=indices, counts=data,
                gamma=gamma)


def _wide_lambda(K, V, eta):
    """Every row runs from eta up to 1e4, log-spaced, each row rotated by its index."""
    row = np.geomspace(eta, 1e4, V)
    return np.stack([np.roll(row, 3 * k) for k in range(K)])


@functools.lru_cache(maxsize=None)
def table():
    """name -> case, in a fixed order."""
    cases = [_case(f"K{K}-lengths", K, 300, LENGTHS, seed=3100 + K) for K in KS]
    cases += [
        _case("B1", 7, 40, [5], seed=3201),
        _case("B3", 7, 90, [5, 0, 70], seed=3202),
        _case("V1", 2, 1, [1, 0, 1], seed=3203),
        _case("V5", 7, 5, [5, 2, 0], seed=3204),
        _case(f"V{CHUNK}", 2, CHUNK, [64, 3], seed=3205),
        _case(f"V{CHUNK + 1}", 2, CHUNK + 1, [65, 3], seed=3206),
        _case("counts-ones", 16, 150, [3, 20, 66], seed=3207, counts="ones"),
        _case("counts-thousand", 16, 150, [3, 20, 66], seed=3208, counts="thousand"),
        _case("gamma-is-alpha", 7, 60, [0, 9, 0, 30], seed=3209, prior_rows=(0, 1, 2)),
        _case("gamma-is-alpha-K1", 1, 20, [0, 4], seed=3210, prior_rows=(0, 1)),
        _case("wide-lambda", 3, 70, [1, 40, 70], seed=3211, alpha=0.5, eta=1.0 / 128, lam=_wide_lambda(3, 70, 1.0 / 128)),
        _case("wide-lambda-K128", 128, 130, [1, 64, 130], seed=3212, lam=_wide_lambda(128, 130, 1.0 / 128)),
    ]
    return {c["name"]: c for c in cases}


NAMES = tuple(table())


@functools.lru_cache(maxsize=None)
def reference(name):
    """lda_bound_ref.evaluate of the case; computed once, never written to."""
    c = table()[name]
    out = lda_bound_ref.evaluate(c["indptr"], c["indices"], c["counts"], c["gamma"], c["lam"], c["alpha"], c["eta"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def golden():
    z = lda_bound_ref.load_golden()
    for a in z.values():
        a.setflags(write=False)
    return z


def factors():
    """(of the partials, of the bound): 16 max(d_ref, d_perm, d_fn) as the fixture records them -- test_topic_fit.py's
    rule and factor; a value is near when |x - y| <= factor * 2^-52 * A."""
    z = golden()
    return tuple(16.0 * max(float(z[f"d_{k}_{what}"]) for k in ("ref", "perm", "fn")) for what in ("parts", "total"))


@functools.lru_cache(maxsize=None)
def golden_reference(which):
    """The restatement's score of the fixture's ``train`` or ``held`` documents at ITS OWN gamma (lda_ref's E-step)."""
    z = golden()
    return lda_bound_ref.score(z[f"{which}_indptr"], z[f"{which}_indices"], z[f"{which}_counts"], z["components_"],
                               float(z["doc_topic_prior_"]), float(z["topic_word_prior_"]), float(z["mean_change_tol"]),
                               int(z["max_doc_update_iter"]))
