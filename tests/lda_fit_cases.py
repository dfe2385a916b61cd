"""The case tables of the LDA fit's two launches (csrc/lda_estep.hip: the fit E-step and the M-step): seeded
synthetic inputs at the smallest shapes where the kernels can go wrong, with tests/lda_ref.py's result
for each, computed once.

Fit E-step (lda_cases.py's models and documents, plus a gamma0 ~ Gamma(100, .01) draw per document):
  K in {1, 3, 16, 50, 64, 65, 128}, each with documents of {0, 1, 63, 64, 65, 199} distinct words (199: four
    chunks, so the pass after the loop walks chunks);
  B in {1, 2, 3, 13};  update caps 0, 1, 3 and 100 (at cap 0 the ratio comes from etheta(gamma0));
  counts of 1, of several, of 1,000;  word ids 0 and V - 1.
Every case is checked on the CPU (test_lda_fit_ref.py) to keep each document's mean change at least 1e-6
(relative) from the tolerance at every update; a case that missed it would be re-seeded HERE.

M-step (etheta and ratio are seeded positive numbers: the launch is checked on identical inputs, bit for bit):
  K as above with B = 13, V = 65, a word in every document and a word in none;  empty documents (first,
    inner, last) and a corpus without a word;
  chains of {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 300} documents at
    B = 300 (around the kernel's rings of 16 and 32 entries and its loads of 64), with one topic a lane (K = 50)
    and two (K = 65, 128);  V in {1, 2, 65}.
"""
import functools

import numpy as np

import lda_cases
import lda_ref

KS = lda_cases.KS
LENGTHS = (0, 1, 63, 64, 65, 199)
BATCHES = (1, 2, 3, 13)
MIN_MARGIN = lda_cases.MIN_MARGIN
CHAINS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 300)


def _estep_case(name, K, V, lengths, seed, **kw):
    c = lda_cases._case(name, K, V, lengths, seed, **kw)
    B = len(c["indptr"]) - 1
    c["gamma0"] = np.random.default_rng(seed + 5000).gamma(100.0, 0.01, (B, K))
    return c


@functools.lru_cache(maxsize=None)
def estep_table():
    """name -> fit E-step case, in a fixed order."""
    cases = [_estep_case(f"K{K}-lengths", K, 240, LENGTHS, seed=1100 + K) for K in KS]
    cases += [_estep_case(f"B{B}", 16, 120, [5 + (7 * i) % 36 for i in range(B)], seed=1200 + B) for B in BATCHES]
    cases += [
        _estep_case("counts-ones", 16, 150, [3, 20, 66], seed=1301, counts="ones"),
        _estep_case("counts-thousand", 16, 150, [3, 20, 66], seed=1302, counts="thousand"),
        _estep_case("edge-ids-unsorted", 50, 90, [12, 70], seed=1303, sort=False, edge_ids=True),
        _estep_case("cap0", 50, 200, [0, 9, 65, 199], seed=1304, max_iter=0),
        _estep_case("cap1", 50, 200, [0, 9, 65], seed=1305, max_iter=1),
        _estep_case("cap3", 16, 200, [9, 30, 65], seed=1306, max_iter=3),
    ]
    return {c["name"]: c for c in cases}


ESTEP_NAMES = tuple(estep_table())


@functools.lru_cache(maxsize=None)
def estep_reference(name):
    """lda_ref.estep of the case: (gamma, etheta, ratio, iters, margin); computed once, read-only."""
    c = estep_table()[name]
    out = lda_ref.estep(c["indptr"], c["indices"], c["counts"], c["beta"], c["gamma0"], c["alpha"], c["tol"],
                        c["max_iter"])
    for a in out:
        a.setflags(write=False)
    return out


def bound(iters):
    """64 (its + 1) 2^-52, lda_cases.bound with one more pass for the ratio after the loop: reasoned, not
    measured.  It is RELATIVE here, because gamma and etheta are not normalised as theta is:
      gamma, etheta  per document, max_k |dev - ref| <= bound * max_k |ref|.  (Relative to the row's largest
                     entry, as theta's absolute bound is relative to the row's sum 1: an etheta_k of a topic the
                     document does not use is exp(psi(gamma_k)) with gamma_k near alpha, where psi's slope
                     1 / gamma_k^2 multiplies gamma_k's own rounding by 1 / alpha -- no bound in ulps of such an
                     entry holds, and nothing downstream reads it to that precision: it enters phi and S only
                     in sums beside the row's large entries.)
      ratio          per entry, |dev - ref| <= bound * |ref|: c / phi with phi a sum of positive terms."""
    return 64.0 * (np.asarray(iters, np.float64) + 1.0) * 2.0 ** -52


def _mstep_case(name, K, B, V, seed, holders=None, density=0.3, empty=()):
    """holders: word -> the number of first documents that hold it (the rest of the words are random);
    empty: documents without a word."""
    rng = np.random.default_rng(seed)
    has = rng.random((B, V)) < density
    for w, n in (holders or {}).items():
        has[:, w] = np.arange(B) < n
    has[list(empty), :] = False
    indptr, indices = lda_cases.csr_of(has)
    return dict(name=name, K=K, B=B, V=V, indptr=indptr, indices=indices, eta=1.0 / K,
                etheta=rng.uniform(1e-3, 1.0, (B, K)), ratio=rng.gamma(2.0, 3.0, indices.size),
                beta=rng.gamma(0.3, 1.0, (K, V)) + 1e-3)


@functools.lru_cache(maxsize=None)
def mstep_table():
    cases = [_mstep_case(f"K{K}", K, 13, 65, seed=2100 + K, holders={0: 13, 5: 0}) for K in KS]
    cases += [
        _mstep_case("chains", 65, 300, len(CHAINS), seed=2201, holders=dict(enumerate(CHAINS))),
        _mstep_case("chains-K50", 50, 300, len(CHAINS), seed=2200, holders=dict(enumerate(CHAINS))),
        _mstep_case("chains-K128", 128, 300, len(CHAINS), seed=2202, holders=dict(enumerate(CHAINS))),
        _mstep_case("V1", 3, 13, 1, seed=2203, holders={0: 13}),
        _mstep_case("V1-unheld", 3, 2, 1, seed=2204, holders={0: 0}),
        _mstep_case("V2", 50, 300, 2, seed=2205, holders={0: 300}),
        _mstep_case("B1", 16, 1, 9, seed=2206, density=0.6),
        _mstep_case("empty-documents", 16, 13, 65, seed=2207, holders={5: 0}, empty=(0, 4, 12)),
        _mstep_case("empty-corpus", 3, 2, 5, seed=2208, density=0.0),
    ]
    return {c["name"]: c for c in cases}


MSTEP_NAMES = tuple(mstep_table())


@functools.lru_cache(maxsize=None)
def mstep_reference(name):
    c = mstep_table()[name]
    lam = lda_ref.mstep(c["indptr"], c["indices"], c["ratio"], c["etheta"], c["beta"], c["eta"])
    lam.setflags(write=False)
    return lam


@functools.lru_cache(maxsize=None)
def golden_fit():
    """The restatement's fit of the R8 fixture from its stored draws: (lambda, iterations, margin)."""
    z = lda_ref.load_fit_golden()
    lam, iters, margin = lda_ref.fit(z["indptr"], z["indices"], z["counts"], z["lambda0"], z["gamma0"],
                                     float(z["doc_topic_prior_"]), float(z["topic_word_prior_"]),
                                     float(z["mean_change_tol"]), int(z["max_doc_update_iter"]))
    lam.setflags(write=False)
    iters.setflags(write=False)
    return lam, iters, margin
