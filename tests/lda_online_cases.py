"""The case table of the online M-step (csrc/lda_estep.hip, gcnk_lda_mstep_online_f64): seeded synthetic inputs at
the smallest shapes where the kernel can go wrong, with tests/lda_ref.py's serial loop for each, computed
once.  etheta, ratio, beta and lambda are seeded positive numbers: the launch is checked on identical inputs, bit
for bit.  The etheta rows of the documents OUTSIDE [doc_lo, doc_hi) are NaN: a search that is off by one entry on
either side poisons a sum instead of moving it a little.

  sub-ranges  B = 340 documents, the minibatch [20, 320): one word for every combination of
              (none / one / many) entries before the minibatch x (none / one / many) after it x an in-range chain of
              {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300} documents (lda_fit_cases.CHAINS: around
              the chain's rings of 16 and 32 entries and its loads of 64), plus a word no document holds and one
              random word: V = 137, not a multiple of the 4 words a workgroup takes.  K in {1, 50, 64, 65, 128}
              (one topic a lane and two), rho and doc_ratio varied across them.
  ranges      at the very start [0, 5), at the very end [8, 13), one document [6, 7), every document [0, 13) of B = 13.
  rho         1.0 (learning_decay = 0: lambda * +0), a typical np.power(10 + 2, -0.7) = 0.17..., and the smallest
              normal step np.power(10 + 10**6, -1.0);  doc_ratio 1.0 and 1e6 / 7: all six pairs.
  ldl         V and V + 3 (guard columns, which must come back untouched).
  no word     documents without any word (first, inner, last) and a corpus without one.
"""
import functools
import itertools

import numpy as np

import lda_cases
import lda_fit_cases
import lda_ref

KS = (1, 50, 64, 65, 128)
IN_RANGE = tuple(n for n in lda_fit_cases.CHAINS if n not in (47, 48, 49, 79, 80, 81))
SIDES = (0, 1, 7)            # none / one / many entries on a side of the minibatch
RHOS = (1.0, float(np.power(10.0 + 2, -0.7)), float(np.power(10.0 + 10 ** 6, -1.0)))
DOC_RATIOS = (1.0, 1e6 / 7)
assert IN_RANGE == (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)


def _case(name, K, has, doc_lo, doc_hi, rho, doc_ratio, seed, pad=0):
    """has: bool [B x V], which document holds which word."""
    rng = np.random.default_rng(seed)
    B, V = has.shape
    indptr, indices = lda_cases.csr_of(has)
    etheta = rng.uniform(1e-3, 1.0, (B, K))
    etheta[:doc_lo] = np.nan
    etheta[doc_hi:] = np.nan
    return dict(name=name, K=K, B=B, V=V, indptr=indptr, indices=indices, eta=1.0 / K, etheta=etheta,
                ratio=rng.gamma(2.0, 3.0, indices.size), beta=rng.gamma(0.3, 1.0, (K, V)) + 1e-3,
                lam=rng.gamma(100.0, 0.01, (K, V)), doc_lo=doc_lo, doc_hi=doc_hi, rho=rho, doc_ratio=doc_ratio, pad=pad)


def _sub_range_words(seed):
    """bool [340 x 137] and the (before, inside, after) counts of its first 135 words."""
    rng = np.random.default_rng(seed)
    B, lo, hi = 340, 20, 320
    combos = list(itertools.product(SIDES, IN_RANGE, SIDES))
    has = np.zeros((B, len(combos) + 2), bool)
    for w, (before, inside, after) in enumerate(combos):
        # "one" sits right at the edge of the minibatch: the entry a search off by one would take in
        has[[lo - 1] if before == 1 else rng.choice(lo, before, replace=False), w] = True
        has[rng.choice(np.arange(lo, hi), inside, replace=False) if inside not in (1, 300) else
            ([lo] if inside == 1 else np.arange(lo, hi)), w] = True
        has[[hi] if after == 1 else hi + rng.choice(B - hi, after, replace=False), w] = True
    has[:, -1] = rng.random(B) < 0.3          # (the word before it, len(combos), is held by no document)
    return has, combos


def _small(seed, B=13, V=67, empty=()):
    rng = np.random.default_rng(seed)
    has = rng.random((B, V)) < 0.3
    has[:, 0] = True      # a word in every document
    has[:, 5] = False     # and a word in none
    has[list(empty), :] = False
    return has


@functools.lru_cache(maxsize=None)
def table():
    """name -> case, in a fixed order."""
    pairs = list(itertools.product(RHOS, DOC_RATIOS))
    cases = []
    for i, K in enumerate(KS):
        has, _ = _sub_range_words(3100 + K)
        rho, ratio = pairs[(2 * i + 1) % len(pairs)]
        cases.append(_case(f"sub-ranges-K{K}", K, has, 20, 320, rho, ratio, seed=3200 + K, pad=3 * (i % 2)))
    for name, lo, hi in (("range-start", 0, 5), ("range-end", 8, 13), ("range-one-document", 6, 7), ("range-all", 0, 13)):
        cases.append(_case(name, 50, _small(3300 + lo), lo, hi, RHOS[1], 13.0 / (hi - lo), seed=3310 + lo, pad=3))
    for i, (rho, ratio) in enumerate(pairs):
        cases.append(_case(f"rho{RHOS.index(rho)}-ratio{DOC_RATIOS.index(ratio)}", 16, _small(3400 + i), 3, 9, rho, ratio,
                           seed=3410 + i, pad=3 * (i % 2)))
    cases += [
        _case("empty-documents", 65, _small(3500, empty=(0, 4, 5, 12)), 4, 13, RHOS[1], DOC_RATIOS[1], seed=3501, pad=3),
        _case("empty-corpus", 3, np.zeros((2, 5), bool), 0, 1, RHOS[1], 2.0, seed=3502),
        _case("V1", 3, np.ones((13, 1), bool), 2, 11, RHOS[1], 13.0 / 9, seed=3503, pad=3),
    ]
    return {c["name"]: c for c in cases}


NAMES = tuple(table())


@functools.lru_cache(maxsize=None)
def reference(name):
    """lda_ref.mstep_online of the case: the new lambda [K x V]; computed once, read-only."""
    c = table()[name]
    lam = lda_ref.mstep_online(c["indptr"], c["indices"], c["ratio"], c["etheta"], c["beta"], c["lam"], c["eta"], c["rho"],
                               c["doc_ratio"], c["doc_lo"], c["doc_hi"])
    lam.setflags(write=False)
    return lam
