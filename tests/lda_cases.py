"""The case table of the LDA E-step (csrc/lda_estep.hip): seeded synthetic models and documents at the
smallest shapes where the kernel can go wrong, with tests/lda_ref.py's result for each, computed once.

With T = words a wave holds in LDS and W = documents per workgroup:
  K in {1, 3, 16, 50, 64, 65, 128} (one topic; below, at and above a wave's 64 lanes; the maximum), each with
    documents of {0, 1, 63, 64, 65, T - 1, T, T + 1, 3T + 7} distinct words (empty, one word, a full tile and
    both neighbours, four chunks with a partial last one);
  B in {1, W - 1, W, W + 1, 3W + 7};
  counts of 1, of several, of 1,000; word ids 0 and V - 1; unsorted word ids;
  max_doc_update_iter in {0, 1, 100}, and a tolerance no document reaches before the cap.
Every case is checked on the CPU (test_lda_ref.py) to keep each document's mean change at least 1e-6
(relative) from the tolerance at every update: the condition under which two correct implementations stop
at the same update.  A case that missed it would be re-seeded HERE; nothing is skipped at run time.
"""
import functools

import numpy as np

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import topic_infer

import lda_ref

T, W = topic_infer.TILE_WORDS, topic_infer.DOCS_PER_BLOCK
KS = (1, 3, 16, 50, 64, 65, 128)
LENGTHS = tuple(sorted({0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7}))
BATCHES = tuple(sorted({1, W - 1, W, W + 1, 3 * W + 7} - {0}))
MIN_MARGIN = 1e-6


def _model(rng, K, V):
    """A topic-word model with a few strong words a topic (gamma(0.3) draws): beta = exp(E[log beta])."""
    lam = rng.gamma(0.3, 1.0, (K, V)) + 0.01
    return lda_ref.exp_dirichlet(lam)


def _docs(rng, V, lengths, counts="several", sort=True):
    indptr, indices, data = [0], [], []
    for n in lengths:
        ids = rng.choice(V, n, replace=False)
        if sort:
            ids.sort()
        c = {"ones": np.ones(n), "several": rng.integers(1, 10, n), "thousand": np.full(n, 1000)}[counts]
        indices += ids.tolist()
        data += np.asarray(c).tolist()
        indptr.append(len(indices))
    return np.array(indptr, np.int32), np.array(indices, np.int32), np.array(data, np.float64)


def _case(name, K, V, lengths, seed, counts="several", sort=True, alpha=None, tol=1e-3, max_iter=100, edge_ids=False):
    rng = np.random.default_rng(seed)
    beta = _model(rng, K, V)
    indptr, indices, data = _docs(rng, V, lengths, counts, sort)
    if edge_ids:   # the first and last word of the vocabulary, alone and together
        extra = [[0], [V - 1], [0, V - 1], [V - 1, 0]]
        for ids in extra:
            indices = np.concatenate([indices, np.array(ids, np.int32)])
            data = np.concatenate([data, np.arange(1, len(ids) + 1, dtype=np.float64)])
            indptr = np.concatenate([indptr, np.array([indices.size], np.int32)])
    return dict(name=name, K=K, V=V, beta=beta, alpha=1.0 / K if alpha is None else alpha, tol=tol, max_iter=max_iter,
                indptr=indptr, indices=indices, counts=data)


def csr_of(has):
    """bool [B x V], which document holds which word -> (indptr, indices) int32, a document's words ascending."""
    indptr = np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int32)
    indices = np.concatenate([np.flatnonzero(r) for r in has]).astype(np.int32) if has.any() else np.zeros(0, np.int32)
    return indptr, indices


@functools.lru_cache(maxsize=None)
def table():
    """name -> case, in a fixed order."""
    cases = [_case(f"K{K}-lengths", K, 3 * T + 40, LENGTHS, seed=100 + K) for K in KS]
    cases += [_case(f"B{B}", 16, 120, [5 + (7 * i) % 36 for i in range(B)], seed=200 + B) for B in BATCHES]
    cases += [
        _case("counts-ones", 16, 150, [3, 20, T + 2], seed=301, counts="ones"),
        _case("counts-thousand", 16, 150, [3, 20, T + 2], seed=302, counts="thousand"),
        _case("edge-ids-unsorted", 50, 90, [12, 70], seed=303, sort=False, edge_ids=True),
        _case("cap0", 50, 200, [0, 9, T + 1], seed=304, max_iter=0),
        _case("cap1", 50, 200, [0, 9, T + 1], seed=305, max_iter=1),
        _case("cap3", 16, 200, [9, 30, T + 1], seed=306, max_iter=3),
        _case("never-converges", 16, 200, [9, 30, T + 1, 0], seed=307, tol=-1.0),   # (no mean change is < -1)
        _case("wide-prior", 3, 64, [1, 2, 17, 64], seed=308, alpha=0.7),
    ]
    return {c["name"]: c for c in cases}


NAMES = tuple(table())


@functools.lru_cache(maxsize=None)
def reference(name):
    """lda_ref.transform of the case: (theta, gamma, iters, margin); computed once, never written to."""
    c = table()[name]
    out = lda_ref.transform(c["indptr"], c["indices"], c["counts"], c["beta"], c["alpha"], c["tol"], c["max_iter"])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def golden_reference():
    """The same for the R8 fixture (tests/golden/lda_r8_small.npz)."""
    z = lda_ref.load_golden()
    out = lda_ref.transform(z["indptr"], z["indices"], z["counts"], z["exp_dirichlet_component_"],
                            float(z["doc_topic_prior_"]), float(z["mean_change_tol"]), int(z["max_doc_update_iter"]))
    for a in out:
        a.setflags(write=False)
    return out


def bound(iters):
    """Per document, max_k |theta_dev - theta_ref| <= 64 max(its, 1) 2^-52: reasoned, not measured.  An update
    adds a few roundings and <= 2-ulp exp / log per term, its sums hold at most a few hundred terms, and the
    converging map does not amplify what earlier updates left."""
    return 64.0 * np.maximum(np.asarray(iters, np.float64), 1.0) * 2.0 ** -52
