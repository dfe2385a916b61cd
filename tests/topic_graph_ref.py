"""The doc-topic graph restated in numpy: what csrc/topic_graph.hip must produce, bit for bit.

The reference's path (build_graph.py:99-133 -> text edge list -> trainer.py:98-151): keep
theta[d, k] >= threshold compared in float64, keep sim[i, j] > threshold for i < j, store
both weights as float32, mirror every edge, then A-hat = D^-1/2 (A + I) D^-1/2 as
datasets.sym_normalize computes it (float64, sequential row sums in (row, col) order, one
rounding to fp32).  Every document and topic is a node whether or not it keeps an edge.
"""
import os

import numpy as np

from graph_convolutional_networks_for_text_classification_amd import datasets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r8_graph.npz")
R8_THRESHOLDS = (0.02, 0.3)


def build(theta, sim, doc_topic_threshold, topic_topic_threshold):
    """(rowptr int32[N+1], colind int32[nnz], val fp32[nnz], doc-topic edges, topic-topic edges)
    of A-hat for theta [D x K] and sim [K x K] or None (fp32 inputs widen exactly)."""
    theta = np.asarray(theta).astype(np.float64)
    D, K = theta.shape
    N = D + K
    with np.errstate(invalid="ignore"):
        d, k = np.nonzero(theta >= np.float64(doc_topic_threshold))
    w = theta[d, k].astype(np.float32)
    rows, cols, vals = [d, D + k], [D + k, d], [w, w]
    ntt = 0
    if sim is not None:
        sim = np.asarray(sim).astype(np.float64)
        i, j = np.triu_indices(K, 1)
        with np.errstate(invalid="ignore"):
            keep = sim[i, j] > np.float64(topic_topic_threshold)
        i, j = i[keep], j[keep]
        ww = sim[i, j].astype(np.float32)
        rows += [D + i, D + j]
        cols += [D + j, D + i]
        vals += [ww, ww]
        ntt = int(i.size)
    rr, cc, vv = datasets.sym_normalize(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), N)
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rr, minlength=N))
    return rowptr.astype(np.int32), cc.astype(np.int32), vv.astype(np.float32), int(d.size), ntt


def r8_inputs(path=GOLDEN):
    """(theta [D x K] float64, sim [K x K] float64, D, K) holding R8's KEPT entries, from the
    raw adjacency the reference built (a_row / a_col / a_val of the fixture): the kept theta
    and the topic block's similarities at their float32 weights, zero elsewhere."""
    z = np.load(path, allow_pickle=False)
    N, _, D, K, _ = (int(v) for v in z["shape"])
    r, c, v = z["a_row"].astype(np.int64), z["a_col"].astype(np.int64), z["a_val"].astype(np.float64)
    theta = np.zeros((D, K), np.float64)
    dt = (r < D) & (c >= D)
    theta[r[dt], c[dt] - D] = v[dt]
    sim = np.zeros((K, K), np.float64)
    tt = (r >= D) & (c >= D)
    sim[r[tt] - D, c[tt] - D] = v[tt]
    return theta, sim, D, K


def r8_golden(path=GOLDEN):
    """The reference's A-hat of R8 sorted by (row, col): (rowptr, colind, val)."""
    z = np.load(path, allow_pickle=False)
    N = int(z["shape"][0])
    r, c, v = z["adj_row"].astype(np.int64), z["adj_col"].astype(np.int64), z["adj_val"].astype(np.float32)
    order = np.lexsort((c, r))
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=N))
    return rowptr.astype(np.int32), c[order].astype(np.int32), v[order]


def dirichlet_theta(D, K, seed):
    return np.random.default_rng(seed).dirichlet(np.full(K, 1.0 / K), size=D)


def uniform_sim(K, seed):
    u = np.random.default_rng(seed).random((K, K))
    return np.triu(u, 1) + np.triu(u, 1).T + np.eye(K)


def cosine(emb):
    """numpy float64: rows normalised (a zero row stays zero), then the Gram matrix."""
    e = np.asarray(emb).astype(np.float64)
    n = np.sqrt((e * e).sum(1, keepdims=True))
    e = e / np.where(n == 0, 1.0, n)
    return e @ e.T
