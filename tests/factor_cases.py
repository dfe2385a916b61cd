"""Hand-built doc-topic graphs and feature matrices for the hub factorisation
at the edges the generated graphs never reach (test infrastructure: numpy and
scipy only, no GPU import).

datasets.doc_topic_graph always puts the documents' features in columns 0 ..,
so every factor built from it has k0 == 0.  Here the documents' feature range
[k0, k0 + Kc) is chosen: k0 > 0 (and no multiple of 4: the dense X's light
rows are then read from a base 4 bytes off a 16-byte boundary), Kc = 1, past 64
(factor_u_kernel's second column per lane), 128 (the maximum) and 129
(refused), and documents with no feature at all (the (0, 1) fallback).

graph(): ndoc documents then ntopic topics, document d linked to the topics
(d + j) % ntopic for j < min_links + d % (max_links - min_links + 1), the
topics linked in a ring, A-hat = D^-1/2 (A + I) D^-1/2 in float64 rounded to
fp32.  The small graph (150 + 2, M = 152: five 32-row blocks, the last ragged)
meets the hub rule hmin = max(64, 8 ceil(nnz / M)) = 64 with topic rows of 152
and 77 nonzeros; the wide one (600 + 26) has 26 hubs of 72 or 73 nonzeros, enough
S_T rows to take Kc = 128, F = 256 past the factored kernel's LDS.
"""
from typing import NamedTuple, Optional

import numpy as np
import scipy.sparse as sp

NDOC, NTOPIC = 150, 2
WIDE_NDOC, WIDE_NTOPIC = 600, 26


def graph(ndoc=NDOC, ntopic=NTOPIC, min_links=1, max_links=2):
    M = ndoc + ntopic
    rows, cols = [], []
    for d in range(ndoc):
        for j in range(min_links + d % (max_links - min_links + 1)):
            t = ndoc + (d + j) % ntopic
            rows += [d, t]
            cols += [t, d]
    for t in range(ntopic):                            # hub-hub items
        u = (t + 1) % ntopic
        if u != t:
            rows += [ndoc + t, ndoc + u]
            cols += [ndoc + u, ndoc + t]
    A = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(M, M))
    A.data[:] = 1.0                                    # (the ring of two topics names its edge twice)
    A = A + sp.eye(M)
    dinv = 1.0 / np.sqrt(np.asarray(A.sum(1)).ravel())
    A = sp.csr_matrix(sp.diags(dinv) @ A @ sp.diags(dinv)).astype(np.float32)
    A.sort_indices()
    return A


def wide_graph():
    return graph(WIDE_NDOC, WIDE_NTOPIC, 3, 3)


class Config(NamedTuple):
    k0: int                 # the documents' feature range [k0, k0 + kc) ...
    kc: int
    K: int                  # ... of K columns
    per_doc: int            # nonzeros per document row (0: the documents have no feature)
    expect: Optional[tuple]  # (k0, Kc) of the factor, None: refused
    F: int = 0              # the GCN the forward test runs: hidden width, classes
    P: int = 0


CONFIGS = {
    "k0_0_kc1": Config(0, 1, 8, 1, (0, 1), 16, 3),
    "k0_37_kc50": Config(37, 50, 100, 5, (37, 50), 200, 8),
    "k0_3_kc65": Config(3, 65, 80, 6, (3, 65), 132, 20),
    "k0_1_kc128": Config(1, 128, 130, 8, (1, 128), 64, 8),
    "kc129": Config(0, 129, 129, 8, None),
    "light_zero": Config(0, 1, 8, 0, (0, 1), 32, 4),
}
ACCEPTED = [k for k, c in CONFIGS.items() if c.expect is not None]
# every config with a dense and a CSR X; one also with explicit zeros stored outside the range
RUNS = [(k, v) for k in CONFIGS for v in ("dense", "csr")] + [("k0_37_kc50", "csr_zeros")]


def features(name, ndoc=NDOC, ntopic=NTOPIC, explicit_zeros=False):
    """X [ndoc + ntopic x K] as a sorted scipy CSR (fp32): document 0 has column
    k0, document 1 column k0 + kc - 1, so the range is exact; the topic rows are
    half full over all K columns, outside the range too.  explicit_zeros: every
    third document also stores a 0.0 at column 0 or K - 1, outside the range."""
    c = CONFIGS[name]
    M = ndoc + ntopic
    rng = np.random.default_rng([c.k0, c.kc, c.K])
    X = sp.lil_matrix((M, c.K), dtype=np.float32)
    for d in range(ndoc if c.per_doc else 0):
        cols = c.k0 + rng.choice(c.kc, size=min(c.per_doc, c.kc), replace=False)
        if d == 0:
            cols[0] = c.k0
        elif d == 1:
            cols[0] = c.k0 + c.kc - 1
        for col in np.unique(cols):
            X[d, col] = np.float32(rng.uniform(0.1, 1.0) * rng.choice([-1.0, 1.0]))
    for t in range(ndoc, M):
        for col in np.flatnonzero(rng.random(c.K) < 0.5):
            X[t, col] = np.float32(rng.standard_normal())
    X = sp.csr_matrix(X)
    X.sort_indices()
    if explicit_zeros:
        assert c.k0 > 0 and c.k0 + c.kc < c.K
        zr = np.arange(0, ndoc, 3)
        Z = sp.csr_matrix((np.ones(len(zr)), (zr, np.where(np.arange(len(zr)) % 2, 0, c.K - 1))),
                          shape=(M, c.K), dtype=np.float32)
        S = (X + Z).tocsr()                            # the union pattern ...
        S.sort_indices()
        Zc = Z.tocoo()
        for r, col in zip(Zc.row, Zc.col):             # ... with 0.0 stored at the added places
            lo, hi = S.indptr[r], S.indptr[r + 1]
            S.data[lo + np.searchsorted(S.indices[lo:hi], col)] = 0.0
        assert S.nnz == X.nnz + Z.nnz and (S.data == 0).sum() == Z.nnz
        X = S
    return X
