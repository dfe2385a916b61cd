"""sklearn's online variational EM for LDA (LatentDirichletAllocation with learning_method='online', and
partial_fit; _lda.py _em_step(batch_update=False), which the reference's TopicModel offers as learning_method,
topic_model.py:46,55,113), restated in float64 numpy on tests/lda_fit_ref.py's E-step and tests/lda_ref.py's
exp_dirichlet.  One minibatch of documents [doc_lo, doc_hi), n = sklearn's n_batch_iter_ (1 at the start):

    beta    = exp_dirichlet(lambda)                                           (after every minibatch)
    E-step  lda_fit_ref.estep_fit of the minibatch's documents, from their rows of a fresh gamma0 draw
    M-step  rho = np.power(learning_offset + n, -learning_decay)
            S_kw = sum over the minibatch's documents d, ascending, of etheta_dk r_dw  (product rounded, then added)
            lambda_kw = lambda_kw (1 - rho) + rho (eta + doc_ratio (S_kw beta_kw)),  doc_ratio = total / (doc_hi - doc_lo)
            n += 1

Every word is blended, held by the minibatch or not.  fit() walks gen_batches(B, batch_size) slices max_iter
times with total = B; partial_fit() walks them once with total = total_samples.
"""
import os

import numpy as np

import lda_fit_ref
from lda_ref import exp_dirichlet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lda_online_r8_small.npz")


def rho_of(learning_offset, n, learning_decay):
    return float(np.power(learning_offset + n, -learning_decay))


def batches(B, batch_size):
    """sklearn.utils.gen_batches(B, batch_size) as (b0, b1) pairs."""
    return [(b0, min(b0 + batch_size, B)) for b0 in range(0, B, batch_size)]


def mstep_online(indptr, indices, ratio, etheta, beta, lam, eta, rho, doc_ratio, doc_lo, doc_hi):
    """-> the new lambda [K x V] (lam is left as it is).  indptr / indices / ratio / etheta are the WHOLE
    matrix's; only the documents [doc_lo, doc_hi) enter the sums.  The serial loop, one rounded operation a line."""
    beta, lam = np.asarray(beta, np.float64), np.asarray(lam, np.float64)
    K, V = beta.shape
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    doc_of = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    order = np.argsort(indices, kind="stable")         # word-major, a word's entries in ascending document order
    starts = np.searchsorted(indices[order], np.arange(V + 1))
    rho, doc_ratio, eta = np.float64(rho), np.float64(doc_ratio), np.float64(eta)
    keep = np.float64(1.0) - rho
    out = np.empty((K, V), np.float64)
    for w in range(V):
        s = np.zeros(K, np.float64)
        for i in order[starts[w]:starts[w + 1]]:
            d = doc_of[i]
            if doc_lo <= d < doc_hi:
                prod = etheta[d] * ratio[i]
                s = s + prod
        ss = s * beta[:, w]
        t = doc_ratio * ss
        u = eta + t
        v = rho * u
        a = lam[:, w] * keep
        out[:, w] = a + v
    return out


def _walk(indptr, indices, counts, lam, gamma0, alpha, eta, total, batch_size, decay, offset, n, tol, cap):
    """One walk over the documents in minibatches -> lambda, iterations int32 [B], smallest margin, n."""
    indptr = np.asarray(indptr, np.int64)
    B = len(indptr) - 1
    K = lam.shape[0]
    iters = np.zeros(B, np.int32)
    margin = np.inf
    ratio = np.zeros(int(indptr[-1]), np.float64)
    etheta = np.zeros((B, K), np.float64)
    for b0, b1 in batches(B, batch_size):
        beta = exp_dirichlet(lam)
        lo, hi = int(indptr[b0]), int(indptr[b1])
        _, et, r, its, m = lda_fit_ref.estep_fit(indptr[b0:b1 + 1] - lo, indices[lo:hi], counts[lo:hi], beta,
                                                 gamma0[b0:b1], alpha, tol, cap)
        etheta[b0:b1], ratio[lo:hi], iters[b0:b1] = et, r, its
        margin = min(margin, float(m.min()))
        lam = mstep_online(indptr, indices, ratio, etheta, beta, lam, eta, rho_of(offset, n, decay),
                           float(total) / (b1 - b0), b0, b1)
        n += 1
    return lam, iters, margin, n


def fit_online(indptr, indices, counts, lambda0, gamma0s, alpha, eta, batch_size=128, learning_decay=0.7,
               learning_offset=10.0, tol=1e-3, max_doc_update_iter=100):
    """len(gamma0s) EM iterations from lambda0 (gamma0s [max_iter x B x K]: sklearn's stream, rows [b0, b1) of
    iteration it are that minibatch's draw) -> lambda, iterations int32 [max_iter x B], smallest stop margin,
    n_batch_iter_."""
    lam = np.array(lambda0, np.float64)
    B = len(indptr) - 1
    counts_of, margin, n = [], np.inf, 1
    for g0 in gamma0s:
        lam, iters, m, n = _walk(indptr, indices, counts, lam, g0, alpha, eta, B, batch_size, learning_decay,
                                 learning_offset, n, tol, max_doc_update_iter)
        counts_of.append(iters)
        margin = min(margin, m)
    return lam, np.stack(counts_of).astype(np.int32), margin, n


def partial_fit(indptr, indices, counts, lam, gamma0, alpha, eta, total_samples, n=1, batch_size=128,
                learning_decay=0.7, learning_offset=10.0, tol=1e-3, max_doc_update_iter=100):
    """sklearn's partial_fit of these documents on the model lam at n_batch_iter_ = n (gamma0 [B x K]) ->
    lambda, iterations int32 [B], smallest stop margin, the new n_batch_iter_."""
    return _walk(indptr, indices, counts, np.array(lam, np.float64), gamma0, alpha, eta, total_samples, batch_size,
                 learning_decay, learning_offset, n, tol, max_doc_update_iter)


def load_golden():
    """tests/golden/lda_online_r8_small.npz (make_lda_online_golden.py) as a dict of arrays."""
    return dict(np.load(GOLDEN, allow_pickle=False))
