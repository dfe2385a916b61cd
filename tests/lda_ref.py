"""The LDA E-step that csrc/lda_estep.hip runs, restated in float64 numpy from sklearn's rules
(LatentDirichletAllocation.transform, which the reference calls in topic_model.py:133-164):

  * psi is Bernardo's AS 103 as sklearn's _online_lda_fast.pyx states it (NOT an accurate digamma);
  * transform starts every document at gamma = 1, so exp(E[log theta]) = exp(psi(1) - psi(K));
  * an update is  phi_w = sum_k etheta_k beta_kw + eps,  gamma'_k = etheta_k sum_w (c_w / phi_w) beta_kw + alpha,
    etheta_k = exp(psi(gamma'_k) - psi(sum_k gamma'_k));
  * the loop ends after the update whose mean change sum_k |gamma_k - gamma'_k| / K is < mean_change_tol,
    or after max_doc_update_iter updates;  theta = gamma / sum_k gamma.

Sums over topics are taken in ascending k, sums over a document's words in stored order.  Besides theta,
gamma and the number of updates, ``transform`` returns each document's stop margin
min over its updates of |mean change - tol| / |tol|: a document is a fair test of "equal iteration counts"
only when that margin is far above rounding.
"""
import os

import numpy as np

EULER = 0.577215664901532860606512090082402431
EPS = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lda_r8_small.npz")


def psi(x):
    """AS 103, elementwise on a float64 array (or scalar), sklearn's operation order."""
    x = np.array(x, dtype=np.float64, ndmin=1)
    small = x <= 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        out_small = -EULER - 1.0 / x
        result = np.zeros_like(x)
        y = x.copy()
        for _ in range(6):            # x > 1e-6 reaches 6 after at most six shifts
            m = (y < 6) & ~small
            if not m.any():
                break
            result[m] -= 1.0 / y[m]
            y[m] += 1
        r = 1.0 / y
        result = result + (np.log(y) - 0.5 * r)
        r = r * r
        result = result - r * ((1.0 / 12.0) - r * ((1.0 / 120.0) - r * (1.0 / 252.0)))
    return np.where(small, out_small, result)


def seq_sum(a, axis=-1):
    """Sum along ``axis`` strictly in ascending index order (numpy's own sum is pairwise)."""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    s = np.zeros(a.shape[1:], np.float64)
    for row in a:
        s = s + row
    return s


def exp_dirichlet(components):
    """exp(psi(lambda_kw) - psi(sum_w lambda_kw)) [K x V]: sklearn's _dirichlet_expectation_2d plus exp,
    the row sum serial and ascending in w."""
    lam = np.asarray(components, np.float64)
    rows = np.cumsum(lam, axis=1)[:, -1]     # (cumsum IS sequential)
    return np.exp(psi(lam.ravel()).reshape(lam.shape) - psi(rows)[:, None])


def transform(indptr, indices, counts, exp_topic_word, alpha, tol=1e-3, max_iter=100):
    """-> theta [B x K], gamma [B x K], iterations int32 [B], margin float64 [B] (inf: no update ran)."""
    beta = np.asarray(exp_topic_word, np.float64)
    K = beta.shape[0]
    B = len(indptr) - 1
    gamma = np.ones((B, K), np.float64)
    iters = np.zeros(B, np.int32)
    margin = np.full(B, np.inf)
    e0 = np.exp(psi(1.0) - psi(float(K)))[0]
    for d in range(B):
        ids = np.asarray(indices[indptr[d]:indptr[d + 1]], np.int64)
        c = np.asarray(counts[indptr[d]:indptr[d + 1]], np.float64)
        bt = np.ascontiguousarray(beta[:, ids].T)      # [n x K]
        g = gamma[d].copy()
        et = np.full(K, e0)
        for _ in range(max_iter):
            phi = seq_sum(bt * et, axis=1) + EPS if len(ids) else np.zeros(0)
            acc = seq_sum(bt * (c / phi)[:, None], axis=0) if len(ids) else np.zeros(K)
            new = et * acc + alpha
            total = seq_sum(new)
            et = np.exp(psi(new) - psi(total)[0])
            change = seq_sum(np.abs(g - new)) / K
            g = new
            iters[d] += 1
            margin[d] = min(margin[d], abs(change - tol) / abs(tol))
            if change < tol:
                break
        gamma[d] = g
    theta = gamma / seq_sum(gamma, axis=1)[:, None]
    return theta, gamma, iters, margin


def load_golden():
    """tests/golden/lda_r8_small.npz (make_lda_golden.py) as a dict of arrays."""
    return dict(np.load(GOLDEN, allow_pickle=False))
