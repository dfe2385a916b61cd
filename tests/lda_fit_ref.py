"""sklearn's batch variational EM for LDA (LatentDirichletAllocation.fit, learning_method='batch', which the
reference calls in topic_model.py:109-117), restated in float64 numpy on tests/lda_ref.py's psi, seq_sum and
exp_dirichlet.  One EM iteration (_lda.py _em_step(batch_update=True)):

    beta    = exp(psi(lambda_kw) - psi(sum_w lambda_kw))                     (lda_ref.exp_dirichlet)
    E-step  per document, from a FRESH gamma0 ~ Gamma(100, .01) draw (random_init=True):
            etheta = exp(psi(gamma0_k) - psi(sum_k gamma0_k)), then transform's update loop unchanged; after
            the loop ONCE MORE  phi_w = sum_k etheta_k beta_kw + eps,  r_w = c_w / phi_w  with the final etheta
    M-step  S_kw = sum_d etheta_dk r_dw, documents ascending, the product rounded and then added (np.outer,
            then +=);  lambda_kw = eta + S_kw beta_kw

Sums over topics ascend in k, sums over a document's words run in stored order, sums over documents ascend
in d.  A document's word ids are distinct (a CSR row of a document-term matrix).
"""
import os

import numpy as np

from lda_ref import EPS, exp_dirichlet, psi, seq_sum

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lda_fit_r8_small.npz")


def estep_fit(indptr, indices, counts, exp_topic_word, gamma0, alpha, tol=1e-3, max_iter=100):
    """-> gamma [B x K], etheta [B x K], ratio [nnz] (CSR order), iterations int32 [B], margin [B] (inf: no
    update ran).  margin is lda_ref.transform's: min over a document's updates of |mean change - tol| / |tol|."""
    beta = np.asarray(exp_topic_word, np.float64)
    K = beta.shape[0]
    B = len(indptr) - 1
    gamma = np.array(gamma0, np.float64).reshape(B, K).copy()
    etheta = np.empty((B, K), np.float64)
    ratio = np.zeros(int(indptr[-1]), np.float64)
    iters = np.zeros(B, np.int32)
    margin = np.full(B, np.inf)
    for d in range(B):
        lo, hi = int(indptr[d]), int(indptr[d + 1])
        ids = np.asarray(indices[lo:hi], np.int64)
        c = np.asarray(counts[lo:hi], np.float64)
        bt = np.ascontiguousarray(beta[:, ids].T)      # [n x K]
        g = gamma[d].copy()
        et = np.exp(psi(g) - psi(seq_sum(g))[0])
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
        etheta[d] = et
        if len(ids):
            ratio[lo:hi] = c / (seq_sum(bt * et, axis=1) + EPS)
    return gamma, etheta, ratio, iters, margin


def mstep(indptr, indices, ratio, etheta, exp_topic_word, eta):
    """lambda [K x V]: word by word, down the word's documents in ascending order, s = s + (etheta_dk * r),
    multiply then add; then eta + s * beta.  A word no document holds gets exactly eta."""
    beta = np.asarray(exp_topic_word, np.float64)
    K, V = beta.shape
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    doc_of = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    order = np.argsort(indices, kind="stable")         # word-major, a word's entries in ascending document order
    starts = np.searchsorted(indices[order], np.arange(V + 1))
    lam = np.empty((K, V), np.float64)
    for w in range(V):
        s = np.zeros(K, np.float64)
        for i in order[starts[w]:starts[w + 1]]:
            prod = etheta[doc_of[i]] * ratio[i]
            s = s + prod
        lam[:, w] = eta + s * beta[:, w]
    return lam


def fit(indptr, indices, counts, lambda0, gamma0s, alpha, eta, tol=1e-3, max_doc_update_iter=100):
    """len(gamma0s) EM iterations from lambda0 -> lambda [K x V], iterations int32 [max_iter x B], the smallest
    stop margin of any document in any EM iteration."""
    lam = np.array(lambda0, np.float64)
    counts_of, margin = [], np.inf
    for g0 in gamma0s:
        beta = exp_dirichlet(lam)
        _, etheta, ratio, iters, m = estep_fit(indptr, indices, counts, beta, g0, alpha, tol, max_doc_update_iter)
        lam = mstep(indptr, indices, ratio, etheta, beta, eta)
        counts_of.append(iters)
        margin = min(margin, float(m.min()))
    return lam, np.stack(counts_of).astype(np.int32), margin


def draws(random_state, K, V, B, max_iter):
    """sklearn's host draws in its order: lambda0 [K x V], then gamma0 [max_iter x B x K] in ONE call (the same
    stream as max_iter successive (B, K) draws)."""
    rs = np.random.RandomState(random_state)
    lam0 = rs.gamma(100.0, 0.01, (K, V))
    return lam0, rs.gamma(100.0, 0.01, (max_iter, B, K))


def permuted(indptr, indices, counts, seed=0):
    """The same documents, every document's words in a random order."""
    rng = np.random.default_rng(seed)
    indices, counts = np.array(indices), np.array(counts)
    for d in range(len(indptr) - 1):
        lo, hi = int(indptr[d]), int(indptr[d + 1])
        p = lo + rng.permutation(hi - lo)
        indices[lo:hi], counts[lo:hi] = indices[p], counts[p]
    return indices, counts


def max_rel(a, b):
    return float((np.abs(np.asarray(a) - b) / np.abs(b)).max())


def load_golden():
    """tests/golden/lda_fit_r8_small.npz (make_lda_fit_golden.py) as a dict of arrays."""
    return dict(np.load(GOLDEN, allow_pickle=False))
