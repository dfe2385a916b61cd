"""What csrc/lda_estep.hip runs, restated in float64 numpy from sklearn's rules: the E-step, the M-step of both
fits and the loops around them.  Every rule is stated ONCE here: ``estep`` is the update loop of transform and
of both fits, ``word_chains`` the M-step sum of the batch and the online method.

The E-step (LatentDirichletAllocation.transform, which the reference calls in topic_model.py:133-164):

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

The batch fit (LatentDirichletAllocation.fit, learning_method='batch', which the reference calls in
topic_model.py:109-117).  One EM iteration (_lda.py _em_step(batch_update=True)):

    beta    = exp(psi(lambda_kw) - psi(sum_w lambda_kw))                     (exp_dirichlet)
    E-step  per document, from a FRESH gamma0 ~ Gamma(100, .01) draw (random_init=True):
            etheta = exp(psi(gamma0_k) - psi(sum_k gamma0_k)), then transform's update loop unchanged; after
            the loop ONCE MORE  phi_w = sum_k etheta_k beta_kw + eps,  r_w = c_w / phi_w  with the final etheta
    M-step  S_kw = sum_d etheta_dk r_dw, documents ascending, the product rounded and then added (np.outer,
            then +=);  lambda_kw = eta + S_kw beta_kw

The online fit (learning_method='online', and partial_fit; _em_step(batch_update=False), which the reference's
TopicModel offers as learning_method, topic_model.py:46,55,113).  One minibatch of documents [doc_lo, doc_hi),
n = sklearn's n_batch_iter_ (1 at the start):

    beta    = exp_dirichlet(lambda)                                           (after every minibatch)
    E-step  of the minibatch's documents, from their rows of a fresh gamma0 draw
    M-step  rho = np.power(learning_offset + n, -learning_decay)
            S_kw as above over the minibatch's documents alone
            lambda_kw = lambda_kw (1 - rho) + rho (eta + doc_ratio (S_kw beta_kw)),  doc_ratio = total / (doc_hi - doc_lo)
            n += 1

Every word is blended, held by the minibatch or not.  fit_online() walks gen_batches(B, batch_size) slices
max_iter times with total = B; partial_fit() walks them once with total = total_samples.  Sums over documents
ascend in d; a document's word ids are distinct (a CSR row of a document-term matrix).
"""
import os

import numpy as np

EULER = 0.577215664901532860606512090082402431
EPS = float(np.finfo(np.float64).eps)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def estep(indptr, indices, counts, exp_topic_word, gamma0, alpha, tol=1e-3, max_iter=100):
    """The update loop from gamma0 [B x K] -> gamma [B x K], etheta [B x K], ratio [nnz] (CSR order, c_w / phi_w
    under the final etheta), iterations int32 [B], margin [B] (inf: no update ran)."""
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


def transform(indptr, indices, counts, exp_topic_word, alpha, tol=1e-3, max_iter=100):
    """-> theta [B x K], gamma [B x K], iterations int32 [B], margin float64 [B] (inf: no update ran)."""
    ones = np.ones((len(indptr) - 1, np.shape(exp_topic_word)[0]), np.float64)
    gamma, _, _, iters, margin = estep(indptr, indices, counts, exp_topic_word, ones, alpha, tol, max_iter)
    theta = gamma / seq_sum(gamma, axis=1)[:, None]
    return theta, gamma, iters, margin


def word_chains(indptr, indices, ratio, etheta, V, doc_lo=None, doc_hi=None):
    """S [K x V]: word by word, down the word's documents in ascending order (those in [doc_lo, doc_hi) alone,
    where given), s = s + (etheta_dk * r), multiply then add.  A word no such document holds gets exactly 0."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    doc_of = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    order = np.argsort(indices, kind="stable")         # word-major, a word's entries in ascending document order
    starts = np.searchsorted(indices[order], np.arange(V + 1))
    K = np.shape(etheta)[1]
    S = np.empty((K, V), np.float64)
    for w in range(V):
        s = np.zeros(K, np.float64)
        for i in order[starts[w]:starts[w + 1]]:
            d = doc_of[i]
            if doc_lo is None or doc_lo <= d < doc_hi:
                prod = etheta[d] * ratio[i]
                s = s + prod
        S[:, w] = s
    return S


def mstep(indptr, indices, ratio, etheta, exp_topic_word, eta):
    """lambda [K x V] = eta + S * beta.  A word no document holds gets exactly eta."""
    beta = np.asarray(exp_topic_word, np.float64)
    return eta + word_chains(indptr, indices, ratio, etheta, beta.shape[1]) * beta


def mstep_online(indptr, indices, ratio, etheta, beta, lam, eta, rho, doc_ratio, doc_lo, doc_hi):
    """-> the new lambda [K x V] (lam is left as it is).  indptr / indices / ratio / etheta are the WHOLE
    matrix's; only the documents [doc_lo, doc_hi) enter the sums.  One rounded operation a line."""
    beta, lam = np.asarray(beta, np.float64), np.asarray(lam, np.float64)
    rho, doc_ratio, eta = np.float64(rho), np.float64(doc_ratio), np.float64(eta)
    keep = np.float64(1.0) - rho
    ss = word_chains(indptr, indices, ratio, etheta, beta.shape[1], doc_lo, doc_hi) * beta
    t = doc_ratio * ss
    u = eta + t
    v = rho * u
    a = lam * keep
    return a + v


def fit(indptr, indices, counts, lambda0, gamma0s, alpha, eta, tol=1e-3, max_doc_update_iter=100):
    """len(gamma0s) EM iterations from lambda0 -> lambda [K x V], iterations int32 [max_iter x B], the smallest
    stop margin of any document in any EM iteration."""
    lam = np.array(lambda0, np.float64)
    counts_of, margin = [], np.inf
    for g0 in gamma0s:
        beta = exp_dirichlet(lam)
        _, etheta, ratio, iters, m = estep(indptr, indices, counts, beta, g0, alpha, tol, max_doc_update_iter)
        lam = mstep(indptr, indices, ratio, etheta, beta, eta)
        counts_of.append(iters)
        margin = min(margin, float(m.min()))
    return lam, np.stack(counts_of).astype(np.int32), margin


def rho_of(learning_offset, n, learning_decay):
    return float(np.power(learning_offset + n, -learning_decay))


def batches(B, batch_size):
    """sklearn.utils.gen_batches(B, batch_size) as (b0, b1) pairs."""
    return [(b0, min(b0 + batch_size, B)) for b0 in range(0, B, batch_size)]


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
        _, et, r, its, m = estep(indptr[b0:b1 + 1] - lo, indices[lo:hi], counts[lo:hi], beta, gamma0[b0:b1], alpha, tol,
                                 cap)
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


def _load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name), allow_pickle=False))


def load_golden():
    """tests/golden/lda_r8_small.npz (make_lda_golden.py) as a dict of arrays."""
    return _load("lda_r8_small.npz")


def load_fit_golden():
    """tests/golden/lda_fit_r8_small.npz (make_lda_fit_golden.py) as a dict of arrays."""
    return _load("lda_fit_r8_small.npz")


def load_online_golden():
    """tests/golden/lda_online_r8_small.npz (make_lda_online_golden.py) as a dict of arrays."""
    return _load("lda_online_r8_small.npz")
