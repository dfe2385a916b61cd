"""The variational bound of csrc/lda_estep.hip (gcnk_lda_bound_*_f64) restated in float64 numpy from sklearn's
rules (_lda.py _approx_bound, score, _perplexity_precomp_distr), on lda_ref's psi and seq_sum.

    l_dk = psi(gamma_dk) - psi(sum_k gamma_dk)          b_kw = psi(lambda_kw) - psi(sum_w lambda_kw)
    doc_d   = sum_w c_dw logsumexp_k(l_dk + b_kw) + sum_k (alpha - gamma_dk) l_dk
            + sum_k (lgamma(gamma_dk) - lgamma(alpha)) + lgamma(alpha K) - lgamma(sum_k gamma_dk)
    topic_k = sum_w (eta - lambda_kw) b_kw + sum_w (lgamma(lambda_kw) - lgamma(eta))
            + lgamma(eta V) - lgamma(sum_w lambda_kw)
    bound   = doc_ratio sum_d doc_d + sum_k topic_k      perplexity = exp(-bound / (doc_ratio sum c))

The logsumexp here is the real one over the LOG-domain b (scipy's unless another is given): the device's shifted
form over the exp table is what is under test.  The summation orders are the ones include/gcnk_lda.h
documents: sums over k ascend; a document's words in tiles of 64, a tile by the wave tree, the tiles one after the
other; a topic's words dealt to 256 threads (thread t: words t, t + 256, ... ascending), then the block tree; the
final sums dealt to 1024 threads the same way.

Beside every value comes A, the sum of the absolute values of the addends it was formed from: every c lse, every
(prior - x) E[log x] and every lgamma TAKEN, each by its own size.  (A difference lgamma(x) - lgamma(prior) carries
the roundings of both values however small it is itself: counted as one addend, a gamma row equal to alpha -- what
the E-step gives a document without a word -- would have A = 0 and no rounding at all would be near.  On the R8
fixture A is 3.49e5 this way and 3.05e5 with the differences counted once.)  A distance between two evaluations
of the same quantity is |x - y| / (2^-52 A): the roundings of full-size addends that separate them.
"""
import math

import numpy as np
from scipy.special import gammaln, logsumexp

import lda_ref

ULP = 2.0 ** -52
TILE, TOPIC_CHUNK, FINISH_THREADS = 64, 256, 1024


class Functions:
    """The library functions an evaluation uses: (lgamma, logsumexp over axis 0)."""

    def __init__(self, lgamma, lse):
        self.lgamma, self.lse = lgamma, lse


def _shift_lse(a):
    """A hand-written max-shift logsumexp over axis 0."""
    m = a.max(axis=0)
    return m + np.log(lda_ref.seq_sum(np.exp(a - m), axis=0))


SCIPY = Functions(lambda x: gammaln(np.asarray(x, np.float64)), lambda a: logsumexp(a, axis=0))
LIBM = Functions(np.vectorize(math.lgamma, otypes=[np.float64]), _shift_lse)


def wave_tree(v):
    """64 values (fewer: +0 follows) in adjacent pairs, then those sums in pairs, six levels."""
    a = np.zeros(64, np.float64)
    a[:len(v)] = v
    while a.size > 1:
        a = a[0::2] + a[1::2]
    return float(a[0])


def block_tree(per_thread):
    """Each wave's tree, then the waves' sums one after the other in ascending wave order."""
    waves = [wave_tree(per_thread[i:i + 64]) for i in range(0, len(per_thread), 64)]
    return float(lda_ref.seq_sum(np.array(waves)))


def dealt_sum(values, nthreads):
    """Thread t adds the elements t, t + nthreads, ... ascending, then the block tree."""
    values = np.asarray(values, np.float64)
    return block_tree(np.array([float(lda_ref.seq_sum(values[t::nthreads])) for t in range(nthreads)]))


def elog_beta(lam):
    """b [K x V], the row sum serial and ascending in w -> b, the row sums."""
    lam = np.asarray(lam, np.float64)
    rows = np.cumsum(lam, axis=1)[:, -1]
    return lda_ref.psi(lam.ravel()).reshape(lam.shape) - lda_ref.psi(rows)[:, None], rows


def doc_parts(indptr, indices, counts, gamma, lam, alpha, fn=SCIPY):
    """-> doc_bound [B], A [B]."""
    b, _ = elog_beta(lam)
    gamma = np.asarray(gamma, np.float64)
    B, K = gamma.shape
    out, A = np.zeros(B), np.zeros(B)
    lg_alpha, lg_alpha_K = float(fn.lgamma(alpha)), float(fn.lgamma(alpha * K))
    for d in range(B):
        g = gamma[d]
        total = float(lda_ref.seq_sum(g))
        l = lda_ref.psi(g) - lda_ref.psi(total)[0]
        lo, hi = int(indptr[d]), int(indptr[d + 1])
        c = np.asarray(counts[lo:hi], np.float64)
        words = 0.0
        terms = np.zeros(0)
        if hi > lo:
            terms = c * fn.lse(l[:, None] + b[:, np.asarray(indices[lo:hi], np.int64)])
            for t0 in range(0, hi - lo, TILE):
                words = words + wave_tree(terms[t0:t0 + TILE])
        a1 = (alpha - g) * l
        lg = fn.lgamma(g)
        s1, s2 = float(lda_ref.seq_sum(a1)), float(lda_ref.seq_sum(lg - lg_alpha))
        lg_total = float(fn.lgamma(total))
        out[d] = ((words + s1) + s2) + (lg_alpha_K - lg_total)
        A[d] = np.abs(terms).sum() + np.abs(a1).sum() + np.abs(lg).sum() + K * abs(lg_alpha) + abs(lg_alpha_K) + abs(lg_total)
    return out, A


def topic_parts(lam, eta, fn=SCIPY):
    """-> topic_bound [K], A [K]."""
    lam = np.asarray(lam, np.float64)
    K, V = lam.shape
    b, rows = elog_beta(lam)
    out, A = np.zeros(K), np.zeros(K)
    lg_eta, lg_eta_V = float(fn.lgamma(eta)), float(fn.lgamma(eta * V))
    for k in range(K):
        a1 = (eta - lam[k]) * b[k]
        lg = fn.lgamma(lam[k])
        lg_row = float(fn.lgamma(rows[k]))
        out[k] = (dealt_sum(a1, TOPIC_CHUNK) + dealt_sum(lg - lg_eta, TOPIC_CHUNK)) + (lg_eta_V - lg_row)
        A[k] = np.abs(a1).sum() + np.abs(lg).sum() + V * abs(lg_eta) + abs(lg_eta_V) + abs(lg_row)
    return out, A


def finish(doc_bound, A_doc, topic_bound, A_topic, counts, doc_ratio=1.0):
    """-> bound, word count, perplexity, A of the bound."""
    docs, topics = dealt_sum(doc_bound, FINISH_THREADS), dealt_sum(topic_bound, FINISH_THREADS)
    counts = np.asarray(counts)
    count = float(counts.sum()) if counts.dtype.kind in "iu" else dealt_sum(counts, FINISH_THREADS)
    bound = doc_ratio * docs + topics
    A = doc_ratio * float(np.sum(A_doc)) + float(np.sum(A_topic))
    with np.errstate(divide="ignore", over="ignore"):      # (no word at all: x / 0, as the device divides)
        perplexity = float(np.exp(-1.0 * (np.float64(bound) / np.float64(count * doc_ratio))))
    return bound, count, perplexity, A


def evaluate(indptr, indices, counts, gamma, lam, alpha, eta, doc_ratio=1.0, fn=SCIPY):
    """-> dict(doc, A_doc, topic, A_topic, bound, count, perplexity, A) of documents [indptr[0], indptr[-1])."""
    doc, A_doc = doc_parts(indptr, indices, counts, gamma, lam, alpha, fn)
    topic, A_topic = topic_parts(lam, eta, fn)
    bound, count, perp, A = finish(doc, A_doc, topic, A_topic, counts[int(indptr[0]):int(indptr[-1])], doc_ratio)
    return dict(doc=doc, A_doc=A_doc, topic=topic, A_topic=A_topic, bound=bound, count=count, perplexity=perp, A=A)


def gamma_of(indptr, indices, counts, lam, alpha, tol=1e-3, max_iter=100):
    """sklearn's _unnormalized_transform under lambda: lda_ref's E-step from gamma = 1."""
    return lda_ref.transform(indptr, indices, counts, lda_ref.exp_dirichlet(lam), alpha, tol, max_iter)[1]


def score(indptr, indices, counts, lam, alpha, eta, tol=1e-3, max_iter=100, fn=SCIPY):
    """evaluate() at gamma_of(): sklearn's score (``bound``) and perplexity."""
    gamma = gamma_of(indptr, indices, counts, lam, alpha, tol, max_iter)
    return evaluate(indptr, indices, counts, gamma, lam, alpha, eta, 1.0, fn)


def distance(x, y, A):
    """max |x - y| / (2^-52 A), element by element; where A is 0 (every addend is) only equality is near."""
    diff, A = np.abs(np.asarray(x, np.float64) - y), np.asarray(A, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(A > 0, diff / (ULP * A), np.where(diff == 0, 0.0, np.inf))))


def distances(a, b):
    """(of the partials, of the bound) between two evaluate() results; A is the first one's."""
    parts = max(distance(a["doc"], b["doc"], a["A_doc"]), distance(a["topic"], b["topic"], a["A_topic"]))
    return parts, distance(a["bound"], b["bound"], a["A"])


def relabelled(indptr, indices, counts, lam, seed):
    """The same model and documents with the vocabulary renumbered at random and every document's words in a
    random order: every sum over words, a document's and a topic's, in another order."""
    rng = np.random.default_rng(seed)
    V = np.shape(lam)[1]
    new_id = rng.permutation(V)
    lam2 = np.empty_like(np.asarray(lam, np.float64))
    lam2[:, new_id] = lam
    ix, ct = lda_ref.permuted(indptr, new_id[np.asarray(indices, np.int64)].astype(np.int32), counts, seed)
    return ix, ct, lam2


def evaluate_every(indptr, indices, counts, lambda0, gamma0s, alpha, eta, every, perp_tol, learning_method="batch",
                   batch_size=128, learning_decay=0.7, learning_offset=10.0, tol=1e-3, cap=100):
    """sklearn's fit loop with evaluate_every, restated on lda_ref's EM steps -> lambda, n_iter_, the perplexities
    evaluated, the closing perplexity (bound_), n_batch_iter_."""
    lam = np.array(lambda0, np.float64)
    B = len(indptr) - 1
    perps, last, n_iter, n = [], None, 0, 1
    for i, g0 in enumerate(gamma0s):
        if learning_method == "online":
            lam, _, _, n = lda_ref._walk(indptr, indices, counts, lam, g0, alpha, eta, B, batch_size, learning_decay,
                                         learning_offset, n, tol, cap)
        else:
            beta = lda_ref.exp_dirichlet(lam)
            _, etheta, ratio, _, _ = lda_ref.estep(indptr, indices, counts, beta, g0, alpha, tol, cap)
            lam = lda_ref.mstep(indptr, indices, ratio, etheta, beta, eta)
            n += 1
        if every > 0 and (i + 1) % every == 0:
            p = score(indptr, indices, counts, lam, alpha, eta, tol, cap)["perplexity"]
            perps.append(p)
            if last and abs(last - p) < perp_tol:
                break
            last = p
        n_iter += 1
    return lam, n_iter, np.array(perps), score(indptr, indices, counts, lam, alpha, eta, tol, cap)["perplexity"], n


def load_golden():
    """tests/golden/lda_bound_r8_small.npz (make_lda_bound_golden.py) as a dict of arrays."""
    return lda_ref._load("lda_bound_r8_small.npz")
