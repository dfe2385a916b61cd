"""How good a topic model is, evaluated on the device (csrc/lda_estep.hip): sklearn's
``LatentDirichletAllocation`` variational bound, ``score`` and ``perplexity``
(_lda.py ``_approx_bound``, ``score``, ``_perplexity_precomp_distr``), the instrument
for turning the ``num_topics`` and ``max_iter`` knobs of the reference's
experiments/r8.yaml.

    tb = fit.scorer()                                # or TopicBound(components, alpha, eta), or from_sklearn(lda)
    held = doc_term(vectorizer.transform(held_out_texts), "cuda")
    tb.score(*held)                                  # lda.score(X)        0-dim float64 on the device
    tb.perplexity(*held)                             # lda.perplexity(X)

With E[log theta_dk] = psi(gamma_dk) - psi(sum_k gamma_dk) and E[log beta_kw] =
psi(lambda_kw) - psi(sum_w lambda_kw), psi sklearn's AS 103:

    doc_d   = sum_w c_dw logsumexp_k(E[log theta_dk] + E[log beta_kw])
            + sum_k (alpha - gamma_dk) E[log theta_dk] + sum_k (lgamma(gamma_dk) - lgamma(alpha))
            + lgamma(alpha K) - lgamma(sum_k gamma_dk)
    topic_k = sum_w (eta - lambda_kw) E[log beta_kw] + sum_w (lgamma(lambda_kw) - lgamma(eta))
            + lgamma(eta V) - lgamma(sum_w lambda_kw)
    bound   = doc_ratio sum_d doc_d + sum_k topic_k       (doc_ratio = 1, or total_samples / B when sub_sampling)
    perplexity = exp(-bound / (doc_ratio sum c))

``score`` is the bound at gamma = ``TopicInferencer.gamma`` (sklearn's
``_unnormalized_transform``: the E-step started from gamma = 1).  An evaluation is
the gamma E-step and three launches (the documents' terms, one wave each; the
topics' terms, cached; one workgroup that sums), all queued on the current stream:
nothing synchronises, every sum has a fixed order (include/gcnk_lda.h), so a
result is bitwise reproducible and a document's term does not depend on its batch.

The limit of the model's validity: the logsumexp shifts theta's side only and
reads the table of exp(E[log beta]) the E-step reads.  A prior so small that
exp(E[log beta_kw]) underflows to 0 in every topic of a word makes that word's term
-inf where sklearn's logsumexp stays finite; sklearn's own E-step is already
degenerate there (it divides by 2^-52).  There is no second code path.
"""
import math

import torch

from . import _lib
from .derived import Cache
from .topic_infer import _COUNTS, TopicInferencer, _model_matrix, check_documents, kernel_documents

TOPIC_CHUNK = 256   # csrc/lda_estep.hip kTopicThreads: the threads the topic term's words are dealt to


class _TopicTerm:
    """topic_bound [K] float64 of one lambda."""

    __slots__ = ("t", "pinned")


def topic_terms(lam, eta):
    """gcnk_lda_bound_topics_f64: topic_k of lambda [K x V] (float64 on the device, unit stride
    along V) -> float64 [K]."""
    K, V = lam.shape
    out = torch.empty(K, dtype=torch.float64, device=lam.device)
    with torch.cuda.device(lam.device):
        _lib.check(_lib.load().gcnk_lda_bound_topics_f64(lam.data_ptr(), lam.stride(0), K, V, eta, out.data_ptr(),
                                                         _lib.stream(lam.device)), "gcnk_lda_bound_topics_f64")
    return out


def doc_terms(table, K, V, indptr, indices, counts, B, gamma, alpha):
    """gcnk_lda_bound_docs_f64: doc_d of checked documents (``kernel_documents``' arrays) under
    ``table`` and gamma [B x K] -> float64 [B]."""
    out = torch.empty(B, dtype=torch.float64, device=table.device)
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().gcnk_lda_bound_docs_f64(
            indptr.data_ptr(), indices.data_ptr(), counts.data_ptr(), _COUNTS[counts.dtype], B, V, K, table.data_ptr(),
            table.stride(0), gamma.data_ptr(), gamma.stride(0), alpha, out.data_ptr(), _lib.stream(table.device)),
            "gcnk_lda_bound_docs_f64")
    return out


def finish(doc_bound, topic_bound, indptr, counts, doc_ratio):
    """gcnk_lda_bound_finish_f64 -> float64 [3]: the bound, the word count, the perplexity."""
    out = torch.empty(3, dtype=torch.float64, device=doc_bound.device)
    with torch.cuda.device(doc_bound.device):
        _lib.check(_lib.load().gcnk_lda_bound_finish_f64(
            doc_bound.data_ptr(), doc_bound.numel(), topic_bound.data_ptr(), topic_bound.numel(), indptr.data_ptr(),
            counts.data_ptr(), _COUNTS[counts.dtype], doc_ratio, out.data_ptr(), _lib.stream(doc_bound.device)),
            "gcnk_lda_bound_finish_f64")
    return out


def doc_ratio_of(who, B, sub_sampling, total_samples):
    """sklearn's doc_ratio: 1, or total_samples / B when sub_sampling (RuntimeError without a finite
    positive total_samples)."""
    if not sub_sampling:
        return 1.0
    total = float("nan") if total_samples is None else float(total_samples)
    if not 0.0 < total < math.inf:
        raise RuntimeError(f"{who}: sub_sampling needs a finite positive total_samples, got {total_samples}")
    return total / B


class TopicBound:
    """score, perplexity and bound of documents under lambda = ``components`` [K x V]
    (float64 on the device; sklearn's ``components_``) with the priors ``doc_topic_prior``
    (alpha) and ``topic_word_prior`` (eta).  It owns a ``TopicInferencer`` for gamma, which
    holds the table of exp(E[log beta]); the topic term, which depends on lambda alone, is
    held the same way, while derived.stamp() of ``components`` is unchanged."""

    def __init__(self, components, doc_topic_prior, topic_word_prior, mean_change_tol=1e-3, max_doc_update_iter=100):
        lam = _model_matrix(components, "components")
        if lam.stride(1) != 1 or lam.stride(0) < lam.shape[1]:
            lam = lam.contiguous()
        self._lam = lam
        self.K, self.V = lam.shape
        self.doc_topic_prior, self.topic_word_prior = float(doc_topic_prior), float(topic_word_prior)
        self.inferencer = TopicInferencer.from_components(lam, doc_topic_prior, mean_change_tol, max_doc_update_iter)
        self._cache = Cache(1)

    @classmethod
    def from_sklearn(cls, lda, device="cuda"):
        """From a fitted ``LatentDirichletAllocation`` (duck-typed: ``components_``,
        ``doc_topic_prior_``, ``topic_word_prior_``, ``mean_change_tol``,
        ``max_doc_update_iter``); lambda is uploaded to ``device``."""
        lam = torch.as_tensor(lda.components_)
        if lam.dtype != torch.float64:
            raise RuntimeError(f"components_ is {lam.dtype}: only sklearn's float64 model is reproduced")
        return cls(lam.to(device), lda.doc_topic_prior_, lda.topic_word_prior_, lda.mean_change_tol,
                   lda.max_doc_update_iter)

    @property
    def components(self):
        return self._lam

    def _build_topics(self):
        term = _TopicTerm()
        term.t, term.pinned = topic_terms(self._lam, self.topic_word_prior), False
        return term

    def topic_bound(self):
        """topic_k, float64 [K]: built once per value of lambda (derived.py's rule)."""
        term = self._cache.get("topic_bound", (self._lam,), self._build_topics)
        if torch.cuda.is_current_stream_capturing():
            term.pinned = True   # (a captured launch keeps reading it: derived.py)
        return term.t

    def _gamma(self, indptr, indices, counts, gamma):
        tb = self.inferencer._table()
        B = check_documents(indptr, indices, counts, tb.t.device)
        if gamma is None:
            return tb, B, self.inferencer.gamma(indptr, indices, counts)
        _model_matrix(gamma, "gamma")
        if tuple(gamma.shape) != (B, self.K) or gamma.device != tb.t.device:
            raise RuntimeError(f"gamma must be float64 [{B} x {self.K}] on {tb.t.device}, got {tuple(gamma.shape)} on "
                               f"{gamma.device}")
        return tb, B, gamma if gamma.stride(1) == 1 else gamma.contiguous()

    def parts(self, indptr, indices, counts, gamma=None):
        """(doc_bound [B], topic_bound [K]) float64: every document's and every topic's term
        (gamma: the inferencer's where not given)."""
        tb, B, gamma = self._gamma(indptr, indices, counts, gamma)
        return doc_terms(tb.t, tb.K, tb.V, *kernel_documents(indptr, indices, counts), B, gamma,
                         self.doc_topic_prior), self.topic_bound()

    def _evaluate(self, indptr, indices, counts, gamma, sub_sampling, total_samples):
        docs, topics = self.parts(indptr, indices, counts, gamma)
        ratio = doc_ratio_of("TopicBound", docs.numel(), sub_sampling, total_samples)
        indptr, _, counts = kernel_documents(indptr, indices, counts)
        return finish(docs, topics, indptr, counts, ratio)

    def bound(self, indptr, indices, counts, gamma, sub_sampling=False, total_samples=None):
        """sklearn's ``_approx_bound(X, gamma, sub_sampling)`` for a gamma [B x K] computed
        before: a 0-dim float64 device tensor."""
        if gamma is None:
            raise RuntimeError("bound takes a precomputed gamma [B x K]; score computes its own")
        return self._evaluate(indptr, indices, counts, gamma, sub_sampling, total_samples)[0]

    def score(self, indptr, indices, counts):
        """sklearn's ``score(X)``: the bound at the inferencer's gamma."""
        return self._evaluate(indptr, indices, counts, None, False, None)[0]

    def perplexity(self, indptr, indices, counts, sub_sampling=False, total_samples=None):
        """sklearn's ``perplexity(X, sub_sampling)``: exp(-bound / word count) at the
        inferencer's gamma, ``total_samples`` standing for the fitted model's."""
        return self._evaluate(indptr, indices, counts, None, sub_sampling, total_samples)[2]
