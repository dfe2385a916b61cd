"""The topic model fitted on the device (csrc/lda_estep.hip): the step before
``TopicInferencer``, ``build_topic_graph`` and ``DocumentScorer``.

The reference fits sklearn's LDA on the host (topic_model.py:74-131,
``LatentDirichletAllocation(learning_method='batch').fit``).  Here the same batch
variational EM -- sklearn's rules restated in float64: its AS 103 psi, a fresh
gamma draw every EM iteration, the mean-change stop rule, the sufficient
statistics summed document by document in ascending order -- runs as
``max_iter x (exp_dirichlet -> fit E-step -> M-step)`` launches queued on the
current stream, then one last ``exp_dirichlet``:

    indptr, indices, counts = doc_term(vectorizer.fit_transform(texts), "cuda")
    fit = fit_topics(indptr, indices, counts, V=len(vectorizer.vocabulary_), num_topics=50, max_iter=20)
    fit.components                 # lambda [K x V] float64            (lda.components_)
    fit.topic_word_distribution    # lambda over its row sums          (topic_model.py:123-126)
    theta = fit.inferencer()(indptr, indices, counts)

Nothing between the first launch and the last synchronises with the host, and
with ``init=`` the whole call can be captured in a hipGraph on one stream.

sklearn's random draws are made on the host up front with
``numpy.random.RandomState(random_state)``: lambda0 = gamma(100, .01, (K, V)),
then gamma0 = gamma(100, .01, (max_iter, B, K)) in one call, which is the stream
of sklearn's successive (B, K) draws; they are uploaded before the first launch.
``init=(lambda0, gamma0s)`` takes float64 device tensors of those shapes instead
and draws nothing.

Not restated (sklearn features the reference never uses): ``bound_`` and the
extra E-step and perplexity sklearn computes for it after the loop,
``learning_method='online'``, ``evaluate_every > 0``, ``n_jobs`` slicing of the
documents, float32 input.  A document's word ids must be distinct (a CSR row of a
document-term matrix); a word id outside [0, V) is the caller's error.
"""
import torch

from . import _lib
from .sparse import require_device
from .topic_infer import _COUNTS, MAX_TOPICS, MAX_UPDATE_ITER, TopicInferencer, check_documents

WORDS_PER_BLOCK = 4   # csrc/lda_estep.hip kWords: the M-step's waves (words) per workgroup


class WordIndex:
    """The document-term CSR walked by word: word w's entries are ``[wptr[w], wptr[w + 1])``,
    entry i is the CSR position ``pos[i]`` in document ``doc[i]``; a word's entries ascend in
    document (the sort is stable), which is the order sklearn sums them in.  int32, on the device."""

    __slots__ = ("wptr", "pos", "doc")


def word_index(indptr, indices, V):
    """-> WordIndex of the CSR (indptr int32 [B + 1], indices int32 [nnz]) over V words.  torch
    only, no host synchronisation."""
    dev = indices.device
    ids, pos = torch.sort(indices.to(torch.int64), stable=True)
    ix = WordIndex()
    ix.wptr = torch.searchsorted(ids, torch.arange(V + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    ix.doc = (torch.searchsorted(indptr.to(torch.int64), pos, right=True) - 1).to(torch.int32)
    ix.pos = pos.to(torch.int32)
    return ix


class TopicFit:
    """What ``fit_topics`` returns; every tensor is on the documents' device."""

    __slots__ = ("components", "topic_word_distribution", "iterations", "doc_topic_prior", "topic_word_prior",
                 "mean_change_tol", "max_doc_update_iter", "n_iter", "_table", "_work")

    @property
    def exp_topic_word(self):
        """exp(E[log beta]) [K x V] float64 of the fitted lambda (sklearn's
        ``exp_dirichlet_component_``): a transposed view of the last table."""
        return self._table[:, :self.components.shape[0]].t()

    def inferencer(self):
        """``TopicInferencer.from_components`` of the fitted lambda with the fit's prior,
        tolerance and update cap: theta of any documents under this model."""
        return TopicInferencer.from_components(self.components, self.doc_topic_prior, self.mean_change_tol,
                                               self.max_doc_update_iter)


def _init_tensor(t, what, shape, dev):
    require_device(t, what)
    if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev:
        raise RuntimeError(f"init: {what} must be float64 {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t if t.is_contiguous() else t.contiguous()


def fit_topics(indptr, indices, counts, V, num_topics=50, max_iter=20, random_state=42, doc_topic_prior=None,
               topic_word_prior=None, mean_change_tol=1e-3, max_doc_update_iter=100, init=None,
               return_iterations=False):
    """sklearn's batch LDA fit of the documents (a CSR over V words, as ``doc_term`` gives it)
    -> TopicFit.  ``doc_topic_prior`` / ``topic_word_prior`` default to 1 / num_topics as
    sklearn's do.  ``init``: (lambda0 [K x V], gamma0s [max_iter x B x K]) float64 on the
    documents' device instead of the host draw.  ``return_iterations``: ``fit.iterations`` is the
    int32 [max_iter x B] count of updates every document ran in every EM iteration.
    RuntimeError, never a fallback: more than 128 topics, max_iter < 1, V < 1, an update cap
    outside [0, 10000], a bad ``init``, and check_documents' refusals (float32 counts, CPU
    tensors, dtypes)."""
    K, V, max_iter, cap = int(num_topics), int(V), int(max_iter), int(max_doc_update_iter)
    if not 1 <= K <= MAX_TOPICS:
        raise RuntimeError(f"fit_topics: num_topics={K} is outside [1, {MAX_TOPICS}] (unsupported: two topics a lane)")
    if max_iter < 1 or V < 1:
        raise RuntimeError(f"fit_topics: needs max_iter >= 1 and V >= 1 (max_iter={max_iter} V={V})")
    if not 0 <= cap <= MAX_UPDATE_ITER:
        raise RuntimeError(f"fit_topics: max_doc_update_iter={cap} is outside [0, {MAX_UPDATE_ITER}]")
    B = check_documents(indptr, indices, counts, getattr(indptr, "device", None))
    dev = indptr.device
    alpha = 1.0 / K if doc_topic_prior is None else float(doc_topic_prior)
    eta = 1.0 / K if topic_word_prior is None else float(topic_word_prior)
    tol = float(mean_change_tol)

    if init is None:
        import numpy as np
        rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        lam0 = torch.from_numpy(rs.gamma(100.0, 0.01, (K, V))).to(dev)
        gamma0s = torch.from_numpy(rs.gamma(100.0, 0.01, (max_iter, B, K))).to(dev)
    else:
        if not isinstance(init, (tuple, list)) or len(init) != 2:
            raise RuntimeError("init must be (lambda0 [K x V], gamma0s [max_iter x B x K])")
        lam0 = _init_tensor(init[0], "lambda0", (K, V), dev)
        gamma0s = _init_tensor(init[1], "gamma0s", (max_iter, B, K), dev)

    indptr, indices, counts = indptr.contiguous(), indices.contiguous(), counts.contiguous()
    nnz = indices.numel()
    ix = word_index(indptr, indices, V)
    if nnz == 0:   # (no word at all: the entry points still want addresses)
        indices = torch.zeros(1, dtype=torch.int32, device=dev)
        counts = torch.zeros(1, dtype=counts.dtype, device=dev)
        ix.pos = ix.doc = torch.zeros(1, dtype=torch.int32, device=dev)
    table = torch.zeros((V, (K + 1) // 2 * 2), dtype=torch.float64, device=dev)
    lam = torch.empty((K, V), dtype=torch.float64, device=dev)
    etheta = torch.empty((B, K), dtype=torch.float64, device=dev)
    ratio = torch.empty(max(nnz, 1), dtype=torch.float64, device=dev)
    iters = torch.empty((max_iter, B), dtype=torch.int32, device=dev) if return_iterations else None

    lib = _lib.load()
    ldt = table.stride(0)
    with torch.cuda.device(dev):
        stream = _lib.stream(dev)

        def exp_dirichlet(src):
            _lib.check(lib.gcnk_lda_exp_dirichlet_f64(src.data_ptr(), src.stride(0), K, V, table.data_ptr(), ldt, stream),
                       "gcnk_lda_exp_dirichlet_f64")

        for it in range(max_iter):
            exp_dirichlet(lam0 if it == 0 else lam)
            g0 = gamma0s[it]
            _lib.check(lib.gcnk_lda_estep_fit_f64(
                indptr.data_ptr(), indices.data_ptr(), counts.data_ptr(), _COUNTS[counts.dtype], B, V, K,
                table.data_ptr(), ldt, alpha, tol, cap, g0.data_ptr(), g0.stride(0), nnz, ratio.data_ptr(),
                etheta.data_ptr(), etheta.stride(0), None, 0, None if iters is None else iters[it].data_ptr(), stream),
                "gcnk_lda_estep_fit_f64")
            _lib.check(lib.gcnk_lda_mstep_f64(
                ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), nnz, ratio.data_ptr(), etheta.data_ptr(),
                etheta.stride(0), B, V, K, table.data_ptr(), ldt, eta, lam.data_ptr(), lam.stride(0), stream),
                "gcnk_lda_mstep_f64")
        exp_dirichlet(lam)

    fit = TopicFit()
    fit.components = lam
    fit.topic_word_distribution = lam / lam.sum(dim=1, keepdim=True)
    fit.iterations = iters
    fit.doc_topic_prior, fit.topic_word_prior = alpha, eta
    fit.mean_change_tol, fit.max_doc_update_iter, fit.n_iter = tol, cap, max_iter
    fit._table = table
    # (a captured call's launches keep reading these through raw pointers: held as long as the result is)
    fit._work = (indptr, indices, counts, lam0, gamma0s, ix, etheta, ratio)
    return fit
