"""The topic model fitted on the device (csrc/lda_estep.hip): the step before
``TopicInferencer``, ``build_topic_graph`` and ``DocumentScorer``.

The reference fits sklearn's LDA on the host (topic_model.py:74-131,
``LatentDirichletAllocation(learning_method=...).fit``, 'batch' or 'online':
topic_model.py:46,55,113).  Here sklearn's variational EM -- its rules restated in
float64: its AS 103 psi, a fresh gamma draw every EM iteration, the mean-change
stop rule, the sufficient statistics summed document by document in ascending
order -- runs as launches queued on the current stream.

``learning_method="batch"`` (the default): ``max_iter x (exp_dirichlet -> fit
E-step -> M-step)``, then one last ``exp_dirichlet``:

    indptr, indices, counts = doc_term(vectorizer.fit_transform(texts), "cuda")
    fit = fit_topics(indptr, indices, counts, V=len(vectorizer.vocabulary_), num_topics=50, max_iter=20)
    fit.components                 # lambda [K x V] float64            (lda.components_)
    fit.topic_word_distribution    # lambda over its row sums          (topic_model.py:123-126)
    theta = fit.inferencer()(indptr, indices, counts)

``learning_method="online"``: sklearn's minibatch EM (_lda.py
``_em_step(batch_update=False)``).  Every EM iteration walks the documents in
``gen_batches(B, batch_size)`` slices, and every slice is ``exp_dirichlet -> fit
E-step on the slice's rows -> online M-step``:

    lambda = lambda * (1 - rho) + rho * (eta + (B / slice size) * S o beta)

with ``rho = numpy.power(learning_offset + n, -learning_decay)`` taken on the host
in float64, n counting the minibatches from 1.  The same launches behind
``OnlineTopics.partial_fit`` move a fitted model as new documents arrive:

    ot = OnlineTopics(V, num_topics=50, total_samples=1e6)     # or OnlineTopics.from_fit(fit, total_samples=...)
    ot.partial_fit(indptr, indices, counts)                    # lda.partial_fit(X)
    theta = ot.inferencer()(indptr, indices, counts)

Nothing between the first launch and the last synchronises with the host, and
with ``init=`` a whole ``fit_topics`` call (either method) can be captured in a
hipGraph on one stream.

sklearn's random draws are made on the host up front with
``numpy.random.RandomState(random_state)``: lambda0 = gamma(100, .01, (K, V)),
then gamma0 = gamma(100, .01, (max_iter, B, K)) in one call, which is the stream
of sklearn's successive draws (per EM iteration for 'batch', per minibatch for
'online': rows [b0, b1) of iteration ``it`` are the slice ``[it, b0:b1]``); they
are uploaded before the first launch.  ``init=(lambda0, gamma0s)`` takes float64
device tensors of those shapes instead and draws nothing.  ``OnlineTopics`` keeps
its RandomState and draws a (B, K) gamma0 per ``partial_fit``.

``evaluate_every`` / ``perp_tol`` / ``bound_`` are sklearn's too (topic_bound.py has
the bound itself, with ``score`` and ``perplexity``).  ``compute_bound=True`` closes
the fit as sklearn does, with an E-step from gamma = 1 and the training perplexity
of the fitted lambda: ``fit.bound`` is sklearn's ``bound_``, a 0-dim device tensor,
and still nothing synchronises.  ``evaluate_every=n > 0`` evaluates that perplexity
after every n-th EM iteration, READS IT ON THE HOST (one scalar: the only
synchronisation, in this mode alone) and stops by sklearn's rule -- the change
since the last evaluation below ``perp_tol``, tested before the iteration is
counted: ``fit.n_iter`` is sklearn's ``n_iter_``, ``fit.perplexities`` the values.
``fit.scorer()`` / ``OnlineTopics.scorer()`` give the ``TopicBound`` of the model
for held-out documents.

Still not restated, out of scope (sklearn features the reference never uses):
``n_jobs`` slicing of the documents, float32 input; the online method shuffles
nothing, as sklearn's does not.  A document's word ids must be distinct (a CSR row
of a document-term matrix); a word id outside [0, V) is the caller's error.
"""
import torch

from . import _lib, topic_bound
from .sparse import require_device
from .topic_infer import (_COUNTS, MAX_TOPICS, MAX_UPDATE_ITER, TopicInferencer, check_documents, kernel_documents,
                          model_table, run_estep)

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
    """What ``fit_topics`` returns; every tensor is on the documents' device.  ``n_batch_iter``
    is sklearn's ``n_batch_iter_`` after the call: 1 + the M-steps run (EM iterations for
    'batch', minibatches for 'online'); ``n_iter`` its ``n_iter_``.  ``bound``: sklearn's
    ``bound_``, the training perplexity of the fitted lambda as a 0-dim float64 device tensor
    (None unless asked for); ``perplexities``: the values ``evaluate_every`` read, host floats."""

    __slots__ = ("components", "topic_word_distribution", "iterations", "doc_topic_prior", "topic_word_prior",
                 "mean_change_tol", "max_doc_update_iter", "n_iter", "n_batch_iter", "bound", "perplexities", "_table",
                 "_work")

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

    def scorer(self):
        """``TopicBound`` of the fitted lambda with the fit's priors, tolerance and update cap:
        score and perplexity of any documents under this model."""
        return topic_bound.TopicBound(self.components, self.doc_topic_prior, self.topic_word_prior,
                                      self.mean_change_tol, self.max_doc_update_iter)


def _init_tensor(t, what, shape, dev):
    require_device(t, what)
    if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev:
        raise RuntimeError(f"init: {what} must be float64 {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t if t.is_contiguous() else t.contiguous()


def _check_model(who, K, cap, **at_least_one):
    """The refusals of a model's size: the topics two a lane, every named size (V, max_iter) at
    least 1, the update cap within the kernel's."""
    if not 1 <= K <= MAX_TOPICS:
        raise RuntimeError(f"{who}: num_topics={K} is outside [1, {MAX_TOPICS}] (unsupported: two topics a lane)")
    if min(at_least_one.values()) < 1:
        raise RuntimeError(f"{who}: needs {' and '.join(f'{k} >= 1' for k in at_least_one)} "
                           f"({' '.join(f'{k}={v}' for k, v in at_least_one.items())})")
    if not 0 <= cap <= MAX_UPDATE_ITER:
        raise RuntimeError(f"{who}: max_doc_update_iter={cap} is outside [0, {MAX_UPDATE_ITER}]")


def _random_state(random_state):
    """A numpy RandomState as it is, anything else as its seed."""
    import numpy as np
    return random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)


def _draw(rs, shape, dev):
    """sklearn's initial draw, gamma(100, .01), made on the host and uploaded."""
    return torch.from_numpy(rs.gamma(100.0, 0.01, shape)).to(dev)


def _check_online(who, batch_size, learning_decay, learning_offset):
    """sklearn's own constraints on the online method's parameters -> (batch_size, decay, offset)."""
    bs, decay, offset = int(batch_size), float(learning_decay), float(learning_offset)
    if bs < 1:
        raise RuntimeError(f"{who}: batch_size={batch_size} must be at least 1")
    if not 0.0 <= decay <= 1.0:
        raise RuntimeError(f"{who}: learning_decay={learning_decay} is outside [0, 1]")
    if not 1.0 <= offset < float("inf"):
        raise RuntimeError(f"{who}: learning_offset={learning_offset} must be a finite number >= 1")
    return bs, decay, offset


def _rho(offset, n, decay):
    """sklearn's weight of minibatch n (its ``n_batch_iter_``), in float64 on the host."""
    import numpy as np
    return float(np.power(offset + n, -decay))


def _exp_dirichlet(lib, stream, lam, table):
    K, V = lam.shape
    _lib.check(lib.gcnk_lda_exp_dirichlet_f64(lam.data_ptr(), lam.stride(0), K, V, table.data_ptr(), table.stride(0),
                                              stream), "gcnk_lda_exp_dirichlet_f64")


class _Documents:
    """A document batch as the fit's launches read it: the CSR, its word-major index and the
    E-step's outputs (etheta [B x K], a ratio per stored nonzero)."""

    __slots__ = ("indptr", "indices", "counts", "B", "V", "K", "nnz", "ix", "etheta", "ratio")

    def __init__(self, indptr, indices, counts, B, V, K):
        dev = indptr.device
        self.B, self.V, self.K, self.nnz = B, V, K, indices.numel()
        self.indptr, self.indices, self.counts = kernel_documents(indptr, indices, counts)
        self.ix = word_index(self.indptr, indices.contiguous(), V)
        if self.nnz == 0:   # (kernel_documents' stand-ins, for the index too)
            self.ix.pos = self.ix.doc = torch.zeros(1, dtype=torch.int32, device=dev)
        self.etheta = torch.empty((B, K), dtype=torch.float64, device=dev)
        self.ratio = torch.empty(max(self.nnz, 1), dtype=torch.float64, device=dev)


def _estep_fit(lib, stream, docs, b0, b1, table, gamma0, iters, alpha, tol, cap):
    """The fit E-step of rows [b0, b1) of ``docs``, from those rows of ``gamma0`` [B x K], into
    ``docs.etheta``, ``docs.ratio`` and ``iters`` (int32 [B] or None).  A row range needs no copy:
    indptr, gamma0, etheta and iters go in advanced by b0 rows (8-byte scalar accesses, so any
    row offset is aligned) with the whole ratio array, where the kernel stores at absolute CSR
    positions."""
    _lib.check(lib.gcnk_lda_estep_fit_f64(
        docs.indptr[b0:].data_ptr(), docs.indices.data_ptr(), docs.counts.data_ptr(), _COUNTS[docs.counts.dtype],
        b1 - b0, docs.V, docs.K, table.data_ptr(), table.stride(0), alpha, tol, cap, gamma0[b0:].data_ptr(),
        gamma0.stride(0), docs.nnz, docs.ratio.data_ptr(), docs.etheta[b0:].data_ptr(), docs.etheta.stride(0), None, 0,
        None if iters is None else iters[b0:].data_ptr(), stream), "gcnk_lda_estep_fit_f64")


def _online_pass(lib, stream, docs, lam, table, gamma0, iters, alpha, eta, tol, cap, bs, decay, offset, total, n):
    """One walk over ``docs`` in minibatches of ``bs``: fit E-step on the rows -> online M-step
    -> exp_dirichlet, the table being current on entry and on return.  ``gamma0`` [B x K] and
    ``iters`` (int32 [B] or None) are the walk's; ``n`` is sklearn's n_batch_iter_ on entry ->
    on return.  The M-step takes the whole index and the minibatch's row range."""
    B, V, K, ix = docs.B, docs.V, docs.K, docs.ix
    for b0 in range(0, B, bs):
        b1 = min(b0 + bs, B)
        _estep_fit(lib, stream, docs, b0, b1, table, gamma0, iters, alpha, tol, cap)
        _lib.check(lib.gcnk_lda_mstep_online_f64(
            ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), docs.nnz, b0, b1, docs.ratio.data_ptr(),
            docs.etheta.data_ptr(), docs.etheta.stride(0), B, V, K, table.data_ptr(), table.stride(0), eta,
            _rho(offset, n, decay), float(total) / (b1 - b0), lam.data_ptr(), lam.stride(0), stream),
            "gcnk_lda_mstep_online_f64")
        _exp_dirichlet(lib, stream, lam, table)
        n += 1
    return n


def _training_perplexity(docs, lam, table, alpha, eta, tol, cap):
    """sklearn's perplexity of the fit's own documents under ``lam``, whose ``table`` is current:
    the E-step from gamma = 1 (``_e_step(random_init=False)``), then the bound's three launches
    -> float64 [3] on the device (bound, word count, perplexity)."""
    held = (docs.indptr, docs.indices, docs.counts, docs.B)
    gamma = run_estep(table, docs.K, docs.V, *held, alpha, tol, cap, gamma=True)["gamma"]
    doc_bound = topic_bound.doc_terms(table, docs.K, docs.V, *held, gamma, alpha)
    return topic_bound.finish(doc_bound, topic_bound.topic_terms(lam, eta), docs.indptr, docs.counts, 1.0)


def fit_topics(indptr, indices, counts, V, num_topics=50, max_iter=20, random_state=42, doc_topic_prior=None,
               topic_word_prior=None, mean_change_tol=1e-3, max_doc_update_iter=100, init=None,
               return_iterations=False, learning_method="batch", batch_size=128, learning_decay=0.7,
               learning_offset=10.0, evaluate_every=0, perp_tol=0.1, compute_bound=False):
    """sklearn's LDA fit of the documents (a CSR over V words, as ``doc_term`` gives it)
    -> TopicFit.  ``doc_topic_prior`` / ``topic_word_prior`` default to 1 / num_topics as
    sklearn's do.  ``init``: (lambda0 [K x V], gamma0s [max_iter x B x K]) float64 on the
    documents' device instead of the host draw.  ``return_iterations``: ``fit.iterations`` is the
    int32 [max_iter x B] count of updates every document ran in every EM iteration.
    ``learning_method``: 'batch' or 'online'; ``batch_size``, ``learning_decay`` and
    ``learning_offset`` are the online method's (sklearn's names and defaults) and are not
    looked at for 'batch'.  ``evaluate_every`` / ``perp_tol`` (sklearn's; <= 0: never) and
    ``compute_bound``: see the module docstring; with their defaults the launches are the
    fit's alone.  A fit that ``evaluate_every`` stops early leaves the rows of
    ``fit.iterations`` past ``n_batch_iter`` unwritten.
    RuntimeError, never a fallback: more than 128 topics, max_iter < 1, V < 1, an update cap
    outside [0, 10000], a bad ``init``, an unknown ``learning_method``, batch_size < 1,
    learning_decay outside [0, 1], learning_offset < 1, ``evaluate_every > 0`` with a
    ``perp_tol`` that is negative or NaN or inside a stream capture (it reads the device), and
    check_documents' refusals (float32 counts, CPU tensors, dtypes)."""
    K, V, max_iter, cap = int(num_topics), int(V), int(max_iter), int(max_doc_update_iter)
    _check_model("fit_topics", K, cap, max_iter=max_iter, V=V)
    if learning_method not in ("batch", "online"):
        raise RuntimeError(f"fit_topics: learning_method={learning_method!r} is neither 'batch' nor 'online'")
    online = learning_method == "online"
    if online:
        bs, decay, offset = _check_online("fit_topics", batch_size, learning_decay, learning_offset)
    every, perp_tol = max(int(evaluate_every), 0), float(perp_tol)
    if every and not perp_tol >= 0.0:
        raise RuntimeError(f"fit_topics: perp_tol={perp_tol} must be at least 0")
    B = check_documents(indptr, indices, counts, getattr(indptr, "device", None))
    dev = indptr.device
    if every and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("fit_topics: evaluate_every > 0 reads a perplexity on the host after an EM iteration, "
                           "which a stream capture cannot do (capture with evaluate_every=0)")
    alpha = 1.0 / K if doc_topic_prior is None else float(doc_topic_prior)
    eta = 1.0 / K if topic_word_prior is None else float(topic_word_prior)
    tol = float(mean_change_tol)

    if init is None:
        rs = _random_state(random_state)
        lam0 = _draw(rs, (K, V), dev)
        gamma0s = _draw(rs, (max_iter, B, K), dev)
    else:
        if not isinstance(init, (tuple, list)) or len(init) != 2:
            raise RuntimeError("init must be (lambda0 [K x V], gamma0s [max_iter x B x K])")
        lam0 = _init_tensor(init[0], "lambda0", (K, V), dev)
        gamma0s = _init_tensor(init[1], "gamma0s", (max_iter, B, K), dev)

    docs = _Documents(indptr, indices, counts, B, V, K)
    table = model_table(K, V, dev)
    iters = torch.empty((max_iter, B), dtype=torch.int32, device=dev) if return_iterations else None

    perplexities, last, n_iter = [], None, 0

    def converged():
        """sklearn's check after an EM iteration (lam's table is current): the training
        perplexity, read on the host, within perp_tol of the last one read."""
        nonlocal last
        p = float(_training_perplexity(docs, lam, table, alpha, eta, tol, cap)[2])
        perplexities.append(p)
        if last and abs(last - p) < perp_tol:
            return True
        last = p
        return False

    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _lib.stream(dev)
        if online:
            lam = lam0.clone()   # (the online M-step works in place)
            _exp_dirichlet(lib, stream, lam, table)
            n = 1
            for it in range(max_iter):
                n = _online_pass(lib, stream, docs, lam, table, gamma0s[it], None if iters is None else iters[it],
                                 alpha, eta, tol, cap, bs, decay, offset, B, n)
                if every and (it + 1) % every == 0 and converged():
                    break
                n_iter += 1
        else:
            lam = torch.empty((K, V), dtype=torch.float64, device=dev)
            ix = docs.ix
            n = 1
            for it in range(max_iter):
                _exp_dirichlet(lib, stream, lam0 if it == 0 else lam, table)
                _estep_fit(lib, stream, docs, 0, B, table, gamma0s[it], None if iters is None else iters[it], alpha, tol,
                           cap)
                _lib.check(lib.gcnk_lda_mstep_f64(
                    ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), docs.nnz, docs.ratio.data_ptr(),
                    docs.etheta.data_ptr(), docs.etheta.stride(0), B, V, K, table.data_ptr(), table.stride(0), eta,
                    lam.data_ptr(), lam.stride(0), stream), "gcnk_lda_mstep_f64")
                n += 1
                if every and (it + 1) % every == 0:
                    _exp_dirichlet(lib, stream, lam, table)   # (the next iteration makes the same table again)
                    if converged():
                        break
                n_iter += 1
            _exp_dirichlet(lib, stream, lam, table)
        bound = _training_perplexity(docs, lam, table, alpha, eta, tol, cap)[2] if compute_bound or every else None

    fit = TopicFit()
    fit.components = lam
    fit.topic_word_distribution = lam / lam.sum(dim=1, keepdim=True)
    fit.iterations = iters
    fit.doc_topic_prior, fit.topic_word_prior = alpha, eta
    fit.mean_change_tol, fit.max_doc_update_iter, fit.n_iter = tol, cap, n_iter
    fit.n_batch_iter = n
    fit.bound, fit.perplexities = bound, perplexities
    fit._table = table
    # (a captured call's launches keep reading these through raw pointers: held as long as the result is)
    fit._work = (docs, lam0, gamma0s)
    return fit


class OnlineTopics:
    """A topic model that keeps learning on the device: sklearn's
    ``LatentDirichletAllocation(learning_method='online').partial_fit``.

    The first construction draws lambda0 = gamma(100, .01, (K, V)) from
    ``RandomState(random_state)`` on the host, as sklearn's ``_init_latent_vars`` does at its
    first ``partial_fit``; ``init_components`` takes a float64 [K x V] device tensor instead
    (it is copied).  ``total_samples`` is sklearn's: the corpus size the minibatches are
    scaled to.  ``n_batch_iter`` (sklearn's ``n_batch_iter_``) lives on the host; nothing
    synchronises."""

    def __init__(self, V, num_topics=50, total_samples=1e6, batch_size=128, learning_decay=0.7, learning_offset=10.0,
                 random_state=42, doc_topic_prior=None, topic_word_prior=None, mean_change_tol=1e-3,
                 max_doc_update_iter=100, device="cuda", init_components=None):
        K, V, cap = int(num_topics), int(V), int(max_doc_update_iter)
        _check_model("OnlineTopics", K, cap, V=V)
        self.batch_size, self.learning_decay, self.learning_offset = _check_online(
            "OnlineTopics", batch_size, learning_decay, learning_offset)
        self.total_samples = float(total_samples)
        if not 0.0 < self.total_samples < float("inf"):
            raise RuntimeError(f"OnlineTopics: total_samples={total_samples} must be a finite positive number")
        self.num_topics, self.V = K, V
        self.doc_topic_prior = 1.0 / K if doc_topic_prior is None else float(doc_topic_prior)
        self.topic_word_prior = 1.0 / K if topic_word_prior is None else float(topic_word_prior)
        self.mean_change_tol, self.max_doc_update_iter = float(mean_change_tol), cap
        self.n_batch_iter = 1
        self.iterations = None
        self._rs = _random_state(random_state)
        if init_components is None:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise RuntimeError(f"OnlineTopics needs a ROCm GPU device, got {dev}")
            self._lam = _draw(self._rs, (K, V), dev)
        else:
            require_device(init_components, "init_components")
            self._lam = _init_tensor(init_components, "init_components", (K, V), init_components.device).clone()
        self._table = None   # (made at the first use: construction launches nothing)
        self._work = None

    @classmethod
    def from_fit(cls, fit, total_samples, random_state=42, batch_size=128, learning_decay=0.7, learning_offset=10.0):
        """Go on from a ``fit_topics`` result (batch or online): its lambda (copied), priors,
        tolerance, update cap and ``n_batch_iter``.  ``random_state`` seeds the gamma0 draws of
        the ``partial_fit`` calls to come."""
        K, V = fit.components.shape
        ot = cls(V, num_topics=K, total_samples=total_samples, batch_size=batch_size, learning_decay=learning_decay,
                 learning_offset=learning_offset, random_state=random_state, doc_topic_prior=fit.doc_topic_prior,
                 topic_word_prior=fit.topic_word_prior, mean_change_tol=fit.mean_change_tol,
                 max_doc_update_iter=fit.max_doc_update_iter, init_components=fit.components)
        ot.n_batch_iter = int(fit.n_batch_iter)
        return ot

    def _current_table(self, lib, stream):
        if self._table is None:
            self._table = model_table(self.num_topics, self.V, self._lam.device)
            _exp_dirichlet(lib, stream, self._lam, self._table)
        return self._table

    def partial_fit(self, indptr, indices, counts, gamma0=None, return_iterations=False):
        """sklearn's ``partial_fit`` of these documents (a CSR over the model's V words) -> self:
        the minibatch walk in ``batch_size`` slices with doc_ratio = total_samples / slice size.
        ``gamma0``: float64 [B x K] on the device instead of the host draw.
        ``return_iterations``: ``self.iterations`` is the int32 [B] update counts of this call."""
        K, V, dev = self.num_topics, self.V, self._lam.device
        B = check_documents(indptr, indices, counts, dev)
        if gamma0 is None:
            g0 = _draw(self._rs, (B, K), dev)
        else:
            g0 = _init_tensor(gamma0, "gamma0", (B, K), dev)
        docs = _Documents(indptr, indices, counts, B, V, K)
        iters = torch.empty(B, dtype=torch.int32, device=dev) if return_iterations else None
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = _lib.stream(dev)
            table = self._current_table(lib, stream)
            self.n_batch_iter = _online_pass(lib, stream, docs, self._lam, table, g0, iters, self.doc_topic_prior,
                                             self.topic_word_prior, self.mean_change_tol, self.max_doc_update_iter,
                                             self.batch_size, self.learning_decay, self.learning_offset,
                                             self.total_samples, self.n_batch_iter)
        self.iterations = iters
        self._work = (docs, g0)
        return self

    @property
    def components(self):
        """lambda [K x V] float64 (sklearn's ``components_``), updated in place by ``partial_fit``."""
        return self._lam

    @property
    def topic_word_distribution(self):
        """lambda over its row sums (topic_model.py:123-126)."""
        return self._lam / self._lam.sum(dim=1, keepdim=True)

    @property
    def exp_topic_word(self):
        """exp(E[log beta]) [K x V] float64 of the current lambda (sklearn's
        ``exp_dirichlet_component_``): a transposed view of the table."""
        with torch.cuda.device(self._lam.device):
            table = self._current_table(_lib.load(), _lib.stream(self._lam.device))
        return table[:, :self.num_topics].t()

    def inferencer(self):
        """``TopicInferencer.from_components`` of a copy of the current lambda: theta of any
        documents under the model as it stands now."""
        return TopicInferencer.from_components(self._lam.clone(), self.doc_topic_prior, self.mean_change_tol,
                                               self.max_doc_update_iter)

    def scorer(self):
        """``TopicBound`` of a copy of the current lambda: score and perplexity of any documents
        under the model as it stands now (so whether a ``partial_fit`` made it better)."""
        return topic_bound.TopicBound(self._lam.clone(), self.doc_topic_prior, self.topic_word_prior,
                                      self.mean_change_tol, self.max_doc_update_iter)
