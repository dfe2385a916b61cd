"""Documents' topic mixtures inferred on the device (csrc/lda_estep.hip): the step
before ``build_topic_graph`` and ``DocumentScorer``.

The reference gets theta from sklearn on the host (topic_model.py:133-164,
``LatentDirichletAllocation.transform``).  Here the same E-step -- sklearn's
rules restated in float64: its AS 103 psi, gamma = 1 at the start, the
mean-change stop rule -- runs one wave per document in one launch:

    inf = TopicInferencer.from_sklearn(lda)                  # or (exp_topic_word, alpha), or from_components
    indptr, indices, counts = doc_term(vectorizer.transform(texts), "cuda")
    theta = inf(indptr, indices, counts)                     # float64 [B x K]
    x, a = inf.scorer_operands(indptr, indices, counts, 0.02)
    labels = scorer.predict(x, a)

Documents are a CSR over the vocabulary: ``indptr`` int32 [B + 1], ``indices``
int32, ``counts`` float64, int32 or int64 (widened exactly).  float32 counts
are refused: sklearn would run a float32 E-step on them, which this does not
restate.  A word id outside [0, V) is the caller's error and is not checked on
the device (the same policy as ``from_theta``'s for bad theta).  No call
synchronises with the host, and every call can be captured in a hipGraph on one
stream.  A document's row depends on its own words and K alone: not on the
batch, its place in it, or the launch.
"""
import torch

from . import _lib
from .derived import Cache
from .sparse import require_device

MAX_TOPICS = 128      # csrc/lda_estep.hip kMaxTopics
TILE_WORDS = 64       # csrc/lda_estep.hip kTile: the words a wave holds in LDS
DOCS_PER_BLOCK = 2    # csrc/lda_estep.hip kDocs
MAX_UPDATE_ITER = 10000

_COUNTS = {torch.float64: 0, torch.int32: 1, torch.int64: 2}
_F32_COUNTS = ("counts are float32: sklearn would run a float32 E-step on them, which this does not reproduce "
               "(CountVectorizer's int64 counts, or float64, give sklearn's float64 E-step)")


class _Table:
    """The model as the kernel reads it: exp(E[log beta]) transposed, [V x ldt] float64."""

    __slots__ = ("t", "K", "V", "pinned")


def _model_matrix(t, what):
    require_device(t, what)
    if t.dim() != 2 or t.dtype != torch.float64 or t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError(f"{what} must be a non-empty float64 [K x V] tensor, got {t.dtype} {tuple(t.shape)}")
    return t


def check_documents(indptr, indices, counts, device=None):
    """The refusals of a document batch, float32 counts first: -> B.  RuntimeError on float32
    counts, CPU tensors, a tensor off ``device``, wrong dtypes or shapes."""
    if getattr(counts, "dtype", None) == torch.float32:
        raise RuntimeError("TopicInferencer: " + _F32_COUNTS)
    for what, t in (("indptr", indptr), ("indices", indices), ("counts", counts)):
        require_device(t, what)
        if device is not None and t.device != device:
            raise RuntimeError(f"{what} is on {t.device}, the model on {device}")
        if t.dim() != 1:
            raise RuntimeError(f"{what} must be one-dimensional, got {tuple(t.shape)}")
    if indptr.dtype != torch.int32 or indices.dtype != torch.int32 or counts.dtype not in _COUNTS:
        raise RuntimeError(f"indptr and indices must be int32 and counts float64, int32 or int64, got "
                           f"{indptr.dtype}, {indices.dtype}, {counts.dtype}")
    B = indptr.numel() - 1
    if B < 1 or indices.numel() != counts.numel():
        raise RuntimeError(f"indptr holds {indptr.numel()} entries (B + 1, B >= 1), indices {indices.numel()}, "
                           f"counts {counts.numel()}")
    return B


def model_table(K, V, device):
    """The zeroed [V x even(K)] float64 table the kernels read: a word's K values are one row of 16-byte pairs."""
    return torch.zeros((V, (K + 1) // 2 * 2), dtype=torch.float64, device=device)


def kernel_documents(indptr, indices, counts):
    """-> contiguous (indptr, indices, counts) as the entry points take them.  With no word at all,
    indices and counts are one-element stand-ins: the entry points still want addresses."""
    indptr, indices, counts = indptr.contiguous(), indices.contiguous(), counts.contiguous()
    if indices.numel() == 0:
        indices = torch.zeros(1, dtype=torch.int32, device=indptr.device)
        counts = torch.zeros(1, dtype=counts.dtype, device=indptr.device)
    return indptr, indices, counts


def run_estep(table, K, V, indptr, indices, counts, B, alpha, tol, cap, theta=False, gamma=False, iters=False,
              operands=None):
    """gcnk_lda_estep_f64 of checked documents (``kernel_documents``' arrays) under ``table`` (``model_table``'s
    form, current for the model) -> {name: tensor} of the outputs asked for; ``operands``: the threshold of x, a."""
    dev = table.device
    out = {}
    if theta:
        out["theta"] = torch.empty((B, K), dtype=torch.float64, device=dev)
    if gamma:
        out["gamma"] = torch.empty((B, K), dtype=torch.float64, device=dev)
    if iters:
        out["iters"] = torch.empty(B, dtype=torch.int32, device=dev)
    threshold = 0.0
    if operands is not None:
        threshold = float(operands)
        for k in ("x", "a"):   # rows 16-byte aligned: what DocumentScorer takes without a copy
            out[k] = torch.empty((B, (K + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :K]
    ptr = lambda k: out[k].data_ptr() if k in out else None   # noqa: E731
    ld = lambda k: out[k].stride(0) if k in out else 0        # noqa: E731
    with torch.cuda.device(dev):
        rc = _lib.load().gcnk_lda_estep_f64(
            indptr.data_ptr(), indices.data_ptr(), counts.data_ptr(), _COUNTS[counts.dtype], B, V, K,
            table.data_ptr(), table.stride(0), alpha, tol, cap, ptr("theta"), K, ptr("gamma"), ptr("iters"), ptr("x"),
            ld("x"), ptr("a"), ld("a"), threshold, _lib.stream(dev))
    _lib.check(rc, "gcnk_lda_estep_f64")   # (no fallback: a shape the kernel refuses is an error)
    return out


class TopicInferencer:
    """theta of unseen documents under a fitted LDA model.

    ``exp_topic_word`` [K x V] float64 on the device is sklearn's
    ``exp_dirichlet_component_``; ``doc_topic_prior`` its ``doc_topic_prior_``.
    The transposed table the kernel reads is built here and held while
    derived.stamp() of the model tensor is unchanged (derived.py's one rule):
    an in-place change of the model rebuilds it on the next call."""

    def __init__(self, exp_topic_word, doc_topic_prior, mean_change_tol=1e-3, max_doc_update_iter=100,
                 _from_components=False):
        self._src = _model_matrix(exp_topic_word, "components" if _from_components else "exp_topic_word")
        self._lambda = bool(_from_components)
        self.K, self.V = self._src.shape
        self.doc_topic_prior = float(doc_topic_prior)
        self.mean_change_tol = float(mean_change_tol)
        self.max_doc_update_iter = int(max_doc_update_iter)
        if not 0 <= self.max_doc_update_iter <= MAX_UPDATE_ITER:
            raise RuntimeError(f"max_doc_update_iter={max_doc_update_iter} is outside [0, {MAX_UPDATE_ITER}]")
        self._cache = Cache(1)
        self._table()

    @classmethod
    def from_components(cls, components, doc_topic_prior, mean_change_tol=1e-3, max_doc_update_iter=100):
        """From lambda (sklearn's ``components_``, [K x V] float64 on the device):
        exp(psi(lambda) - psi(row sum)) is computed on the device, straight into the table."""
        return cls(components, doc_topic_prior, mean_change_tol, max_doc_update_iter, _from_components=True)

    @classmethod
    def from_sklearn(cls, lda, device="cuda"):
        """From a fitted ``LatentDirichletAllocation`` (duck-typed: its
        ``exp_dirichlet_component_``, ``doc_topic_prior_``, ``mean_change_tol`` and
        ``max_doc_update_iter``); the model matrix is uploaded to ``device``."""
        e = torch.as_tensor(lda.exp_dirichlet_component_)
        if e.dtype != torch.float64:
            raise RuntimeError(f"exp_dirichlet_component_ is {e.dtype}: only sklearn's float64 model is reproduced")
        return cls(e.to(device), lda.doc_topic_prior_, lda.mean_change_tol, lda.max_doc_update_iter)

    def _table(self):
        tb = self._cache.get("table", (self._src,), self._build)
        if torch.cuda.is_current_stream_capturing():
            tb.pinned = True   # (a captured launch keeps reading the table: derived.py)
        return tb

    def _build(self):
        src = self._src
        if src.stride(1) != 1 or src.stride(0) < src.shape[1]:
            src = src.contiguous()
        K, V = src.shape
        tb = _Table()
        tb.K, tb.V, tb.pinned = K, V, False
        tb.t = model_table(K, V, src.device)
        lib = _lib.load()
        name = "gcnk_lda_exp_dirichlet_f64" if self._lambda else "gcnk_lda_table_from_exp_f64"
        with torch.cuda.device(src.device):
            _lib.check(getattr(lib, name)(src.data_ptr(), src.stride(0), K, V, tb.t.data_ptr(), tb.t.stride(0),
                                          _lib.stream(src.device)), name)
        return tb

    @property
    def exp_topic_word(self):
        """exp(E[log beta]) [K x V] float64 as the held table has it (a transposed view)."""
        tb = self._table()
        return tb.t[:, :tb.K].t()

    def _run(self, indptr, indices, counts, **outputs):
        tb = self._table()
        B = check_documents(indptr, indices, counts, tb.t.device)
        return run_estep(tb.t, tb.K, tb.V, *kernel_documents(indptr, indices, counts), B, self.doc_topic_prior,
                         self.mean_change_tol, self.max_doc_update_iter, **outputs)

    def __call__(self, indptr, indices, counts, return_iterations=False):
        """theta, float64 [B x K] on the model's device (sklearn's ``transform``); with
        ``return_iterations`` also the updates each document ran, int32 [B]."""
        out = self._run(indptr, indices, counts, theta=True, iters=return_iterations)
        return (out["theta"], out["iters"]) if return_iterations else out["theta"]

    def gamma(self, indptr, indices, counts):
        """The unnormalised gamma, float64 [B x K] (sklearn's ``_unnormalized_transform``);
        theta is gamma over its sum taken in ascending topic order."""
        return self._run(indptr, indices, counts, gamma=True)["gamma"]

    def scorer_operands(self, indptr, indices, counts, threshold):
        """(x, a) fp32 [B x K] for ``DocumentScorer``, written by the launch that infers
        theta: what ``inductive.from_theta(self(...), threshold)`` gives (its two row sums
        taken in ascending topic order).  Rows are 16-byte aligned."""
        out = self._run(indptr, indices, counts, operands=threshold)
        return out["x"], out["a"]


def doc_term(X, device="cuda"):
    """A scipy CSR document-term matrix (CountVectorizer's output) -> (indptr int32,
    indices int32, counts float64) on ``device``, rows in stored order.  Integer and
    float64 counts become float64, as sklearn's input check makes them; float32 is
    refused (RuntimeError)."""
    import numpy as np
    X = X.tocsr() if hasattr(X, "tocsr") else X
    if not all(hasattr(X, k) for k in ("indptr", "indices", "data")):
        raise RuntimeError(f"doc_term takes a scipy sparse matrix, got {type(X)}")
    if X.data.dtype == np.float32:
        raise RuntimeError("doc_term: " + _F32_COUNTS)
    if X.data.dtype != np.float64 and not np.issubdtype(X.data.dtype, np.integer):
        raise RuntimeError(f"doc_term: counts must be integers or float64, got {X.data.dtype}")
    if X.nnz >= 2 ** 31:
        raise RuntimeError(f"doc_term: {X.nnz} entries exceed an int32 CSR")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)   # noqa: E731
    return up(X.indptr, np.int32), up(X.indices, np.int32), up(X.data, np.float64)
