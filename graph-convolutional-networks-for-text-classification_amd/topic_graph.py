"""The doc-topic graph built on the device (csrc/topic_graph.hip): the topic
model's output -> A-hat, the step before everything else in this package.

The reference turns (theta, topic embeddings) into a graph with two Python
loops over every (document, topic) and (topic, topic) pair into an nx.Graph
(build_graph.py:99-133), writes a text edge list, parses it back, symmetrises
and normalises with scipy (trainer.py:98-151).  Here the same A-hat -- bit for
bit -- is written straight into a sorted int32 CSR on theta's device:

    g = build_topic_graph(theta, topic_emb=E)     # thresholds 0.02 / 0.3
    model(g.features, g.adj)                      # g.adj is GCN.forward's adj

An edge (d, D + k) exists iff theta[d, k] >= doc_topic_threshold, compared in
float64, with weight float32(theta[d, k]); an edge (D + i, D + j), i < j, iff
sim[i, j] > topic_topic_threshold (strict; only the upper triangle of
``topic_sim`` is read), with weight float32(sim[i, j]).  Two departures from
the reference: every document and topic is a node even without a kept edge
(its row is the diagonal alone, A-hat = 1.0; the reference's nx.Graph drops
such a node and mis-numbers the rest), and NaN / negative theta is the
caller's error and is not checked (as in ``inductive.from_theta``).
"""
import torch

from . import _lib
from .inductive import from_theta
from .sparse import CSR, require_device

DOCS_PER_BLOCK = 256   # csrc/topic_graph.hip kChunk: documents a workgroup stages (64 a wave)
MAX_TOPICS = 128       # csrc/topic_graph.hip kMaxTopics (factor.MAX_HUBS)

_F32 = {torch.float64: 0, torch.float32: 1}


def _matrix(t, what, shape=None):
    """``t`` as the kernels read it: fp64 / fp32 [rows x cols] on the device with unit column
    stride and rows at least cols apart (anything else is copied once) -> (tensor, f32 flag, ld)."""
    require_device(t, what)
    if t.dim() != 2 or t.dtype not in _F32 or (shape is not None and tuple(t.shape) != shape):
        want = "[rows x cols]" if shape is None else f"[{shape[0]} x {shape[1]}]"
        raise RuntimeError(f"{what} must be float64 or float32 {want}, got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError(f"{what} must not be empty, got {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, _F32[t.dtype], t.stride(0)


def topic_similarity(topic_emb):
    """Cosine similarity of the rows of ``topic_emb`` [K x dim] (fp32 or fp64, on the
    device) as float64 [K x K] on the same device (build_graph.py:118): float64 sums in
    ascending index order; a zero row is similar to nothing (0)."""
    e, f32, lde = _matrix(topic_emb, "topic_emb")
    K, dim = e.shape
    sim = torch.empty((K, K), dtype=torch.float64, device=e.device)
    with torch.cuda.device(e.device):
        _lib.check(_lib.load().gcnk_topic_cosine_f64(e.data_ptr(), f32, lde, K, dim, sim.data_ptr(), K,
                                                     _lib.stream(e.device)), "gcnk_topic_cosine_f64")
    return sim


class TopicGraph:
    """What ``build_topic_graph`` returns: ``adj`` (the CSR of A-hat), the node and
    (undirected) edge counts, and ``features`` (None without ``topic_emb``)."""

    def __init__(self, adj, ndoc, ntopic, doc_topic_edges, topic_topic_edges, theta, topic_emb, threshold):
        self.adj, self.ndoc, self.ntopic = adj, ndoc, ntopic
        self.doc_topic_edges, self.topic_topic_edges = doc_topic_edges, topic_topic_edges
        self._theta, self._emb, self._threshold, self._features = theta, topic_emb, threshold, None

    def __repr__(self):
        return (f"TopicGraph(ndoc={self.ndoc}, ntopic={self.ntopic}, doc_topic_edges={self.doc_topic_edges}, "
                f"topic_topic_edges={self.topic_topic_edges}, adj={self.adj})")

    @property
    def features(self):
        """X as trainer.py:197-238 builds it, a torch sparse COO fp32 [N x max(K, dim)] in
        row-major order without explicit zeros: document rows ``from_theta(theta, .)[0]`` on
        columns 0 .. K-1, topic rows the embedding row over its float64 norm (a zero row stays
        zero).  Plain torch, made on first use (its nonzero() is a host synchronisation of its
        own); None when the graph was built without ``topic_emb``."""
        if self._emb is None:
            return None
        if self._features is None:
            self._features = _features(self._theta, self._emb, self._threshold)
        return self._features


def _features(theta, emb, threshold):
    D, K = theta.shape
    dim = emb.shape[1]
    xd = from_theta(theta, threshold)[0]
    e = emb.to(torch.float64)
    norm = e.square().sum(1, keepdim=True).sqrt()
    xt = (e / torch.where(norm == 0, torch.ones_like(norm), norm)).to(torch.float32)
    id_, it = xd.nonzero().t(), xt.nonzero().t()
    idx = torch.cat([id_, torch.stack([it[0] + D, it[1]])], 1)
    vals = torch.cat([xd[id_[0], id_[1]], xt[it[0], it[1]]])
    return torch.sparse_coo_tensor(idx, vals, (D + K, max(K, dim)))


def build_topic_graph(theta, topic_sim=None, topic_emb=None, doc_topic_threshold=0.02, topic_topic_threshold=0.3):
    """A-hat of the doc-topic graph of ``theta`` [D x K] (fp64 as sklearn returns it, or
    fp32, on the device) as a ``TopicGraph`` on theta's device.  Topic-topic edges come
    from ``topic_sim`` [K x K] or from ``topic_similarity(topic_emb)`` ([K x dim]); give one
    of them or neither (no topic-topic edges).  One host synchronisation, which reads the
    two edge counts (and with them nnz).  RuntimeError on CPU tensors, wrong dtypes or
    shapes, or a shape the kernels refuse; ValueError on a threshold that is not > 0."""
    if topic_sim is not None and topic_emb is not None:
        raise ValueError("build_topic_graph: give topic_sim or topic_emb, not both")
    if not doc_topic_threshold > 0 or not topic_topic_threshold > 0:
        raise ValueError(f"build_topic_graph: thresholds must be > 0 (got {doc_topic_threshold}, "
                         f"{topic_topic_threshold}); 0 would keep explicit zero-weight entries")
    th, th_f32, ldt = _matrix(theta, "theta")
    D, K = th.shape
    dev = th.device
    sim, sim_f32, lds = None, 0, 0
    if topic_emb is not None:
        emb = _matrix(topic_emb, "topic_emb")[0]
        if emb.shape[0] != K or emb.device != dev:
            raise RuntimeError(f"topic_emb must be [{K} x dim] on {dev}, got {tuple(emb.shape)} on {emb.device}")
        topic_emb, topic_sim = emb, topic_similarity(emb)
    if topic_sim is not None:
        sim, sim_f32, lds = _matrix(topic_sim, "topic_sim", (K, K))
        if sim.device != dev:
            raise RuntimeError(f"topic_sim is on {sim.device}, theta on {dev}")
    lib = _lib.load()
    N = D + K
    cap = int(lib.gcnk_topic_graph_nnz_bound(D, K, int(sim is not None)))
    if cap < 0:
        _lib.check(cap, "gcnk_topic_graph_nnz_bound")
    wsb = int(lib.gcnk_topic_graph_workspace_bytes(D, K))
    if wsb < 0:
        _lib.check(wsb, "gcnk_topic_graph_workspace_bytes")
    rp = torch.empty(N + 1, dtype=torch.int32, device=dev)
    ci = torch.empty(cap, dtype=torch.int32, device=dev)
    v = torch.empty(cap, dtype=torch.float32, device=dev)
    edges = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gcnk_topic_graph_build(
            th.data_ptr(), th_f32, ldt, None if sim is None else sim.data_ptr(), sim_f32, lds, D, K,
            float(doc_topic_threshold), float(topic_topic_threshold), rp.data_ptr(), ci.data_ptr(), v.data_ptr(),
            cap, edges.data_ptr(), ws.data_ptr(), wsb, _lib.stream(dev)), "gcnk_topic_graph_build")
    ndt, ntt = edges.tolist()   # the one synchronisation
    nnz = N + 2 * (ndt + ntt)
    # (copies of the used part: the capacity-sized buffers are released)
    adj = CSR(rp, ci[:nnz].clone(), v[:nnz].clone(), (N, N))
    return TopicGraph(adj, D, K, ndt, ntt, th, topic_emb, doc_topic_threshold)
