"""MI355X-native GCN hot path (gfx950 HIP kernels behind a C-ABI).

Drop-in for the reference's ``layer.py`` (GraphConvolution, GCN) — see
DESIGN.md for the path, the boundary and the kernels.
"""
from . import (_lib, datasets, inductive, metrics, parallel, sparse, text_count, topic_bound, topic_fit, topic_graph,
               topic_infer, train)
from .inductive import DocumentScorer, from_theta
from .layer import GCN, GraphConvolution
from .ops import GCNFn, GraphConvFn, Operand, colsum, gemm, spmm
from .parallel import ColumnShardedSpMM, shard_bounds, sharded_gcn_forward
from .sparse import CSR, as_csr, from_arrays, from_torch, preprocess_adj
from .text_count import TextCounter
from .topic_bound import TopicBound
from .topic_fit import OnlineTopics, TopicFit, fit_topics
from .topic_graph import TopicGraph, build_topic_graph, topic_similarity
from .topic_infer import TopicInferencer, doc_term
from .train import Adam, BestKeeper, EpochLog, FitResult, IndexedCrossEntropy, cross_entropy, fit, run_epoch

__all__ = [
    "datasets", "inductive", "metrics", "parallel", "sparse", "topic_bound", "topic_fit", "topic_graph", "topic_infer",
    "train", "text_count", "TextCounter", "DocumentScorer", "TopicBound", "TopicFit", "fit_topics", "OnlineTopics",
    "from_theta", "TopicGraph", "build_topic_graph", "topic_similarity", "TopicInferencer", "doc_term",
    "Adam", "IndexedCrossEntropy", "cross_entropy",
    "EpochLog", "BestKeeper", "FitResult", "fit", "run_epoch",
    "GCN", "GraphConvolution", "GCNFn", "GraphConvFn", "Operand", "CSR",
    "as_csr", "from_arrays", "from_torch", "preprocess_adj", "spmm", "gemm", "colsum",
    "ColumnShardedSpMM", "shard_bounds", "sharded_gcn_forward",
]


def native_library_path():
    """Path of the in-tree libgcnk.so this package runs on."""
    return _lib.LIB_PATH
