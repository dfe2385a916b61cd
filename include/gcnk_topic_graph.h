/*
 * gcnk_topic_graph.h — the part of libgcnk.so's C-ABI that builds the doc-topic
 * graph: the topic model's output to the CSR of A-hat, and the topics' cosine
 * similarities (csrc/topic_graph.hip).  include/gcnk.h includes this file, so a
 * C caller sees one ABI; it is a file of its own in gcnk.h's form (_lib.py reads
 * every public header with the same reader): a header per family.
 */
#ifndef GCNK_TOPIC_GRAPH_H_
#define GCNK_TOPIC_GRAPH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * The doc-topic graph built on the device (csrc/topic_graph.hip; additions
 * within ABI 13): the topic model's output -> the CSR of A-hat, without the
 * nx.Graph, the text edge list and scipy of build_graph.py:99-133 and
 * trainer.py:98-151.  N = D + K nodes: documents 0 .. D-1, topics D .. N-1.
 *   theta [D x K], sim [K x K] (nullable: no topic-topic edges): row-major
 *     fp64 (*_f32 = 0) or fp32 (*_f32 = 1, widened exactly), leading
 *     dimensions ldt / lds in elements.
 *   edge (d, D+k)    iff theta[d,k] >= doc_topic_threshold, in float64
 *                    (build_graph.py:106), weight float32(theta[d,k]);
 *   edge (D+i, D+j)  i < j, iff sim[i,j] > topic_topic_threshold (strict,
 *                    build_graph.py:124), weight float32(sim[i,j]); the lower
 *                    triangle and the diagonal of sim are never read;
 *   A_hat = D^-1/2 (A + I) D^-1/2 with gcnk_sym_normalize's arithmetic: float64
 *     row sums taken sequentially in ascending column order with the diagonal
 *     at its sorted place, d = rowsum^-0.5 (inf -> 0), (d[r] a) d[c] rounded
 *     to fp32 once -- bit for bit what the reference's path gives.
 * Unlike the reference, a document or topic without a kept edge is still a
 * node (its row is the diagonal alone, A_hat = 1.0), and NaN / negative theta
 * is not looked for (a NaN compares false and is dropped).
 * Output: rowptr int32[N + 1] (rowptr[N] = nnz, readable once the stream
 * completes), colind / val of `capacity` >= gcnk_topic_graph_nnz_bound(D, K,
 * sim != NULL) entries, columns ascending in every row; edges (nullable)
 * int32[2] = doc-topic edges, topic-topic edges (undirected counts:
 * nnz = N + 2 (edges[0] + edges[1])).  Nothing is allocated; six launches on
 * `stream`.  GCNK_EARG: D < 1, K < 1, a threshold not > 0 (0 would keep
 * explicit zeros), a null pointer, a leading dimension < K, a short capacity
 * or workspace.  GCNK_EUNSUP: K > gcnk_topic_graph_max_topics() (128), or
 * N + the nnz bound >= 2^31.  Every refusal comes before any HIP call.
 * gcnk_topic_graph_chunk(): documents per workgroup (256) -- a topic column's
 * entries are ranked per 64-document segment of such a chunk, in order.
 * ------------------------------------------------------------------------- */
int32_t gcnk_topic_graph_chunk(void);
int32_t gcnk_topic_graph_max_topics(void);
int64_t gcnk_topic_graph_nnz_bound(int32_t D, int32_t K, int32_t has_sim);
int64_t gcnk_topic_graph_workspace_bytes(int32_t D, int32_t K);
int gcnk_topic_graph_build(const void* theta, int32_t theta_f32, int64_t ldt, const void* sim, int32_t sim_f32,
                           int64_t lds, int32_t D, int32_t K, double doc_topic_threshold,
                           double topic_topic_threshold, int32_t* rowptr, int32_t* colind, float* val,
                           int64_t capacity, int32_t* edges, void* workspace, int64_t workspace_bytes, void* stream);
/* sim [K x K] fp64 = the cosine similarity of the rows of emb [K x dim] (fp64,
 * or fp32 with emb_f32 = 1), build_graph.py:118: dot products and squared
 * norms as float64 sums in ascending index order, dot / (|a| |b|); a zero row
 * gives 0.  sim is written symmetric, diagonal included. */
int gcnk_topic_cosine_f64(const void* emb, int32_t emb_f32, int64_t lde, int32_t K, int32_t dim, double* sim,
                          int64_t lds, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GCNK_TOPIC_GRAPH_H_ */
