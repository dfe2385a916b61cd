/*
 * gcnk_lda_bound.h — the part of libgcnk.so's C-ABI that evaluates a topic
 * model: sklearn's variational bound, score and perplexity.  include/gcnk.h
 * includes this file, so a C caller sees one ABI; it is a file of its own in
 * gcnk.h's form (_lib.py reads both with the same reader) so that gcnk.h's own
 * list of entry points stays the one its tests count.
 */
#ifndef GCNK_LDA_BOUND_H_
#define GCNK_LDA_BOUND_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * The topic model's variational bound on the device (csrc/lda_estep.hip;
 * additions within ABI 13): sklearn's LatentDirichletAllocation._approx_bound,
 * score, perplexity and bound_ (_lda.py), all float64, which tell whether the
 * num_topics / max_iter of the reference's experiments/r8.yaml were well
 * chosen.  With E[log theta_dk] = psi(gamma_dk) - psi(sum_k gamma_dk) and
 * E[log beta_kw] = psi(lambda_kw) - psi(sum_w lambda_kw), psi sklearn's AS 103:
 *     doc_d   = sum_w c_dw logsumexp_k(E[log theta_dk] + E[log beta_kw])
 *             + sum_k (alpha - gamma_dk) E[log theta_dk]
 *             + sum_k (lgamma(gamma_dk) - lgamma(alpha))
 *             + lgamma(alpha K) - lgamma(sum_k gamma_dk)
 *     topic_k = sum_w (eta - lambda_kw) E[log beta_kw]
 *             + sum_w (lgamma(lambda_kw) - lgamma(eta))
 *             + lgamma(eta V) - lgamma(sum_w lambda_kw)
 *     bound   = doc_ratio sum_d doc_d + sum_k topic_k
 *     perplexity = exp(-bound / (doc_ratio sum c))
 * Three launches on one stream, none of which synchronises; no atomics, no
 * workspace, every sum in a fixed order, so a result is bitwise reproducible.
 * "The wave tree": 64 values summed in adjacent pairs, then those sums in
 * pairs, six levels.  "The block tree" of a workgroup: each wave's tree, then
 * the waves' sums one after the other in ascending wave order.
 *
 *   gcnk_lda_bound_docs_f64    doc_bound[d] = doc_d for the B documents of a CSR
 *       (as gcnk_lda_estep_f64 takes it) under the table [V x ldt] of
 *       exp(E[log beta]) and gamma [B x ldg], one wave per document.  The
 *       logsumexp shifts theta's side only -- m = max_k E[log theta_dk], e_k =
 *       exp(E[log theta_dk] - m), word term = c_w (m + log(sum_k e_k
 *       table[id_w, k])) -- so it takes one logarithm a word and reads the table
 *       the E-step reads.  (A prior so small that exp(E[log beta]) underflows to
 *       0 for every topic of a word gives -inf here where logsumexp would not:
 *       sklearn's own E-step divides by 2^-52 for such a word.)  Sums over k
 *       ascend; a document's words go in stored order in tiles of
 *       gcnk_lda_tile_words() = 64, a tile's terms by the wave tree, the tiles'
 *       sums one after the other; doc_d = ((words + second line) + third) +
 *       fourth.  A document without a word is its last three lines.  A
 *       document's value depends on its words, its gamma row and K alone.
 *   gcnk_lda_bound_topics_f64  topic_bound[k] = topic_k of lambda [K x ldl], a
 *       workgroup per topic.  sum_w lambda_kw is serial and ascending, as
 *       gcnk_lda_exp_dirichlet_f64 takes it.  Each of the two sums over w:
 *       thread t of gcnk_lda_bound_topic_chunk() = 256 adds the words t, t +
 *       256, ... in ascending order, then the block tree; topic_k = (first line
 *       + second) + third.
 *   gcnk_lda_bound_finish_f64  one workgroup of 1024: out[0] = bound, out[1] =
 *       the word count sum of counts[indptr[0] .. indptr[B]), out[2] = the
 *       perplexity exp(-(bound / (count * doc_ratio))); out is float64 [3].
 *       Each sum (doc_bound[B], topic_bound[K], the counts): thread t adds the
 *       elements t, t + 1024, ... ascending, then the block tree; int32 / int64
 *       counts are summed exactly in int64.  doc_ratio is 1, or total_samples /
 *       B for sklearn's sub_sampling.  For a row range of a larger matrix pass
 *       indptr advanced to the range's first row with the WHOLE indices and
 *       counts, as gcnk_lda_estep_fit_f64's callers do.
 * GCNK_EARG: B < 1, K < 1, V < 1, a null pointer, a bad table (gcnk.h), ldg < K,
 * ldl < V, counts_kind outside 0..2, doc_ratio not finite or <= 0.
 * GCNK_EUNSUP: K > gcnk_lda_max_topics() (128); a table past 32-bit byte
 * offsets (the table alone is read through a buffer resource: gamma, lambda and
 * the partials are indexed in 64 bits).  Every refusal comes before any HIP call.
 * ------------------------------------------------------------------------- */
int32_t gcnk_lda_bound_topic_chunk(void);
int gcnk_lda_bound_docs_f64(const int32_t* indptr, const int32_t* indices, const void* counts, int32_t counts_kind,
                            int32_t B, int32_t V, int32_t K, const double* table, int64_t ldt, const double* gamma,
                            int64_t ldg, double alpha, double* doc_bound, void* stream);
int gcnk_lda_bound_topics_f64(const double* lambda, int64_t ldl, int32_t K, int32_t V, double eta, double* topic_bound,
                              void* stream);
int gcnk_lda_bound_finish_f64(const double* doc_bound, int32_t B, const double* topic_bound, int32_t K,
                              const int32_t* indptr, const void* counts, int32_t counts_kind, double doc_ratio,
                              double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GCNK_LDA_BOUND_H_ */
