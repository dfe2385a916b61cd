/*
 * gcnk_lda.h — the part of libgcnk.so's C-ABI that is the topic model: sklearn's
 * LatentDirichletAllocation transform, batch and online fit, and its variational
 * bound, score and perplexity (everything csrc/lda_estep.hip exports).
 * include/gcnk.h includes this file, so a C caller sees one ABI; it is a file of
 * its own in gcnk.h's form (_lib.py reads every public header with the same
 * reader): a header per family.
 */
#ifndef GCNK_LDA_H_
#define GCNK_LDA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Documents' topic mixtures on the device (csrc/lda_estep.hip; additions within
 * ABI 13): the LDA E-step behind topic_model.py:133-164, sklearn's
 * LatentDirichletAllocation.transform, restated in float64 with sklearn's own
 * rules -- its AS 103 psi (_online_lda_fast.pyx, not an accurate digamma),
 * gamma = 1 at the start, eps = 2^-52 added to phi, the mean-change stop rule
 * taken after the prior is added.
 *
 * The model is held as a transposed table [V x ldt] float64, ldt even and >= K,
 * 16-byte aligned, V * ldt * 8 < 2^31 - 2^20: table[w * ldt + k] =
 * exp(E[log beta_kw]).  Columns K .. ldt-1 are never read into a sum and never
 * written.
 *   gcnk_lda_exp_dirichlet_f64   from components (lambda, [K x V], row stride
 *       ldc): exp(psi(lambda_kw) - psi(sum_w lambda_kw)), the row sum serial and
 *       ascending in w (_dirichlet_expectation_2d, then exp).
 *   gcnk_lda_table_from_exp_f64  the transpose of a model's own
 *       exp_dirichlet_component_ ([K x V], row stride lde), bit for bit.
 *
 * gcnk_lda_estep_f64: B documents as a CSR over the vocabulary -- indptr
 * int32[B + 1], indices int32, counts float64 / int32 / int64 (counts_kind 0 /
 * 1 / 2, widened exactly) -- one wave each, one launch:
 *     gamma = 1;  etheta_k = exp(psi(1) - psi(K))
 *     at most max_iter times:
 *       phi_w    = sum_k etheta_k table[id_w, k] + 2^-52
 *       gamma'_k = etheta_k * sum_w (c_w / phi_w) table[id_w, k] + alpha
 *       etheta_k = exp(psi(gamma'_k) - psi(sum_k gamma'_k))
 *       stop after this update if sum_k |gamma_k - gamma'_k| / K < tol
 *     theta = gamma / sum_k gamma
 * Sums over k ascend, sums over a document's words run in stored order (the two
 * dot products by fma, nothing else contracted): a document's row depends on its
 * own words and K alone, not on B, its place in the batch or the launch.  No
 * atomics, no workspace, no synchronisation.  Outputs, each nullable:
 *   theta, gamma  float64 [B x ldth]  (gamma: sklearn's _unnormalized_transform)
 *   iters         int32 [B], the updates run (0 .. max_iter)
 *   x, a          fp32 [B x ldx], [B x lda], given together: what
 *       gcnk_score_docs_f32 reads, made from this launch's theta as the
 *       reference makes them (trainer.py:205-221, build_graph.py:105-110):
 *       x = theta / (sum_k theta + 1e-8) rounded to fp32, over its float64 L2
 *       norm (a zero row stays zero), rounded to fp32; a = fp32(theta) where
 *       theta >= threshold in float64, else 0.  The two sums ascend in k.
 * A word id outside [0, V) is the caller's error and is not checked on the
 * device (the table is read through a bounds-checked buffer resource: such an id
 * reads another row or zeros).  indptr must ascend within the arrays given.
 * GCNK_EARG: B < 1, K < 1, V < 1, a null input, a bad table (see above),
 * counts_kind outside 0..2, max_iter outside [0, 10000], x without a or a
 * without x, no output at all, a leading dimension < K.  GCNK_EUNSUP: K >
 * gcnk_lda_max_topics() (128), a table past 32-bit byte offsets.  Every refusal
 * comes before any HIP call.  gcnk_lda_tile_words(): the words a wave holds in
 * LDS (64; a longer document walks chunks of that many, re-read every update);
 * gcnk_lda_docs_per_block(): waves per workgroup (2).
 * ------------------------------------------------------------------------- */
int32_t gcnk_lda_max_topics(void);
int32_t gcnk_lda_tile_words(void);
int32_t gcnk_lda_docs_per_block(void);
int gcnk_lda_exp_dirichlet_f64(const double* components, int64_t ldc, int32_t K, int32_t V, double* table, int64_t ldt,
                               void* stream);
int gcnk_lda_table_from_exp_f64(const double* exp_topic_word, int64_t lde, int32_t K, int32_t V, double* table,
                                int64_t ldt, void* stream);
int gcnk_lda_estep_f64(const int32_t* indptr, const int32_t* indices, const void* counts, int32_t counts_kind,
                       int32_t B, int32_t V, int32_t K, const double* table, int64_t ldt, double alpha, double tol,
                       int32_t max_iter, double* theta, int64_t ldth, double* gamma, int32_t* iters, float* x,
                       int64_t ldx, float* a, int64_t lda, double threshold, void* stream);

/* ---------------------------------------------------------------------------
 * The topic model fitted on the device (csrc/lda_estep.hip; additions within
 * ABI 13): sklearn's batch variational EM behind topic_model.py:74-131,
 * LatentDirichletAllocation.fit with learning_method='batch' (_lda.py
 * _em_step(batch_update=True)), all float64.  One EM iteration is three
 * launches on one stream, none of which synchronises:
 *   gcnk_lda_exp_dirichlet_f64   the table from lambda (above)
 *   gcnk_lda_estep_fit_f64       the update loop of gcnk_lda_estep_f64, the same
 *       device code instantiated a second time, started from gamma0 [B x ldg0]
 *       (sklearn's fresh Gamma(100, .01) draw of every EM iteration) instead of
 *       1: etheta_k = exp(psi(gamma0_k) - psi(sum_k gamma0_k)), the sum ascending.
 *       After the loop it walks the document's words once more with the final
 *       etheta: ratio[indptr[d] + w] = c_w / (sum_k etheta_k table[id_w, k] +
 *       2^-52), one per stored nonzero in CSR order (nnz of them), and stores
 *       etheta [B x lde]; gamma [B x ldg] and iters int32 [B] are nullable.
 *   gcnk_lda_mstep_f64           lambda[k * ldl + w] = eta + S_kw * table[w, k],
 *       S_kw = sum over the documents d that hold w, ASCENDING d, of
 *       etheta[d, k] * ratio[its entry]: the product rounded, then added (as
 *       np.outer and += do; no fma, no atomics), one wave per word and no word's
 *       chain split, so lambda is bit for bit that serial loop.  The word-major
 *       index of the document-term matrix: wptr int32 [V + 1] (word w's entries
 *       are [wptr[w], wptr[w + 1])), pos int32 [nnz] (an entry's position in CSR
 *       order, so in ratio) and doc int32 [nnz] (its document), a word's entries
 *       in ascending document order (a stable sort of indices).  A word no
 *       document holds gets exactly eta.
 * The M-step's chain runs over [wptr[w], wptr[w + 1]) clamped to [0, nnz]; ratio
 * and etheta are accessed through bounds-checked buffer resources (a bad pos or
 * doc reads zeros, a bad indptr stores nothing outside ratio).
 * GCNK_EARG: B < 1, K < 1, V < 1, a null pointer (gamma and iters excepted), a
 * bad table, counts_kind outside 0..2, max_iter outside [0, 10000], a leading
 * dimension below K (ldl below V), nnz < 0.  GCNK_EUNSUP: K > 128, a table, nnz
 * ratios or an etheta of B * lde doubles past 32-bit byte offsets (2^31 - 2^20).
 * Every refusal comes before any HIP call.  gcnk_lda_words_per_block(): the
 * M-step's waves per workgroup (4).
 * ------------------------------------------------------------------------- */
int32_t gcnk_lda_words_per_block(void);
int gcnk_lda_estep_fit_f64(const int32_t* indptr, const int32_t* indices, const void* counts, int32_t counts_kind,
                           int32_t B, int32_t V, int32_t K, const double* table, int64_t ldt, double alpha, double tol,
                           int32_t max_iter, const double* gamma0, int64_t ldg0, int64_t nnz, double* ratio,
                           double* etheta, int64_t lde, double* gamma, int64_t ldg, int32_t* iters, void* stream);
int gcnk_lda_mstep_f64(const int32_t* wptr, const int32_t* pos, const int32_t* doc, int64_t nnz, const double* ratio,
                       const double* etheta, int64_t lde, int32_t B, int32_t V, int32_t K, const double* table,
                       int64_t ldt, double eta, double* lambda, int64_t ldl, void* stream);

/* ---------------------------------------------------------------------------
 * The topic model fitted ONLINE on the device (csrc/lda_estep.hip; an addition
 * within ABI 13): sklearn's minibatch variational EM, learning_method='online'
 * and partial_fit (_lda.py _em_step(batch_update=False)), which the reference's
 * TopicModel offers as learning_method (topic_model.py:46,55,113).  A minibatch
 * of documents [doc_lo, doc_hi) is three launches on one stream:
 *   gcnk_lda_exp_dirichlet_f64   the table from the current lambda
 *   gcnk_lda_estep_fit_f64       on the row range: indptr + doc_lo, B = doc_hi -
 *       doc_lo, gamma0 and etheta advanced by doc_lo rows, the WHOLE ratio and
 *       nnz (a ratio is stored at its absolute CSR position)
 *   gcnk_lda_mstep_online_f64    for every word w and topic k, in place, every
 *       line one correctly rounded float64 operation (no fma, no atomics):
 *           S   = sum over w's entries whose document d is in [doc_lo, doc_hi),
 *                 ASCENDING d, of etheta[d, k] * ratio[its entry] (the product
 *                 rounded, then added: gcnk_lda_mstep_f64's chain, the same code)
 *           ss  = S * table[w, k]
 *           t   = doc_ratio * ss
 *           u   = eta + t
 *           v   = rho * u
 *           a   = lambda[k * ldl + w] * (1.0 - rho)
 *           lambda[k * ldl + w] = a + v
 *       wptr / pos / doc are the word-major index of the WHOLE matrix, the one
 *       gcnk_lda_mstep_f64 takes; etheta is [B x lde] with the minibatch's rows
 *       filled.  A word's entries ascend in document, so the minibatch's are a
 *       contiguous sub-range of [wptr[w], wptr[w + 1]) (clamped to [0, nnz]),
 *       found on the device by a lower-bound search on doc for doc_lo and for
 *       doc_hi: no index is built per minibatch.  A word the minibatch does not
 *       hold is blended with S = 0.  rho = (learning_offset + n_batch_iter) ^
 *       -learning_decay is the caller's (float64, on the host); 1.0 - rho is
 *       formed from it once; rho = 1 gives a = +0.  doc_ratio = total_samples /
 *       (doc_hi - doc_lo).
 * GCNK_EARG: gcnk_lda_mstep_f64's (B < 1, K < 1, V < 1, a null pointer, a bad
 * table, lde < K, ldl < V, nnz < 0), doc_lo < 0, doc_hi > B, doc_lo >= doc_hi,
 * rho outside (0, 1] or not finite, doc_ratio not finite or <= 0.  GCNK_EUNSUP:
 * K > 128, a table, nnz ratios or an etheta past 32-bit byte offsets.  Every
 * refusal comes before any HIP call.
 * ------------------------------------------------------------------------- */
int gcnk_lda_mstep_online_f64(const int32_t* wptr, const int32_t* pos, const int32_t* doc, int64_t nnz, int32_t doc_lo,
                              int32_t doc_hi, const double* ratio, const double* etheta, int64_t lde, int32_t B,
                              int32_t V, int32_t K, const double* table, int64_t ldt, double eta, double rho,
                              double doc_ratio, double* lambda, int64_t ldl, void* stream);

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
 * GCNK_EARG: B < 1, K < 1, V < 1, a null pointer, a bad table (above), ldg < K,
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

#endif /* GCNK_LDA_H_ */
