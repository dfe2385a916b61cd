/*
 * gcnk.h — C-ABI of libgcnk.so, the MI355X (gfx950) kernels behind the
 * drop-in GraphConvolution / GCN modules.
 *
 * The reference (anargh-t/Graph-Convolutional-Networks-for-Text-Classification)
 * has no native code: every arithmetic site on its hot path is a call into
 * ATen.  Each entry point below replaces one of those call sites:
 *
 *   layer.py:102  support = th.spmm(infeatn, W)   sparse X  -> gcnk_spmm_csr_f32 (X in CSR)
 *                                                 dense  H  -> gcnk_gemm_f32 (fp32 MFMA)
 *   layer.py:106  output  = th.spmm(adj, support)          -> gcnk_spmm_csr_f32 (A-hat in CSR)
 *   layer.py:110  output + bias                             -> fused epilogue (GCNK_EPI_BIAS*)
 *   layer.py:182  th.relu                                   -> fused epilogue (GCNK_EPI_BIAS_RELU)
 *   layer.py:185  th.dropout(x, p, train)                   -> fused epilogue (GCNK_EPI_*_DROP*)
 *   autograd of :102/:106/:110 (trainer.py:361 loss.backward())
 *                  A^T g, X^T g                             -> gcnk_spmm_csr_f32 on cached transposes
 *                  H^T g, g W^T, relu/dropout mask          -> gcnk_gemm_f32 (+GCNK_GEMM_EPI_MASK_POS)
 *                  sum over rows of g  (bias grad)          -> gcnk_colsum_f32
 *   utils.py:196-203 / trainer.py:226-238 (COO tensors handed to th.spmm)
 *                                                           -> gcnk_coo_to_csr + gcnk_spmm_plan_build (one-time)
 *   utils.py:185-213 preprocess_adj / normalize_adj          -> gcnk_sym_normalize (device, bit-exact)
 *   utils.py:25-109  accuracy / macro_f1 counts              -> gcnk_class_stats (one launch, no per-class syncs)
 *   trainer.py:98-148 edge list -> symmetric adjacency        -> gcnk_edgelist_size / _csr (host, no networkx)
 *   build_graph.py:99-133 theta, topic similarities -> graph   -> gcnk_topic_graph_build (device, straight to A-hat)
 *   build_graph.py:118 cosine_similarity(topic_embeddings)     -> gcnk_topic_cosine_f64
 *                                                            (both in gcnk_topic_graph.h, included below)
 *   topic_model.py:133-164 LatentDirichletAllocation.transform -> gcnk_lda_estep_f64 (device, a wave per document)
 *   topic_model.py:74-131  LatentDirichletAllocation.fit (batch) -> gcnk_lda_estep_fit_f64 + gcnk_lda_mstep_f64
 *   experiments/r8.yaml num_topics, max_iter: LatentDirichletAllocation.score / perplexity / bound_
 *                                                            -> gcnk_lda_bound_*_f64
 *                                                            (every gcnk_lda_* in gcnk_lda.h, included below)
 *   topic_model.py:159 CountVectorizer.transform (unseen text) -> gcnk_text_count + gcnk_text_emit (gcnk_text.h, below)
 *   layer.py:185 th.dropout keep-mask draw (CPU generator)    -> gcnk_bernoulli_mt19937 (host, same stream)
 *   trainer.py:307, 358-361, 383-384 CrossEntropyLoss on logits[idx] -> gcnk_ce_forward_f32 / gcnk_ce_backward_f32
 *   trainer.py:308, 359, 362 th.optim.Adam step (and zero_grad)   -> gcnk_adam_f32 (one launch per 8 tensors)
 *   utils.py:244, 254, 257-262 EarlyStopping.save_checkpoint      -> gcnk_keep_best_f32 (one launch per 8 tensors)
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless a parameter says "host".
 *   - Dense matrices are row-major fp32 with an explicit leading dimension.
 *   - CSR uses int32 row pointers / column indices (callers check < 2^31);
 *     element offsets into dense matrices are 64-bit.
 *   - Every call is asynchronous on `stream` (a hipStream_t; NULL = default
 *     stream).  No entry point allocates or frees device memory, and none
 *     synchronises, except gcnk_spmm_plan_query which is documented as a
 *     one-time setup sync.  All entry points are safe to capture in a hipGraph.
 *   - Return 0 on success; GCNK_EARG (-1) bad argument/shape, GCNK_EUNSUP (-2)
 *     unsupported configuration, GCNK_EHIP (-3) HIP launch/runtime error.
 *     The message is in a thread-local buffer returned by gcnk_last_error().
 *   - Reentrant and thread-safe: no global mutable state besides the
 *     thread-local error text (and a per-kernel one-time LDS-limit attribute).
 *     Calls that may run concurrently (two streams, the autograd thread beside
 *     the caller's) must not share a workspace or a counter region; plans
 *     are read-only after gcnk_spmm_plan_build and may be shared freely.
 */
#ifndef GCNK_H_
#define GCNK_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI note: 13 also covers gcnk_factor_diag_f32, gcnk_hubfactor_gc2_f32, the
 * gc2_* fields at the end of gcnk_gcn_fwd and the route reports
 * gcnk_gcn_bwd2_route / gcnk_hubfactor_gc1_route / gcnk_spmm_route / gcnk_dense_gc1_route and held-graph scoring,
 * gcnk_score_docs_f32 / gcnk_score_docs_route, and the graph built on the
 * device, gcnk_topic_graph_* / gcnk_topic_cosine_f64, and the topic mixtures
 * inferred and the topic model fitted on the device, gcnk_lda_* (additions only: no existing
 * symbol, field offset or meaning changed, so the number stayed). */
#define GCNK_ABI_VERSION 13

#define GCNK_OK 0
#define GCNK_EARG (-1)
#define GCNK_EUNSUP (-2)
#define GCNK_EHIP (-3)

/* SpMM epilogues (applied once per finished output row element).
 * keep-mask semantics follow ATen's dropout (noise = bernoulli(1-p)/(1-p),
 * out = x * noise): an element is kept where mask != 0 and multiplied by
 * drop_scale. */
#define GCNK_EPI_NONE 0
#define GCNK_EPI_BIAS 1            /* + bias[col]                      layer.py:110 */
#define GCNK_EPI_BIAS_RELU 2       /* relu(. + bias)                   layer.py:110,182 */
#define GCNK_EPI_BIAS_RELU_DROP 3  /* relu(.+bias) * (mask?scale:0)    layer.py:110,182,185 */
#define GCNK_EPI_BIAS_RELU_HASH 4  /* as 3 with an in-kernel counter-based RNG mask */
/* HASH: element (r, c) is kept iff hash(seed, base + offset + r*ldm + c) <
 * keep_prob, base = *rng_base (a device uint64 read by the kernel; 0 when
 * rng_base is NULL).  A caller replaying a captured graph advances *rng_base
 * on the device after each call (the GCN module adds rows*ldm), so every
 * replay draws a fresh mask with no host involvement. */

/* GEMM epilogues */
#define GCNK_GEMM_EPI_NONE 0
#define GCNK_GEMM_EPI_BIAS 1
#define GCNK_GEMM_EPI_BIAS_RELU 2
#define GCNK_GEMM_EPI_MASK_POS 5   /* C = (R[m,n] > 0) ? acc*scale : 0   (relu+dropout backward) */

int gcnk_abi_version(void);
const char* gcnk_last_error(void);

/* ---------------------------------------------------------------------------
 * CSR SpMM:  C[M x F] = epi( A[M x K] (CSR) * B[K x F] )
 * Replaces th.spmm(adj, support) (layer.py:106) and th.spmm(X, W)
 * (layer.py:102, sparse X) and their autograd (A^T g, X^T g).
 *
 * The operand is converted once (gcnk_spmm_plan_build) into a ROW-UNIT + TILE
 * plan (magic 'GNK5'):
 *  - dense blocks: rows are grouped by off-diagonal degree class (factor-8
 *    buckets, row order within a class) into blocks of 64; a block whose
 *    nonzeros fill >= dense_threshold of its condensed column set (and use
 *    each such column twice on average) is stored densely over those
 *    columns (MFMA fragment order, chunks of 64 columns) and runs on fp32
 *    MFMA, each B row of a chunk staged once per block instead of gathered
 *    per nonzero; its rows' diagonal entries are kept aside and added in the
 *    epilogue; multi-chunk blocks are summed from partial slabs in order.
 *    dense_threshold > 1 disables the part (default callers pass 0.25).
 *
 *  - row units: the other rows.  A row of at most `ipc` nonzeros is one unit
 *    owned by one lane group (LPR lanes, each a 16-B column vector); a
 *    heavier row is cut into segments of about ipc * groups nonzeros (at most
 *    64), each owned by `groups` lane groups (the 64/LPR groups of a
 *    wavefront, or the 4 wavefronts of a workgroup when LPR = 64) that take
 *    interleaved nonzeros and meet in a fixed-order reduction; a row of
 *    several segments leaves one partial per segment and the last segment to
 *    finish (arrival counters in the caller's COUNTER REGION: int32
 *    gcnk_spmm_counter_bytes(header) bytes, zero on entry and left zero on
 *    return) sums them in segment order.
 * All sums have a fixed order (no float atomics): bitwise reproducible.
 * gcnk_spmm_groups(F, lanes_hint) gives the `groups` the kernels use for a
 * width F; a plan serves every F with that count.  The plan copies the
 * values: rebuild it when they change.  Building copies the CSR to the host
 * and synchronises `stream` (one-time setup).  The _host variants build the
 * same plan image from HOST arrays into host memory (no device needed).
 *
 * Plan header (16 int32, first words of the plan; gcnk_spmm_plan_query):
 *   0 magic 'GNK5'  1 M  2 K  3 groups (lane groups per wavefront, 64 / LPR)
 *   4 ipc  5 row units  6 heavy segments (heavy region, padded)
 *   7 heavy rows of > 1 segment  8 tile chunks  9 multi-chunk blocks  10 slabs
 *   11 tile blocks  12 diagonal kept aside | segp << 1 | tops << 30  13 nnz
 *   14 partial slots  15 chunk items of single-chunk tile blocks (listed first)
 * (segp: stride of the heavy segments' padded item copies, 0 = none; tops: some
 * row has more than 64 segments.  csrc/spmm_plan.h names the words.)
 * (Rounds 2-3 also built a hub-split plan and a split-K plan for R8's doc-topic
 * operands; both measured slower than this plan and were removed in ABI 8 --
 * DESIGN.md keeps their numbers.)
 * ------------------------------------------------------------------------- */
int32_t gcnk_spmm_groups(int32_t F, int32_t lanes_hint);
int32_t gcnk_spmm_default_ipc(int32_t M, int64_t nnz, int32_t F, int32_t lanes_hint);
/* Size of the plan buffer (synchronises `stream`; negative error code on failure). */
int64_t gcnk_spmm_plan_bytes(const int32_t* rowptr, const int32_t* colind, int32_t M, int32_t K,
                             int64_t nnz, int32_t ipc, int32_t groups, float dense_threshold, void* stream);
int gcnk_spmm_plan_build(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M,
                         int32_t K, int64_t nnz, int32_t ipc, int32_t groups, float dense_threshold,
                         void* plan, int64_t plan_bytes, void* stream);
/* The same from HOST arrays into a HOST buffer (plan-layout checks without a GPU). */
int64_t gcnk_spmm_plan_bytes_host(const int32_t* rowptr, const int32_t* colind, int32_t M, int32_t K,
                                  int64_t nnz, int32_t ipc, int32_t groups, float dense_threshold);
int gcnk_spmm_plan_build_host(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M,
                              int32_t K, int64_t nnz, int32_t ipc, int32_t groups, float dense_threshold,
                              int32_t* plan, int64_t plan_bytes);
/* Copies the 16-word plan header to host memory `out16` and synchronises
 * `stream` (one-time setup).  Every SpMM call takes this host header. */
int gcnk_spmm_plan_query(const void* plan, int32_t* out16, void* stream);
/* Bytes of workspace (split-row partials, tile slabs) an SpMM of width F needs. */
int64_t gcnk_spmm_workspace_bytes(const int32_t* plan_header, int32_t F);
/* Bytes of the counter region a call needs (0: none).  The region is zeroed
 * ONCE by the caller and then used by calls on one stream in order (never
 * concurrently by two calls): the kernels leave it zero for the next call. */
int64_t gcnk_spmm_counter_bytes(const int32_t* plan_header);

/* C = epi(A B) for the operand of `plan` (M x K from the header). */
int gcnk_spmm_csr_f32(const void* plan, const int32_t* plan_header,
                      const float* B, int64_t ldb, int32_t F,
                      float* C, int64_t ldc,
                      const float* bias, int32_t epilogue,
                      const uint8_t* drop_mask, int64_t ldm, float drop_scale,
                      float keep_prob, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                      float* workspace, int64_t workspace_bytes,
                      int32_t* counters, int64_t counter_bytes,
                      int32_t lanes_hint, void* stream);

/* The same product in two parts that write disjoint rows of C, for callers
 * that overlap them on two streams (join both before reading C):
 *   part 1: the single-chunk dense tile blocks (plan header word 15 items);
 *   part 2: everything else (multi-chunk tile blocks + their slab reduce,
 *           the row kernel);  part 0: all (= gcnk_spmm_csr_f32).
 * Part 2 alone uses the workspace.  (R8's X W1: part 1 = the document rows,
 * part 2 = the 50 dense topic rows, whose reduce launch then overlaps the
 * document blocks instead of following them.) */
int gcnk_spmm_csr_f32_part(const void* plan, const int32_t* plan_header,
                           const float* B, int64_t ldb, int32_t F,
                           float* C, int64_t ldc,
                           const float* bias, int32_t epilogue,
                           const uint8_t* drop_mask, int64_t ldm, float drop_scale,
                           float keep_prob, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                           float* workspace, int64_t workspace_bytes,
                           int32_t* counters, int64_t counter_bytes,
                           int32_t lanes_hint, int32_t part, void* stream);

/* SpMM with a fused dense projection of every finished row:
 *   H = epi(A B)  (stored to C only when C != NULL),   C2[M x P] = H * W[F x P]
 * i.e. layer.py:106,110,182,185 of gc1 followed by layer.py:102 of gc2
 * (support2 = H1 W2) while H1's row is still in registers: the gc2 GEMM
 * launch and, in inference, the H1 round trip through HBM disappear.
 * Supported for plans without dense tile blocks, float4-aligned operands,
 * F <= 256 and P <= 32; otherwise returns GCNK_EUNSUP (callers then run
 * gcnk_spmm_csr_f32 + gcnk_gemm_f32). */
int gcnk_spmm_proj_f32(const void* plan, const int32_t* plan_header,
                       const float* B, int64_t ldb, int32_t F,
                       float* C, int64_t ldc,
                       const float* bias, int32_t epilogue,
                       const uint8_t* drop_mask, int64_t ldm, float drop_scale,
                       float keep_prob, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                       const float* W, int64_t ldw, int32_t P, float* C2, int64_t ldc2,
                       float* workspace, int64_t workspace_bytes,
                       int32_t* counters, int64_t counter_bytes,
                       int32_t lanes_hint, void* stream);

/* Test aid (ABI 13): what gcnk_spmm_csr_f32 / _part / gcnk_spmm_proj_f32 launch
 * for a plan header and these arguments, decided by the one host function the
 * launch itself switches on (host only: nothing is launched, no device access,
 * no stream).  aligned16: bit mask of the base pointers that are 16-B aligned
 * (a null pointer counts as aligned); P = 0: no projection; part as in
 * gcnk_spmm_csr_f32_part.  Returns what the launch returns for the same
 * arguments where that depends on them alone (GCNK_EUNSUP for a refused
 * projection, GCNK_EARG for a plan built for another group count, ...).
 * out16 (all 0 where nothing is launched):
 *   0 the row kernel launches  1 LPR  2 VEC (4 / 1)  3 NP (0, or 8 / 32 with a
 *   projection)  4 column windows (launches of <= 64 column tiles)
 *   5, 6 O32 of the first / last window (32-bit gather byte offsets)
 *   7 spmm_heavy_top_kernel<VEC> follows
 *   8 the tile kernel launches  9 VEC4  10 NT  11 DIAG  12 column slices
 *   13 spmm_tile_reduce_kernel follows  14, 15 reserved (0) */
#define GCNK_SPMM_ALIGNED_B 1
#define GCNK_SPMM_ALIGNED_C 2
#define GCNK_SPMM_ALIGNED_BIAS 4
#define GCNK_SPMM_ALIGNED_WORKSPACE 8
#define GCNK_SPMM_ALIGNED_ALL 15
int gcnk_spmm_route(const int32_t* plan_header, int32_t F, int64_t ldb, int64_t ldc, int32_t aligned16,
                    int32_t lanes_hint, int32_t P, int32_t part, int32_t* out16);

/* ---------------------------------------------------------------------------
 * fp32 GEMM on MFMA (v_mfma_f32_16x16x4_f32; exact fp32 FMA chains):
 *   C[M x N] = epi( op(A)[M x K] * op(B)[K x N] )
 * op(A) = A (row-major [M x K], lda) or A^T (A stored [K x M], lda) when transA.
 * op(B) = B ([K x N], ldb) or B^T (B stored [N x K], ldb) when transB.
 * Replaces th.spmm(dense H, W) (layer.py:102 in gc2, which ATen lowers to mm)
 * and the dense autograd products H^T g, g W^T.
 * split_k > 1 reduces K in slabs (workspace = split_k*M*N floats) summed in a
 * fixed order by a second pass (bitwise reproducible).
 * ------------------------------------------------------------------------- */
int64_t gcnk_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t split_k);
int gcnk_gemm_f32(int32_t transA, int32_t transB, int32_t M, int32_t N, int32_t K,
                  const float* A, int64_t lda, const float* B, int64_t ldb,
                  float* C, int64_t ldc,
                  const float* bias, int32_t epilogue, const float* R, int64_t ldr, float scale,
                  int32_t split_k, float* workspace, int64_t workspace_bytes, void* stream);
/* Test aid (ABI 13): the kernel gcnk_gemm_f32 launches for these arguments,
 * decided by the one host function the launch itself switches on (nothing is
 * launched here).  a_aligned16 / b_aligned16: A's / B's base pointer is 16-B
 * aligned.  out4 = {family, p0, p1, flags}:
 *   family   GCNK_GEMM_ROUTE_*; p0, p1 its template parameters -- NARROW and
 *            SHORTK {KCH, NT}, SKINNY {KB, NT}, SMALLM {KBW, NTG} -- or, for the
 *            two TILED families, {transA, transB} as 0 / 1
 *   flags    GCNK_GEMM_ROUTE_SPLIT: K is reduced in more than one slab (a
 *            reduce kernel applies the epilogue); GCNK_GEMM_ROUTE_PTR_FETCH: an
 *            operand of a TILED family spans more than its 32-bit buffer
 *            offsets, so the kernel loads through 64-bit pointers.
 * M, N > 0 (gcnk_gemm_f32 launches nothing otherwise). */
#define GCNK_GEMM_ROUTE_NARROW 1     /* gemm_shortk_kernel<13|16, 2>: gc2's H1 W2 past 16k rows */
#define GCNK_GEMM_ROUTE_SKINNY 2     /* gemm_skinny_ksplit_kernel<KB, NT> */
#define GCNK_GEMM_ROUTE_SHORTK 3     /* gemm_shortk_kernel<1..8, 3> */
#define GCNK_GEMM_ROUTE_SMALLM 4     /* gemm_smallm_wk_kernel + gemm_slab_reduce4_buf_kernel (or gemm_slab_reduce4_kernel) */
#define GCNK_GEMM_ROUTE_TILED_N16 5  /* gemm_f32_mfma_kernel, 128 x 16 tile (N <= 16) */
#define GCNK_GEMM_ROUTE_TILED 6      /* gemm_f32_mfma_kernel, 64 x 64 tile */
#define GCNK_GEMM_ROUTE_SPLIT 1
#define GCNK_GEMM_ROUTE_PTR_FETCH 2
int gcnk_gemm_route(int32_t transA, int32_t transB, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb,
                    int32_t a_aligned16, int32_t b_aligned16, int32_t split_k, int32_t* out4);

/* ---------------------------------------------------------------------------
 * out[n] = sum_m X[m, n]  (bias gradient, autograd of layer.py:110).
 * Deterministic two-pass reduction; workspace = gcnk_colsum_workspace_bytes.
 * ------------------------------------------------------------------------- */
int64_t gcnk_colsum_workspace_bytes(int32_t M, int32_t N);
int gcnk_colsum_f32(const float* X, int64_t ldx, int32_t M, int32_t N, float* out,
                    float* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Fused backward of gc2 and of gc1's ReLU + dropout (autograd of
 * layer.py:182-188 through layer.py:102-110; replaces gcnk_gemm_f32 with
 * GCNK_GEMM_EPI_MASK_POS for gZ1, the split-K gcnk_gemm_f32 for gW2 and two
 * gcnk_colsum_f32 calls):
 *   gZ1[m, n] = H[m, n] > 0 ? scale * (gS[m, :] . W[n, :]) : 0     [M x N, ldz]
 *   gW[n, p]  = sum_m H[m, n] gS[m, p]                             [N x P, contiguous]
 *   gb1[n]    = sum_m gZ1[m, n]                                    [N]
 *   gb2[p]    = sum_m G[m, p]                 (G nullable)         [P]
 * H = gc1's output after ReLU + dropout [M x N], gS = A^T G [M x P], W = W2
 * [N x P].  gW / gb1 / gb2 are nullable (not stored).  P <= 32 (else
 * GCNK_EUNSUP).  Two launches; sums in a fixed order (bitwise reproducible).
 * Workspace: gcnk_gcn_bwd2_workspace_bytes(M, N, P) bytes at a 16-byte aligned
 * address (the kernel stores 16-B pieces into it; GCNK_EARG otherwise, before
 * any launch -- gcnk_gcn_backward_f32's bwd2_ws likewise).
 * ------------------------------------------------------------------------- */
int64_t gcnk_gcn_bwd2_workspace_bytes(int32_t M, int32_t N, int32_t P);
int gcnk_gcn_bwd2_f32(const float* H, int64_t ldh, const float* gS, int64_t ldgs, const float* W, int64_t ldw,
                      const float* G, int64_t ldg, int32_t M, int32_t N, int32_t P, float scale,
                      float* gZ1, int64_t ldz, float* gW, float* gb1, float* gb2,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* Test aid (within ABI 13, an addition only): what gcnk_gcn_bwd2_f32 launches
 * for these arguments and which run-time branches its kernel takes, from the
 * host function the launch itself is made from and the predicates the kernel
 * itself evaluates (nothing is launched here, no GPU is needed).
 * h_align / z_align: the largest of 16, 8, 4 bytes that H's / gZ1's base pointer
 * is aligned to; has_g: G is given (ldg is ignored otherwise); w_aligned16: W's
 * base pointer is 16-B aligned.  out9 =
 *   0 vec, 1 pm   the instantiation gcn_bwd2_kernel<vec, pm>: vec columns per
 *                 lane (4, 2, 1), pm = P padded to 8, 16 or 32
 *   2 slices      256-column slices (grid y)      3 nblk  workgroups per slice (grid x)
 *   4 rpb         rows per workgroup              5 part_ld  floats per workspace row
 *   6 gS / G rows staged by LDS-DMA (else by scalar loads, zero-padded to pm);
 *     for column slice 0 -- the later slices stage gS alone, whatever ldg is
 *   7 W's rows loaded as 16-B row runs (else guarded 4-B loads)
 *   8 the row lanes' partials summed as float4 pieces (else per float)
 * 1 <= P <= 32, M, N >= 1, leading dimensions as gcnk_gcn_bwd2_f32 takes them
 * (GCNK_EARG otherwise). */
int gcnk_gcn_bwd2_route(int32_t M, int32_t N, int32_t P, int64_t ldh, int64_t ldz, int32_t h_align,
                        int32_t z_align, int64_t ldgs, int32_t has_g, int64_t ldg, int64_t ldw,
                        int32_t w_aligned16, int64_t* out9);

/* ---------------------------------------------------------------------------
 * Hub-factored gc1 (csrc/factor.hip; GCN.forward layer.py:164-190 through
 * layer.py:102,106,110,182,185 and gc2's support layer.py:102) for a graph
 * whose rows split into hub rows and light rows referencing only hub columns
 * and themselves, with X's light rows inside the column range [k0, k0 + Kc):
 *   Z[r, :]   = U[i, :Kc] . W[k0 .. k0+Kc-1, :] + sum_{items of r} val * S[hub, :]
 *   H[r, n]   = epilogue(Z[r, n] + bias[n])            (GCNK_EPI_*, as the SpMM)
 *   C2[r, p]  = sum_n H[r, n] W2[n, p]                 (P <= 32)
 * for r = the row id at position i of the block order.  U [M x Kc] in block
 * order (ldu >= Kc rounded up to 4, zero past Kc), S = X[hubs] W [nhub x F]
 * (lds), rec = one record of rec_words int32 per 32-row block: 33 offsets
 * (block-relative item index), 3 pad words, 32 row ids (the output rows of the
 * block's positions, -1 past M), then items int2 {hub index, value bits}.  H
 * nullable (not stored).  F % 4 == 0, F <= 256, Kc <= 128; GCNK_EUNSUP when
 * the block's operands exceed 160 KiB of LDS (gcnk_hubfactor_lds_bytes).  One
 * launch, fixed-order sums.
 * ------------------------------------------------------------------------- */
int64_t gcnk_hubfactor_lds_bytes(int32_t F, int32_t Kc, int32_t nhub, int32_t rec_words, int32_t P);
/* Test aid: fills every CU's 160 KiB of LDS with `word` (one launch), so a
 * following launch that read LDS it had not written would see it. */
int gcnk_debug_poison_lds(uint32_t word, void* stream);
int gcnk_hubfactor_gc1_f32(int32_t M, int32_t F, int32_t Kc, int32_t nhub, int32_t P, const float* U, int64_t ldu,
                           const float* W, int64_t ldw, int32_t k0, const float* S, int64_t lds,
                           const int32_t* rec, int32_t rec_words, const float* bias, int32_t epilogue,
                           const uint8_t* drop_mask, int64_t ldm, float drop_scale, float keep_prob, uint64_t seed,
                           uint64_t offset, const uint64_t* rng_base, const float* W2, int64_t ldw2, float* H,
                           int64_t ldh, float* C2, int64_t ldc2, void* stream);
/* Test aid (within ABI 13, an addition only): what gcnk_hubfactor_gc1_f32
 * launches for these arguments, from the host function the launch itself is
 * made from (nothing is launched here, no GPU is needed).  u_aligned16: U's
 * base pointer is 16-B aligned.  out6 =
 *   0 KS, 1 NTQ, 2 NP   the instantiation hubfactor_gc1_kernel<KS, NTQ, NP>:
 *                       k-steps of U W[Kc] (13, 18, 25, 32), 16-column tiles
 *                       of F per wave (2, 3, 4), n-tiles of P (1, 2)
 *   3 u_lds             U's rows staged in LDS by 16-B DMA (else loaded directly)
 *   4 dynamic LDS bytes of the launch      5 workgroups per 32 rows (1)
 * GCNK_EARG / GCNK_EUNSUP where gcnk_hubfactor_gc1_f32 returns them for these
 * arguments (sizes, ldu < Kc, rec_words; F % 4, F > 256, Kc > 128, P > 32,
 * more than 160 KiB of LDS). */
int gcnk_hubfactor_gc1_route(int32_t F, int32_t Kc, int32_t nhub, int32_t rec_words, int32_t P, int64_t ldu,
                             int32_t u_aligned16, int64_t* out6);
/* ---------------------------------------------------------------------------
 * gc2's aggregation from the hub factor (csrc/factor_gc2.hip; layer.py:106,110
 * of gc2):  out[r, :P] = sum over row r's items of A-hat, in CSR column order,
 * of val * S2[col, :P]  + b2  -- for the same (A-hat, X) structure as above.
 * One launch: a workgroup per hub row (its full CSR row: hub_rp[H + 1], hub_ci,
 * hub_val in hub order, hub_ids[H] the rows they are) and a workgroup per
 * 32-row block record of gcnk_hubfactor_gc1_f32 (`rec`: a light row's hub-column
 * items), with diag / pre of gcnk_factor_diag_f32 placing the row's diagonal
 * among them; positions with pre < 0 or row id < 0 are skipped.  hub_ids and
 * hub_rp are HOST arrays: they travel in the kernel's arguments.  b2 nullable.
 * A light row is one fma chain from +0 in column order, then + b2: bitwise the
 * SpMM's result for a row of one unit; a hub row is summed by 256 / (P / 4) lane
 * groups that meet in a fixed order.  No workspace, no counters, no atomics.
 * P % 4 == 0, P <= 32, H <= 128, lds2 % 4 == ldo % 4 == 0, S2 / out / rec / b2
 * 16-B aligned, operands below 2 GiB, record + S2[hubs] within 64 KiB of LDS:
 * otherwise GCNK_EUNSUP before any launch (callers run gcnk_spmm_csr_f32).
 * ------------------------------------------------------------------------- */
int gcnk_hubfactor_gc2_f32(int32_t M, int32_t H, int32_t P, const int32_t* rec, int32_t rec_words,
                           const float* diag, const int32_t* pre, const int32_t* hub_ids /* host */,
                           const int32_t* hub_rp /* host */, const int32_t* hub_ci, const float* hub_val,
                           const float* S2, int64_t lds2, const float* b2, float* out, int64_t ldo, void* stream);
/* ---------------------------------------------------------------------------
 * Held-graph scoring (csrc/score_docs.hip; within ABI 13, an addition only):
 * the logits of B documents that are not in the training graph, each as the
 * row it would have in the transductive forward (GCN.forward layer.py:164-190)
 * with the hub nodes' state held as the training graph left it -- for the
 * (A-hat, X) structure above: a document row of A-hat holds its diagonal and
 * hub columns only, a document row of X the columns k0 .. k0 + Kc.
 *   x [B x Kc] (ldx)   the document's feature values on columns k0 .. k0 + Kc
 *   a [B x H] (lda)    its raw edge weight to each hub (0: no edge).  Negative
 *                      or non-finite weights are the caller's error: they are
 *                      NOT checked on the device.
 *   W1 (ldw1)          gc1's weight; rows k0 .. k0 + Kc - 1 are read
 *   S_T [H x F] (lds)  X[hubs] W1 of the training graph
 *   W2 [F x P] (ldw2), S2_T [H x P] (lds2) = (H1 W2)[hubs] of its eval forward
 *   dh [H] float64     the hubs' D^-1/2 (sqrt of A-hat's hub diagonal), device
 *   b1 [F], b2 [P]     nullable
 * Per document d (coefficients: A-hat's recipe, float64 rounded to fp32 once):
 *   deg    = 1 + sum_j a[d, j]                 (float64, j ascending)
 *   dd     = deg^-1/2,  c_self = fp32(dd dd),  c_j = fp32((dd a[d, j]) dh[j])
 *   z[n]   = c_self sum_k x[d, k] W1[k0 + k, n] + sum_j c_j S_T[j, n] + b1[n]
 *   h[n]   = max(z[n], 0)                      (a NaN stays a NaN)
 *   out[d, p] = c_self sum_n h[n] W2[n, p] + sum_j c_j S2_T[j, p] + b2[p]
 *   labels[d] = first index of the maximum of out[d, :], a NaN maximal
 *               (gcnk_class_stats' rule); labels nullable (int32 [B]).
 * One launch on `stream`, fp32 MFMA with fixed-order sums, no atomics, no
 * workspace: bitwise reproducible and capturable.  B = 0 returns GCNK_OK
 * without touching the device.  GCNK_EARG: bad sizes, a null operand, a leading
 * dimension shorter than its row.  GCNK_EUNSUP outside gcnk_hubfactor_gc1_f32's
 * range -- F % 4 == 0, F <= 256, Kc <= 128, H <= 128, P <= 32 -- or where the
 * rows of x, a, W1 or S_T are not 16-B aligned (base and leading dimension).
 * ------------------------------------------------------------------------- */
int gcnk_score_docs_f32(int32_t B, int32_t F, int32_t Kc, int32_t H, int32_t P, int32_t k0, const float* x,
                        int64_t ldx, const float* a, int64_t lda, const float* W1, int64_t ldw1, const float* S_T,
                        int64_t lds, const float* W2, int64_t ldw2, const float* S2_T, int64_t lds2,
                        const double* dh, const float* b1, const float* b2, float* out, int64_t ldo,
                        int32_t* labels, void* stream);
/* Test aid (an addition only): what gcnk_score_docs_f32 launches for a shape, from
 * the host function the launch itself is made from (nothing is launched, no GPU
 * is needed).  out8 =
 *   0 NTQ, 1 NP, 2 KHQ   the instantiation score_docs_kernel<NTQ, NP, KHQ>: 16-column
 *                        tiles of F per wave (2, 3, 4), n-tiles of P (1, 2), k-steps
 *                        of the hub sum per quarter (4, 8)
 *   3 rows of [W1[k0:k0+Kc]; S_T] staged in LDS at a time (a multiple of 4)
 *   4 operand row stride in LDS (floats, = 4 mod 64)
 *   5 operand row columns the kernel writes: [c_self x | c | 0]; the MFMA k-loop
 *     reads columns 0 .. roundup4(Kc + H) - 1, the hub sum Kc .. Kc + 16 KHQ - 1
 *   6 dynamic LDS bytes of the launch      7 workgroups per 32 documents (1)
 * GCNK_EARG / GCNK_EUNSUP where gcnk_score_docs_f32 returns them for these sizes. */
int gcnk_score_docs_route(int32_t F, int32_t Kc, int32_t H, int32_t P, int64_t* out8);
/* ---------------------------------------------------------------------------
 * Narrow-feature gc1 (csrc/dense_gc1.hip; GCN.forward layer.py:164-190 through
 * layer.py:102,106,110,182,185 and gc2's support layer.py:102) for a dense X
 * with at most 128 features (the gensim-shaped topic features, README.md:77,95):
 * with AX = A-hat X [M x K] (ldax >= K, gcnk_aggregate_f32, built once per
 * (A-hat, X) pair),
 *   H[r, n]  = epilogue((AX W1)[r, n] + bias[n])   (GCNK_EPI_BIAS_RELU[_DROP|_HASH])
 *   C2[r, p] = sum_n H[r, n] W2[n, p]
 * in one launch (fp32 MFMA, fixed-order sums).  H nullable (not stored).
 * K <= 128, F <= 256, P <= 32 (GCNK_EUNSUP otherwise).  The association
 * (A-hat X) W1 differs from the reference's A-hat (X W1) in fp32 rounding only.
 *   gcnk_aggregate_f32: out[r, c] = fp32( sum over row r's items in CSR order,
 *   in float64, of val * X[col, c] ), c < K; 0 for K <= c < Kp <= 128.
 * ------------------------------------------------------------------------- */
int gcnk_dense_gc1_f32(int32_t M, int32_t K, int32_t F, int32_t P, const float* AX, int64_t ldax, const float* W1,
                       int64_t ldw1, const float* bias, int32_t epilogue, const uint8_t* drop_mask, int64_t ldm,
                       float drop_scale, float keep_prob, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                       const float* W2, int64_t ldw2, float* H, int64_t ldh, float* C2, int64_t ldc2, void* stream);
/* Test aid (within ABI 13, an addition only): what gcnk_dense_gc1_f32 launches
 * for these sizes, from the host function the launch itself is made from
 * (nothing is launched here, no GPU is needed).  out6 =
 *   0 KS, 1 NI, 2 NPM, 3 PV   the instantiation dense_gc1_kernel<KS, NI, NPM, PV>:
 *                       k-steps of AX W1 (8, 13, 16, 25, 32), 16-column n-tiles
 *                       of F per wave (3, 4), MFMA tiles of P (1, 2), columns of
 *                       P past them on the VALU (0, 4)
 *   4 tail              1 when NI = 3 and F > 192: the rotating tail n-tile runs
 *   5 ntiles            16-row tiles, ceil(M / 16); the launch's grid is
 *                       min(ntiles, two workgroups per CU)
 * GCNK_EARG / GCNK_EUNSUP where gcnk_dense_gc1_f32 returns them for these
 * sizes (a size <= 0; K > 128, F > 256, F % 4, P > 32). */
int gcnk_dense_gc1_route(int32_t M, int32_t K, int32_t F, int32_t P, int64_t* out6);
int gcnk_aggregate_f32(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M, const float* X,
                       int64_t ldx, int32_t K, float* out, int64_t ldo, int32_t Kp, void* stream);

/* The hub factorisation's (A-hat, X)-fixed operands, built on the device once
 * per operand pair (csrc/factor_build.hip; factor.py drives it, the host
 * restatement is oracle/factor_host.py):
 *   gcnk_factor_u_f32:   U[p, c] = fp32( sum over the items (r, d) of row
 *                        r = perm[p], d light (hub_index[d] < 0), in CSR order,
 *                        in float64, of val * Xl[d, c] ), c < Kc; 0 for
 *                        Kc <= c < Kcp <= 128.  Xl [M x >= Kc] (ldxl): X's
 *                        columns k0.. (hub rows never read).
 *   gcnk_factor_records: the per-32-row-block A_H records gcnk_hubfactor_gc1_f32
 *                        reads, into rec [ceil(M/32) x rec_words] (zeroed by
 *                        the call first); *overflow (zeroed by the call)
 *                        counts blocks whose items did not fit.
 *   gcnk_factor_analyze: the structure test in front of them, on the device
 *                        with one host sync (ABI 12; replaces torch element-wise
 *                        / nonzero / index kernels whose first-use loads cost
 *                        the first forward ~120 ms): hub rows = rows of >= hmin
 *                        nonzeros; host outputs info[8] = {H, bad (a light row
 *                        with a column that is neither a hub nor its diagonal),
 *                        k0, k1 (column range of X's nonzero entries in light
 *                        rows, k1 = -1 if none), total length of X's hub rows
 *                        (CSR X), 0, 0, 0}, hubs[max_hubs] (the first H found,
 *                        unordered; H > max_hubs: some missing), cnt[M] (each
 *                        row's hub-column items).  X: CSR (x_rowptr non-NULL, M
 *                        rows) or dense [M x K] (x_dense, ldx).  Workspace:
 *                        gcnk_factor_analyze_workspace_bytes(M, max_hubs).
 *   gcnk_factor_xl_f32:  Xl [M x Kcp] (ldxl) = X[r, k0 .. k0 + Kc) for light
 *                        rows (hub_index[r] < 0) of a CSR X, zero elsewhere.
 *   gcnk_csr_gather_rows / gcnk_dense_gather_rows_f32: the rows `rows[0 ..
 *                        nrows)` of a CSR (out_rowptr[nrows + 1] written; out
 *                        arrays sized by the caller) or of a dense matrix (out
 *                        [nrows x ldo], columns K .. ldo - 1 zero): X's hub rows. */
int gcnk_factor_u_f32(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M,
                      const int32_t* hub_index, const int32_t* perm, const float* Xl, int64_t ldxl, int32_t Kc,
                      float* U, int64_t ldu, int32_t Kcp, void* stream);
/*   gcnk_factor_diag_f32: for each position p of the block order (32 * ceil(M / 32)
 *                        of them), diag[p] = A-hat_rr of r = perm[p] (0 for a
 *                        missing diagonal, a hub row, p >= M) and pre[p] = how
 *                        many of the row's hub-column items have a column below
 *                        r (-1 for a hub row, 0 for p >= M): where the diagonal
 *                        sits among the record's items in CSR column order.
 *                        Fixed by A-hat alone (gcnk_hubfactor_gc2_f32 reads them). */
int gcnk_factor_diag_f32(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M,
                         const int32_t* hub_index, const int32_t* perm, float* diag, int32_t* pre, void* stream);
int gcnk_factor_records(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M,
                        const int32_t* hub_index, const int32_t* perm, int32_t* rec, int32_t rec_words,
                        int32_t* overflow, void* stream);
int64_t gcnk_factor_analyze_workspace_bytes(int32_t M, int32_t max_hubs);
int gcnk_factor_analyze(const int32_t* rowptr, const int32_t* colind, int32_t M, int32_t hmin,
                        const int32_t* x_rowptr, const int32_t* x_colind, const float* x_val,
                        const float* x_dense, int64_t ldx, int32_t K, int32_t max_hubs, int32_t* info /* host */,
                        int32_t* hubs /* host */, int32_t* cnt /* host */, void* workspace, int64_t workspace_bytes,
                        void* stream);
int gcnk_factor_xl_f32(const int32_t* x_rowptr, const int32_t* x_colind, const float* x_val, int32_t M,
                       const int32_t* hub_index, int32_t k0, int32_t Kc, float* Xl, int64_t ldxl, int32_t Kcp,
                       void* stream);
int gcnk_csr_gather_rows(const int32_t* rowptr, const int32_t* colind, const float* val, const int32_t* rows,
                         int32_t nrows, int32_t* out_rowptr, int32_t* out_colind, float* out_val, void* stream);
int gcnk_dense_gather_rows_f32(const float* X, int64_t ldx, int32_t K, const int32_t* rows, int32_t nrows,
                               float* out, int64_t ldo, void* stream);

/* ---------------------------------------------------------------------------
 * Whole-forward launch record (ABI 8): GCN.forward (layer.py:164-190) as the
 * reference's trainer issues it, eagerly, every epoch (trainer.py:357 train,
 * trainer.py:382 eval) -- from ONE call.  The caller fills the record once per
 * (adjacency, features, widths, stream) with everything that does not change
 * from call to call: the plans and their host headers, workspaces and counter
 * regions, the factored operands, the intermediates S1 and S2.  Each call
 * passes only the parameters, the outputs and the dropout arguments, and
 * issues the launches the per-op entry points above issue, in the same order
 * and with the same arguments (results are bitwise those of the per-op path).
 *
 *   GCNK_FWD_FACTORED   S_T = X_hubs W1 (x plan or dense GEMM, x_rows = nhub);
 *                       (H1, S2) = gcnk_hubfactor_gc1_f32; out = A-hat S2 + b2
 *   GCNK_FWD_SPMM_PROJ  S1 = X W1; (H1, S2) = gcnk_spmm_proj_f32(aF); out = A-hat S2 + b2
 *   GCNK_FWD_SPMM_GEMM  S1 = X W1; H1 = epi(A-hat S1 + b1) (aF); S2 = H1 W2; out = A-hat S2 + b2
 *   GCNK_FWD_DENSE_AX   (H1, S2) = gcnk_dense_gc1_f32(U = A-hat X [M x Kc], ldu); out = A-hat S2 + b2
 *                       (no first product: x, s1 unused)
 *
 * gc2's aggregation uses the plan aP with GCNK_EPI_BIAS (GCNK_EPI_NONE when b2
 * is NULL).  W1 [x_cols x F] and W2 [F x P] contiguous; H1 (ldh) is stored
 * when non-NULL (a backward needs it); SPMM_GEMM needs h1_tmp [M x F] when it
 * is NULL.  The record's buffers are used in stream order: calls that may
 * run concurrently need records of their own.
 * ------------------------------------------------------------------------- */
typedef struct gcnk_plan_ref {
  const void* plan;            /* device plan image (gcnk_spmm_plan_build) */
  int32_t hdr[16];             /* its header (gcnk_spmm_plan_query) */
  float* workspace;            /* gcnk_spmm_workspace_bytes(hdr, width) bytes */
  int64_t workspace_bytes;
  int32_t* counters;           /* gcnk_spmm_counter_bytes(hdr) bytes (zeroed once) */
  int64_t counter_bytes;
  int32_t lanes_hint;
  int32_t pad_;
} gcnk_plan_ref;

#define GCNK_FWD_FACTORED 1
#define GCNK_FWD_SPMM_PROJ 2
#define GCNK_FWD_SPMM_GEMM 3
#define GCNK_FWD_DENSE_AX 4

typedef struct gcnk_gcn_fwd {
  int32_t kind;
  int32_t M, F, P;             /* rows of A-hat, nhid, nclass */
  int32_t x_rows, x_cols;      /* first product's operand (factored: the hub rows of X) */
  gcnk_plan_ref x;             /* sparse operand: its plan (x.plan != NULL) ...       */
  const float* x_dense;        /* ... or dense [x_rows x x_cols] (ldx) on the MFMA GEMM */
  int64_t ldx;
  int32_t x_split_k;
  int32_t pad0_;
  float* gemm_ws;              /* GEMM split-K workspace (first product and H1 W2) */
  int64_t gemm_ws_bytes;
  float* s1;                   /* S1 = X W1, or S_T = X_hubs W1 [x_rows x F] */
  int64_t lds1;
  int32_t Kc, nhub, k0, rec_words;   /* factored gc1 (gcnk_hubfactor_gc1_f32); DENSE_AX: Kc = K */
  const float* U;
  int64_t ldu;
  const int32_t* rec;
  gcnk_plan_ref aF;            /* A-hat at width F (SPMM kinds) */
  gcnk_plan_ref aP;            /* A-hat at width P (gc2) */
  float* s2;                   /* S2 = H1 W2 [M x P] */
  int64_t lds2;
  float* h1_tmp;               /* SPMM_GEMM scratch H1 when H1 == NULL */
  int64_t ld_h1_tmp;
  /* FACTORED: gc2's aggregation through gcnk_hubfactor_gc2_f32 when gc2_diag != NULL
   * (aP's SpMM where that entry answers GCNK_EUNSUP).  Added at the end of the
   * struct within ABI 13: a zero-filled tail means "the SpMM", as before. */
  const float* gc2_diag;
  const int32_t* gc2_pre;
  const int32_t* gc2_hub_ids;  /* host */
  const int32_t* gc2_hub_rp;   /* host */
  const int32_t* gc2_hub_ci;
  const float* gc2_hub_val;
} gcnk_gcn_fwd;

int gcnk_gcn_forward_f32(const gcnk_gcn_fwd* rec,
                         const float* W1, const float* b1, const float* W2, const float* b2,
                         float* out, int64_t ldo, float* H1, int64_t ldh,
                         int32_t epilogue, const uint8_t* drop_mask, int64_t ldm, float drop_scale,
                         float keep_prob, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                         void* stream);
/* The backward of the same forward (trainer.py:361 loss.backward()), from
 * one call, with gcnk_gcn_bwd filled once per (adjacency, features, widths,
 * stream) -- the launches ops.GCNFn.backward issues, in its order:
 *   gS2 = A-hat^T G                          (aTP: A-hat^T's plan at width P)
 *   gZ1, gW2, gb1, gb2 = gcnk_gcn_bwd2_f32(H1, gS2, W2, G)  (bwd2 workspace)
 *   gS1 = A-hat^T gZ1; gW1 = X^T gS1         (aTF; X^T's plan xT, or the MFMA
 *                                             GEMM on dense X with x_split_k)
 * G = dlogits [M x P] (contiguous), H1 [M x F] (ldh), W2 [F x P].  gW1, gb1,
 * gW2, gb2 are nullable (not computed); gb2 needs G's column sums only.
 * flags & GCNK_BWD_AX_DIRECT: x_dense holds A-hat X (the DENSE_AX forward) and
 * gW1 = (A-hat X)^T gZ1 directly (no gS1, no aTF plan).
 * (ABI 11's GCNK_BWD_FACTORED -- gW1 through the hub factor -- measured slower
 * than A-hat^T gZ1 + X^T gS1 in the step and was removed in ABI 12.) */
#define GCNK_BWD_AX_DIRECT 1
typedef struct gcnk_gcn_bwd {
  int32_t M, F, P;             /* rows of A-hat, nhid, nclass */
  int32_t x_rows, x_cols;      /* X [x_rows x x_cols]: gW1 is [x_cols x F] */
  int32_t x_split_k;           /* dense X: K-slabs of X^T gS1 */
  int32_t flags;               /* GCNK_BWD_* */
  int32_t pad1_;
  gcnk_plan_ref aTP, aTF;      /* A-hat^T at widths P and F */
  gcnk_plan_ref xT;            /* sparse X: X^T's plan at width F (xT.plan != NULL) ... */
  const float* x_dense;        /* ... or dense X (ldx) */
  int64_t ldx;
  float* gemm_ws;              /* split-K workspace of X^T gS1 */
  int64_t gemm_ws_bytes;
  float* gS2;                  /* scratch [M x P] */
  float* gZ1;                  /* scratch [M x F] */
  float* gS1;                  /* scratch [M x F] */
  void* bwd2_ws;               /* gcnk_gcn_bwd2_workspace_bytes(M, F, P) */
  int64_t bwd2_ws_bytes;
} gcnk_gcn_bwd;

int gcnk_gcn_backward_f32(const gcnk_gcn_bwd* rec, const float* G, const float* H1, int64_t ldh, const float* W2,
                          float scale, float* gW1, float* gb1, float* gW2, float* gb2, void* stream);

/* Layout of the record structs for bindings that mirror them: writes up to n
 * of {sizeof plan_ref, sizeof gcn_fwd, offsetof x, U, aF, aP, ld_h1_tmp,
 * plan_ref.lanes_hint, sizeof gcn_bwd, gcn_bwd.xT, gcn_bwd.bwd2_ws_bytes,
 * gcn_fwd.gc2_diag} to out and returns how many exist. */
int32_t gcnk_gcn_fwd_layout(int64_t* out, int32_t n);

/* ---------------------------------------------------------------------------
 * Sparse-format helpers (one-time graph preparation, utils.py:185-213,
 * trainer.py:226-238).
 *   gcnk_csr_transpose: CSR A[M x K] -> CSR A^T[K x M]; within each output
 *     row entries keep ascending source-row order (stable).  Needs a
 *     workspace of gcnk_csr_transpose_workspace_bytes.
 * ------------------------------------------------------------------------- */
int64_t gcnk_csr_transpose_workspace_bytes(int32_t M, int32_t K, int64_t nnz);
/*  gcnk_coo_to_csr: the torch sparse COO tensors the reference hands th.spmm
 *    (utils.py:196-203: A-hat column-major and uncoalesced; trainer.py:226-238:
 *    X row-major) -> int32 CSR with sorted columns, duplicates summed in input
 *    order (what ATen's coalesce computes).  rows/cols int64[nnz], vals fp32;
 *    outputs have capacity nnz; rowptr[M] is the output nnz (read it after the
 *    stream completes; -1 if an index was out of range).  Replaces ATen's
 *    coalesce + bincount on the one-time conversion path. */
int64_t gcnk_coo_to_csr_workspace_bytes(int64_t nnz, int32_t M, int32_t K);
int gcnk_coo_to_csr(const int64_t* rows, const int64_t* cols, const float* vals, int64_t nnz, int32_t M, int32_t K,
                    int32_t* rowptr, int32_t* colind, float* val, void* workspace, int64_t workspace_bytes,
                    void* stream);
int gcnk_csr_transpose(const int32_t* rowptr, const int32_t* colind, const float* val,
                       int32_t M, int32_t K, int64_t nnz,
                       int32_t* rowptr_t, int32_t* colind_t, float* val_t,
                       void* workspace, int64_t workspace_bytes, void* stream);
/*  gcnk_csr_to_dense: CSR A[M x K] -> dense row-major out[M x ld] (columns
 *    K..ld-1 untouched; duplicate entries summed in CSR order).  The one-time
 *    layout change that sends a dense-enough sparse infeatn (layer.py:102;
 *    e.g. a gensim-style 100-d X at 50-70 % fill) to the MFMA GEMM. */
int gcnk_csr_to_dense(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M, int32_t K,
                      float* out, int64_t ld, void* stream);

/* ---------------------------------------------------------------------------
 * Device-side adjacency preparation (utils.py:185-213, preprocess_adj /
 * normalize_adj, which the reference runs on the host with scipy):
 *   A_hat = D^-1/2 (A + I) D^-1/2,  D = rowsum(A + I)
 * with the reference's arithmetic (A + I and D in float64, d = rowsum^-0.5,
 * inf -> 0, value = (d[r] * a) * d[c] rounded once to fp32), so the values are
 * bit-for-bit the reference's.  Input: n x n CSR with sorted, duplicate-free
 * columns per row (a symmetric A, as trainer.py:148 makes it).  Output CSR
 * arrays have capacity nnz + n; rowptr_out[n] is the output nnz (read it
 * after the stream completes).  Workspace: gcnk_sym_normalize_workspace_bytes.
 * ------------------------------------------------------------------------- */
int64_t gcnk_sym_normalize_workspace_bytes(int32_t n, int64_t nnz);
int gcnk_sym_normalize(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t n, int64_t nnz,
                       int32_t* rowptr_out, int32_t* colind_out, float* val_out,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Evaluation counts in one launch (utils.py:25-109 accuracy / macro_f1 issue
 * 3 * nclass + 1 .item() syncs): for the n scored rows (row = idx[i], or i
 * when idx is NULL) of logits [rows x nclass] (leading dimension ld) with
 * int64 labels `target` (indexed by row), predicted class = first maximal
 * logit (NaN counts as maximal: th.max semantics); counts[3 * nclass + 1]
 * (zeroed by the call) = TP[nclass] | FP[nclass] | FN[nclass] | correct.
 * nclass <= 1024.  Integer atomics: exact.
 * ------------------------------------------------------------------------- */
int gcnk_class_stats(const float* logits, int64_t ld, const int64_t* target, const int64_t* idx, int64_t n,
                     int32_t nclass, int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------
 * Mean cross-entropy over a node set (csrc/loss.hip; additions within ABI 13):
 *   trainer.py:307      criterion = nn.CrossEntropyLoss()
 *   trainer.py:358-361  loss = criterion(logits[train_lst], target[train_lst]); loss.backward()
 *   trainer.py:383-384  the validation loss (forward only, lse = NULL)
 * without materialising logits[idx] and without the sort + scatter ATen's
 * indexing backward runs: the index set is turned once into row multiplicities,
 * and both passes are dense over the M rows of logits [M x P] (ld).
 *
 *   gcnk_ce_row_counts: counts[r] (zeroed by the call) = how often row r occurs
 *     in idx[0 .. n), r < M; counts[M] = entries outside [0, M), which are
 *     skipped, never dereferenced.  Integer atomics: exact.
 *   gcnk_ce_forward_f32: for every row r with counts[r] > 0 (every row, once,
 *     when counts is NULL; n is then M)
 *         lse_r = max_j z_rj + log sum_j exp(z_rj - max_j z_rj)        (fp32)
 *         l_r   = lse_r - z[r, target[r]]                              (float64)
 *         *loss = fp32( (sum_r counts[r] * l_r) / n )
 *     the sum in float64 in a fixed order (a fixed tree over a workgroup's rows,
 *     the workgroups' partials in index order): bitwise reproducible, no float
 *     atomics.  lse[r] is stored for the scored rows when lse != NULL (a
 *     backward needs it); target[r] is read for scored rows only.  A scored row whose target is outside [0, P) makes the
 *     loss NaN; nothing outside the row is read.  1 <= P <= 1024 (GCNK_EARG
 *     otherwise); workspace: gcnk_ce_workspace_bytes(M, P) bytes, 8-B aligned.
 *     Two launches.  M == 0: nothing is launched or written.
 *   gcnk_ce_backward_f32: the whole dense dlogits [M x P] (ldd) in one launch:
 *         counts[r] == 0:  +0.0
 *         otherwise:       g * fp32(counts[r] / n) * (exp(z_rj - lse_r) - [j == target[r]])
 *     g = *grad_out (a device scalar; 1 when NULL).  Columns P .. ldd - 1 are
 *     never written.  No zero-fill launch, no host sync.
 * ------------------------------------------------------------------------- */
int gcnk_ce_row_counts(const int64_t* idx, int64_t n, int32_t M, int32_t* counts, void* stream);
int64_t gcnk_ce_workspace_bytes(int32_t M, int32_t P);
int gcnk_ce_forward_f32(const float* logits, int64_t ld, int32_t M, int32_t P, const int64_t* target,
                        const int32_t* counts, int64_t n, float* loss, float* lse, void* workspace,
                        int64_t workspace_bytes, void* stream);
int gcnk_ce_backward_f32(const float* logits, int64_t ld, int32_t M, int32_t P, const int64_t* target,
                         const int32_t* counts, int64_t n, const float* lse, const float* grad_out,
                         float* dlogits, int64_t ldd, void* stream);

/* ---------------------------------------------------------------------------
 * Adam step (csrc/adam.hip; an addition within ABI 13): trainer.py:308
 * optimizer = th.optim.Adam(...), trainer.py:362 optimizer.step() -- torch's
 * Adam with amsgrad = False, maximize = False -- for up to
 * GCNK_ADAM_MAX_TENSORS contiguous fp32 tensors {p, g, m, v, numel} in ONE
 * launch (the table travels in the kernel's arguments; more tensors take
 * further calls).  With t = state[0] + 1, per element, in fp32 unless said:
 *     g' = fma(wd, p, g)                                  wd   = fp32(weight_decay)
 *     m' = fma(omb1, g' - m, m)                           omb1 = fp32(1 - beta1)
 *     v' = fma(b2, v, (omb2 * g') * g')                   b2   = fp32(beta2), omb2 = fp32(1 - beta2)
 *     p' = p - (step * m') / (sqrt(v') / sbc2 + eps)      step = fp32(lr / (1 - beta1^t))
 *                                                         sbc2 = fp32(sqrt(1 - beta2^t))
 * i.e. m' = beta1 m + (1 - beta1) g', v' = beta2 v + (1 - beta2) g'^2 and
 * p' = p - lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps), with
 * the operations in the order torch's step takes them (lerp_, mul_ + addcmul_,
 * sqrt / div / add_, addcdiv_).  1 - beta, beta^t (pow), step and sbc2 are
 * formed in float64 and rounded once (the last two on the device from the step
 * word, once per workgroup); sqrt and the divisions are correctly rounded.
 * The step word: state[0] is the number of steps taken, on the DEVICE, so a
 * step captured in a hipGraph advances on every replay.  Every workgroup reads
 * it at entry; it is advanced by the last workgroup to arrive at the counter
 * state[1] (zero on entry, left zero on return), after all have read it: THE
 * ARRIVAL HAND-OFF, explained once at arrive_last in csrc/gcnk_common.h.
 * state: int32[2], used by one call at a time.
 * flags:
 *   GCNK_ADAM_ZERO_GRAD  also store +0.0 to g after reading it (trainer.py:359
 *                        optimizer.zero_grad(): a captured step needs no fills)
 *   GCNK_ADAM_HOLD_STEP  read the step word, do not advance it: for every call
 *                        of one optimiser step over more than 8 tensors but the last
 * GCNK_EARG (on the host, before any launch) for a NULL table, buffer or state,
 * numel < 0, ntensors outside [0, 8], beta outside [0, 1), lr, eps or
 * weight_decay < 0.  ntensors == 0 succeeds and does nothing.
 * Work is cut into chunks of GCNK_ADAM_CHUNK elements, one workgroup each (THE
 * CHUNK TABLE, csrc/tensor_chunks.h): 16-B accesses where a tensor's buffers
 * share their offset from a 16-B boundary (a scalar head of up to 3 elements,
 * a scalar ragged tail), scalar otherwise.  28 B of traffic per element: an
 * HBM-bound stream, to be judged against gcnk_stream_copy_f32's rate.
 * ------------------------------------------------------------------------- */
#define GCNK_ADAM_MAX_TENSORS 8
#define GCNK_ADAM_CHUNK 2048
#define GCNK_ADAM_ZERO_GRAD 1
#define GCNK_ADAM_HOLD_STEP 2
typedef struct gcnk_adam_tensor {
  float* p;        /* parameter */
  float* g;        /* its gradient */
  float* m;        /* exp_avg */
  float* v;        /* exp_avg_sq */
  int64_t numel;
} gcnk_adam_tensor;
int gcnk_adam_f32(const gcnk_adam_tensor* t /* host */, int32_t ntensors, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int32_t* state, int32_t flags, void* stream);

/* The same step behind a gate (an addition within ABI 13): `gate` is a device
 * word written by an EARLIER launch on the same stream (gcnk_epoch_state's
 * `stopped`), so it is uniform over the launch.  *gate != 0: the launch changes
 * nothing -- no p, m or v, neither state word, no gradient zeroing (with
 * GCNK_ADAM_ZERO_GRAD too) -- so optimiser steps queued past the epoch that
 * stopped training leave the model where the loop that breaks there leaves it.
 * *gate == 0, or gate == NULL: gcnk_adam_f32, bit for bit (the same kernel).
 * The gate is read by the lane that reads the step word and reaches the other
 * lanes with the step factors, behind the same barrier.  Pass the gate to every
 * launch of one step, the GCNK_ADAM_HOLD_STEP ones included.  Arguments and
 * GCNK_EARG cases otherwise as gcnk_adam_f32. */
int gcnk_adam_gated_f32(const gcnk_adam_tensor* t /* host */, int32_t ntensors, double lr, double beta1,
                        double beta2, double eps, double weight_decay, int32_t* state, int32_t flags,
                        const int32_t* gate, void* stream);

/* ---------------------------------------------------------------------------
 * The tail of a training epoch in one launch (csrc/epoch.hip; an addition
 * within ABI 13): trainer.py:378-398 TopicGCNTrainer.val on the validation set
 * (the loss of trainer.py:383 and the counts behind accuracy / macro_f1),
 * trainer.py:372-376 the history row and the stopping decision of
 * utils.py:216-255 EarlyStopping, all on the DEVICE: a loop built on it never
 * waits for the GPU to decide, and may queue epochs ahead (a hipGraph of one
 * epoch, replayed).  It replaces gcnk_class_stats + gcnk_ce_forward_f32 (a
 * memset and three kernels), their device->host copy and the Python object.
 *
 * Inputs: logits [M x P] (ld), int64 `target` indexed by row, `counts` =
 * gcnk_ce_row_counts of the validation index set (NULL: every row once, n is
 * then M), n = the set's length, `train_loss` a device float (NULL: NaN is
 * recorded).  With e = state->epoch, for every row r with counts[r] > 0, in one
 * dense pass:
 *     lse_r, l_r     as gcnk_ce_forward_f32 forms them (the same code)
 *     pred_r         the first maximal logit, a NaN counting as maximal
 *                    (gcnk_class_stats: th.max semantics)
 *     pred_r == target[r]:  TP[pred_r] += counts[r], correct += counts[r]
 *     otherwise:            FP[pred_r] += counts[r], and FN[target[r]] +=
 *                           counts[r] when target[r] is inside [0, P)
 * so duplicates in the index set count as often as they occur; target[r] is
 * read for scored rows only.  The validation loss
 *     val_loss = fp32( (sum_r counts[r] * l_r) / n )
 * is summed in float64 with gcnk_ce_forward_f32's partition, tree and order:
 * it is BITWISE that function's result on the same inputs (NaN for n == 0 or a
 * scored target outside [0, P)).  The counts are integer atomics into the
 * history row: exact.  No float atomics, no memset node; no workgroup waits on
 * another (the workgroup that arrives last at state->arrivals finishes the
 * epoch), and two launches on equal inputs write bitwise equal rows.
 *
 * The last arriver then runs utils.py:238-255 in float64 on
 * score = -(double)val_loss:
 *     e == 0:                     best = score
 *     score < best + delta:       counter += 1; counter >= patience stops
 *                                 (reason GCNK_EPOCH_STOP_PATIENCE)
 *     otherwise:                  best = score, counter = 0
 * with exactly those comparisons (a NaN loss becomes `best`, an equal loss
 * resets the counter, as in the reference); not stopped and e + 1 == max_epoch
 * stops with reason GCNK_EPOCH_STOP_MAX_EPOCH.  It writes history row e
 *     float train_loss | float val_loss | int32 TP[P] | FP[P] | FN[P] | correct
 * (GCNK_EPOCH_ROW_WORDS(P) = 3 P + 3 four-byte words per row; rows are
 * consecutive), sets stop_epoch = e on a stop, `stopped` to the reason and
 * epoch = e + 1.
 *
 * state->stopped != 0 at entry: the launch writes NOTHING, no history row and
 * no state word (the same when state->epoch is outside [0, max_epoch), which
 * names no row).  `stopped` is the gate of gcnk_adam_gated_f32.
 *
 * The caller zeroes the state and the history (max_epoch rows) ONCE, before the
 * first launch of a run (all-zero is the initial state; the counts of row e are
 * added into it).  epoch and stopped are read by every workgroup at entry and
 * written only by the last arriver (gcnk_adam_f32's arrival hand-off, which
 * here also hands over the partials); `arrivals` is zero on entry and left
 * zero.  One launch at a time per state.  max_epoch, patience and delta are to be the same
 * in every launch of a run.
 *
 * 1 <= P <= 1024; workspace: gcnk_epoch_tail_workspace_bytes(M, P) bytes, 8-B
 * aligned (the loss partials: written before they are read, never zeroed).
 * GCNK_EARG (on the host, before any launch) for M < 0, P outside [1, 1024],
 * ld < P, n < 0, max_epoch < 1, patience < 0, a NaN delta, a NULL state,
 * history or workspace (or logits / target with M > 0), a state or workspace
 * not 8-B aligned, or a workspace too small.
 * ------------------------------------------------------------------------- */
#define GCNK_EPOCH_STOP_PATIENCE 1
#define GCNK_EPOCH_STOP_MAX_EPOCH 2
#define GCNK_EPOCH_ROW_WORDS(P) (3 * (P) + 3)
typedef struct gcnk_epoch_state {
  int32_t epoch;       /* epochs recorded: the index of the next history row */
  int32_t stopped;     /* 0: running; otherwise a GCNK_EPOCH_STOP_* reason -- the gate word */
  int32_t stop_epoch;  /* index of the epoch that stopped the run (valid when stopped != 0) */
  int32_t counter;     /* EarlyStopping.counter */
  double best;         /* EarlyStopping.best_score (set by the first epoch) */
  int32_t arrivals;    /* the launch's arrival counter: zero between launches */
  int32_t reserved;
} gcnk_epoch_state;    /* 32 bytes, 8-B aligned, on the device */
int64_t gcnk_epoch_tail_workspace_bytes(int32_t M, int32_t P);
int gcnk_epoch_tail_f32(const float* logits, int64_t ld, int32_t M, int32_t P, const int64_t* target,
                        const int32_t* counts, int64_t n, const float* train_loss, gcnk_epoch_state* state,
                        void* history, int32_t max_epoch, int32_t patience, double delta, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Keep the parameters of the best epoch (csrc/keep.hip; an addition within ABI
 * 13): utils.py:216-262 EarlyStopping.save_checkpoint at the two places where
 * the validation loss improved, utils.py:244 and utils.py:254 (both calls are
 * commented out in the reference, which therefore tests the model `patience`
 * epochs past its best).  ONE launch, queued on the stream right after
 * gcnk_epoch_tail_f32, copies up to GCNK_KEEP_MAX_TENSORS contiguous fp32
 * tensors src -> dst (the table travels in the kernel's arguments; more tensors
 * take further calls) -- but only if the tail that just ran recorded an epoch
 * that improved.  Nothing is decided on the host: the launch can be captured in
 * a hipGraph with the epoch and replayed.
 *
 * Every workgroup reads epoch_state->epoch, epoch_state->counter and
 * state->seen at entry (one lane, relaxed agent-scope loads, broadcast through
 * LDS: gcnk_adam_f32's step-word pattern).  All three were written by EARLIER
 * launches on the stream, so they are uniform over the launch.
 *     fresh = epoch > seen          a tail has recorded an epoch since the last look
 *     copy  = fresh && counter == 0
 * After a tail that recorded epoch e, counter == 0 holds exactly in the two
 * branches where the reference would have saved a checkpoint: e == 0, and
 * !(score < best + delta) -- which covers an equal loss and a NaN loss, as
 * gcnk_epoch_tail_f32 documents.
 *   copy:      each workgroup copies its chunk bit for bit (32-bit words: NaN
 *              payloads, -0.0 and denormals are preserved).
 *   not copy:  no byte of any dst is written.
 * Without GCNK_KEEP_HOLD_STATE the last workgroup to arrive at state->arrivals
 * (gcnk_adam_f32's arrival hand-off) stores seen = epoch and, when copy,
 * best = epoch (1 + the index of the epoch just kept) and copies += 1; then
 * arrivals = 0.  With GCNK_KEEP_HOLD_STATE the
 * launch reads and decides the same way, touches no state word and counts in
 * nowhere: for every call but the last of one keep over more than 8 tensors.
 *
 * After a stop the tail writes nothing, so `epoch` stands still and every later
 * keep launch is a no-op on all bytes.  A patience stop never copies (its
 * counter is >= 1); a max_epoch stop on an improving last epoch copies in that
 * epoch's own launch.  ONE keep (all its calls) per tail launch: two tails
 * between looks would be judged by the second one's `counter` alone.  One keep
 * at a time per state; the state is zeroed ONCE by the caller (all-zero is
 * initial).
 *
 * Work is cut into chunks of GCNK_KEEP_CHUNK elements, one workgroup (of 1,024
 * threads) each, by gcnk_adam_f32's chunk table (the chunk is four times that
 * step's, because what a launch costs beyond its copy is one arrival per
 * workgroup).  A chunk's loads are issued after the decision: a launch that does not copy
 * moves three words per workgroup.  dst is stored nontemporally (it is not read
 * again before a restore).  No allocation, no sync, no float atomics.
 *
 * GCNK_EARG (on the host, before any launch) for ntensors outside [0, 8]; a
 * NULL table, epoch_state or state; numel < 0; a NULL src or dst with
 * numel > 0; a src range overlapping its own or another tensor's dst range;
 * unknown flag bits; a state not 4-B aligned.  ntensors == 0 succeeds and does
 * nothing.
 * ------------------------------------------------------------------------- */
#define GCNK_KEEP_MAX_TENSORS 8
#define GCNK_KEEP_CHUNK 8192
#define GCNK_KEEP_HOLD_STATE 1   /* every launch but the last of one keep over more than 8 tensors */
typedef struct gcnk_keep_tensor {
  const float* src;    /* the live parameter */
  float* dst;          /* its best-epoch copy */
  int64_t numel;
} gcnk_keep_tensor;
typedef struct gcnk_keep_state {
  int32_t seen;        /* gcnk_epoch_state.epoch at the last launch that looked */
  int32_t best;        /* 1 + index of the epoch whose parameters dst holds; 0: nothing kept yet */
  int32_t arrivals;    /* the launch's arrival counter: zero between launches */
  int32_t copies;      /* launches (steps) that copied */
} gcnk_keep_state;     /* 16 bytes, 4-B aligned, on the device; all-zero is initial */
int gcnk_keep_best_f32(const gcnk_keep_tensor* t /* host */, int32_t ntensors, const gcnk_epoch_state* epoch_state,
                       gcnk_keep_state* state, int32_t flags, void* stream);

/* ---------------------------------------------------------------------------
 * Weighted edge-list loader (HOST pointers; no device work): the graph file
 * build_graph.py:199 writes (nx.write_weighted_edgelist: "u v weight" lines,
 * integer node ids) -> the symmetric float32 adjacency trainer.py:98-148
 * builds from it, as an int32 CSR with sorted, duplicate-free columns
 * (a repeated edge keeps its last weight; ids must be 0..n-1).
 * gcnk_edgelist_size gives n and nnz; gcnk_edgelist_csr fills host buffers
 * rowptr[n + 1], colind[nnz], val[nnz].
 * ------------------------------------------------------------------------- */
int gcnk_edgelist_size(const char* path, int64_t* n_nodes, int64_t* nnz);
int gcnk_edgelist_csr(const char* path, int64_t n_nodes, int64_t nnz, int32_t* rowptr, int32_t* colind, float* val);

/* The doc-topic graph built on the device (additions within ABI 13), declared in a
 * header of its own in this one's form. */
#include "gcnk_topic_graph.h"
/* The topic model on the device: documents' mixtures, the batch and the online fit,
 * and the variational bound, score and perplexity (additions within ABI 13), the
 * same way. */
#include "gcnk_lda.h"

/* ---------------------------------------------------------------------------
 * Dropout keep-mask exactly as the reference's CPU th.dropout draws it
 * (HOST pointers; layer.py:185 -> ATen dropout -> empty_like(x).bernoulli_(p)
 * with p = 1 - dropout): torch's serial CPU bernoulli_ takes one 64-bit draw
 * of the MT19937 generator per element, in order, and keeps the element when
 * (draw & (2^53 - 1)) * 2^-53 < p.  `state` (624 words), `left` and `next` are
 * the generator's state fields (torch's CPU generator state tensor), advanced
 * in place by the 2 n outputs consumed, so writing them back leaves the
 * process's random stream where the reference leaves it.  mask_out[n]: 1 =
 * kept.  One pass, one thread (the twist chain is serial); `threads` is
 * accepted and ignored.
 * ------------------------------------------------------------------------- */
int gcnk_bernoulli_mt19937(uint32_t* state, int32_t* left, int64_t* next, int64_t n, double p, uint8_t* mask_out,
                           int32_t threads);

/* The same draw on a native worker thread (a training loop draws the next
 * step's mask while the GPU runs this one).  *job receives a handle; the
 * buffers must stay alive and untouched until gcnk_bernoulli_mt19937_wait(job)
 * returns, and every started job is waited for exactly once. */
int gcnk_bernoulli_mt19937_start(uint32_t* state, int32_t* left, int64_t* next, int64_t n, double p,
                                 uint8_t* mask_out, void** job);
int gcnk_bernoulli_mt19937_wait(void* job);

/* Measurement floor (not on the GCN path): dst[0..n) = src[0..n) as one
 * float4 grid-stride launch -- the north-star SpMM's dense bytes with no CSR
 * and no gathers (bench.py's "copy" roofline line). */
int gcnk_stream_copy_f32(const float* src, float* dst, int64_t n, void* stream);

/* Debug only: in a library built with -DGCNK_STAMPS, when `buf` is non-null
 * every later row/tile SpMM launch writes 4 x uint64 s_memrealtime stamps
 * (100 MHz) per workgroup to it (entry, items staged, chunk walked, exit).
 * Process-global and not thread-safe, which is why the product build
 * compiles it out: there it returns GCNK_EUNSUP for a non-null buffer. */
int gcnk_debug_set_stamps(void* buf);

/* Counting words, CountVectorizer.transform against a fitted vocabulary (additions
 * within ABI 13), the same way. */
#include "gcnk_text.h"

#ifdef __cplusplus
}
#endif

#endif /* GCNK_H_ */
