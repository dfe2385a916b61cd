// Documents' topic mixtures on the device: the LDA E-step of sklearn's LatentDirichletAllocation.transform,
// which the reference calls in topic_model.py:133-164 (twice an experiment: build_graph.py, trainer.py:179).
// Per document d with word ids `ids`, counts c and beta_kw = exp(E[log beta])[k, ids[w]]
// (_lda.py _update_doc_distribution, then transform's row normalisation):
//     gamma = 1;  etheta_k = exp(psi(1) - psi(K))
//     at most max_doc_update_iter times:
//         phi_w    = sum_k etheta_k beta_kw + 2^-52
//         gamma'_k = etheta_k * sum_w (c_w / phi_w) beta_kw + alpha
//         etheta_k = exp(psi(gamma'_k) - psi(sum_k gamma'_k))
//         stop after this update if sum_k |gamma_k - gamma'_k| / K < tol;   gamma = gamma'
//     theta = gamma / sum_k gamma
// psi is Bernardo's AS 103 exactly as sklearn's _online_lda_fast.pyx states it ("optimized for speed, not
// accuracy"): an accurate digamma does not reproduce sklearn's theta.  All float64, and nothing is contracted
// to an FMA but the two dot products, which say fma().
//
// Schedule: ONE WAVE PER DOCUMENT, no communication between waves, no atomics, no workspace.  The model is a
// transposed table [V x ldt], so a word's K values are one contiguous row.  A wave gathers the rows of up to
// kTile words into LDS (16-byte buffer loads, sixteen in flight), then iterates on LDS alone:
//     phase 1  lane = word   phi_w, an in-lane sum over k ascending (etheta broadcast from LDS)
//     phase 2  lane = topic  sum_w, an in-lane sum over w in stored order (c_w / phi_w broadcast from LDS);
//                            lanes hold topics lane and lane + 64
//     then every lane adds gamma' and |gamma - gamma'| over k ascending from LDS, so the stop decision is the
//     same in all of them.
// A document of more than kTile words walks chunks of kTile words in stored order every iteration, staging
// each again from the table (which stays in L2); the phase-2 sums run on through the chunks, so every sum's
// order depends on the document's own word order and on K alone -- not on B, the document's place in the
// batch, kTile or the launch geometry.
// Bounded loops: psi shifts at most six times (NaN and x <= 1e-6 leave at once), the update loop runs at
// most max_iter <= kMaxIter times (a NaN makes the stop test false and runs to the cap), a document's waves
// stop independently.  A word id outside [0, V) is the caller's error and is not looked for; the table is
// read through a buffer resource, so such an id reads another row or zeros, never outside the table.
//
// The model's fit (sklearn's batch variational EM, _lda.py _em_step(batch_update=True), which the reference
// runs in topic_model.py:109-117) is three launches an EM iteration, all in this file:
//     exp_dirichlet   beta = exp(psi(lambda) - psi(row sum)) into the transposed table (as for transform)
//     fit E-step      the SAME update loop, instantiated a second time (kFit): it starts from a given gamma0
//                     row instead of 1, and after the loop walks the document's chunks once more with the
//                     final etheta: phi_w = sum_k etheta_k beta_kw + 2^-52, ratio[indptr[d] + w] = c_w / phi_w.
//                     It writes etheta [B x K] and that ratio per stored nonzero (and gamma, iterations).
//     M-step          lambda_kw = eta + S_kw beta_kw with S_kw = sum_d etheta_dk r_dw: ONE WAVE PER WORD, lane =
//                     topic (lane and lane + 64), down the word's entries in ascending document order through
//                     a word-major index (wptr, pos, doc) of the document-term matrix: s = s + etheta * r, the
//                     product rounded and then added as np.outer and += do, never an FMA, never an atomic.
//                     No word's chain is split: the order is the specification.  The chain's operands are
//                     loaded kLoads values ahead of the dependent adds.
// The online fit (_em_step(batch_update=False), learning_method='online' and partial_fit) runs the same three
// launches once per MINIBATCH of documents [doc_lo, doc_hi): the fit E-step on that row range, then
//     online M-step   lambda_kw = lambda_kw (1 - rho) + rho (eta + doc_ratio (S_kw beta_kw)), in place, S_kw the same
//                     chain over the word's entries whose document is in the minibatch: a contiguous sub-range of
//                     the whole matrix's index (entries ascend in document), found by two lower-bound searches.
// The M-step's loops run over [wptr[w], wptr[w + 1]) clamped to [0, nnz], nnz checked on the host; ratio and
// etheta are read (and ratio written) through buffer resources, so a bad index reads zeros or writes nothing.
//
// How good a model is (sklearn's _approx_bound, score, perplexity, bound_ and evaluate_every) is three more launches,
// stated above their kernels under "The variational bound": the documents' terms (one wave per document, this
// file's staging and LDS layout, a logsumexp that shifts theta's side only and reads the same table), the topics'
// terms (a workgroup per topic, the table builder's serial row sum) and one workgroup that sums both and the counts.
// Every sum has a fixed order: no atomics, no workspace, no host synchronisation.
//
// The entry points, at the end of the file and all declared in include/gcnk_lda.h, are four families, each with
// its refusals and launch stated once:
//     bound     gcnk_lda_bound_docs_f64 (check_table, check_documents), gcnk_lda_bound_topics_f64,
//               gcnk_lda_bound_finish_f64 (check_topics)
//     tables    gcnk_lda_exp_dirichlet_f64, gcnk_lda_table_from_exp_f64: check_table, then their own source check
//     E-step    gcnk_lda_estep_f64 (transform), gcnk_lda_estep_fit_f64 (both fits): estep_args -- check_table, the
//               document refusals, the common EStep fields -- then each one's own outputs; launch_estep<kFit>
//     M-step    gcnk_lda_mstep_f64 (batch), gcnk_lda_mstep_online_f64 (online, partial_fit): mstep_args the same
//               way, the online one then its minibatch, rho and doc_ratio; launch_mstep picks one or two topics a lane
#include "gcnk_common.h"

#pragma clang fp contract(off)

namespace gcnk {
namespace {

constexpr int kTile = 64;          // words a wave holds in LDS: one per lane
constexpr int kDocs = 2;           // documents (waves) per workgroup: 2 x 68 KB of LDS at K = 128
constexpr int kMaxTopics = 128;    // two topics a lane
constexpr int kStage = 16;         // table rows a wave has in flight while it stages (64 VGPRs; LDS, not registers, sets the occupancy)
constexpr int kMaxIter = 10000;
constexpr double kEuler = 0.577215664901532860606512090082402431;
constexpr double kEps = 2.220446049250313080847263336181640625e-16;   // np.finfo(np.float64).eps

static_assert(kTile == 64 && kMaxTopics == 2 * 64, "a lane per word, two topics per lane");

// _online_lda_fast.pyx psi(), operation for operation
__device__ __forceinline__ double psi(double x) {
  if (x <= 1e-6) return -kEuler - 1.0 / x;
  double result = 0.0;
  for (int i = 0; i < 6 && x < 6.0; ++i) {   // x > 1e-6 is past 6 after six shifts
    result -= 1.0 / x;
    x += 1.0;
  }
  double r = 1.0 / x;
  result += log(x) - 0.5 * r;
  r = r * r;
  result -= r * ((1.0 / 12.0) - r * ((1.0 / 120.0) - r * (1.0 / 252.0)));
  return result;
}

// LDS written by some lanes of this wave is read by others: order the accesses, nothing else
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double readlane_f64(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j),
                          __builtin_amdgcn_readlane(__double2loint(v), j));
}

__host__ __device__ constexpr int tile_stride(int K) { return K | 1; }   // odd: a lane per row reads without bank conflicts
__host__ __device__ constexpr int topics_even(int K) { return (K + 1) & ~1; }
// a wave's LDS in doubles: tile | etheta | gamma' | |gamma - gamma'| | c / phi
__host__ __device__ constexpr int wave_doubles(int K) { return kTile * tile_stride(K) + 3 * topics_even(K) + kTile; }

struct EStep {
  const int32_t* indptr;
  const int32_t* indices;
  const void* counts;
  int32_t counts_kind;   // 0 float64, 1 int32, 2 int64
  int32_t B, K;
  const double* table;
  uint32_t row_bytes, table_bytes;
  double alpha, tol;
  int32_t max_iter;
  double* theta;
  double* gamma;
  int64_t ldth;
  int32_t* iters;
  float* x;
  int64_t ldx;
  float* a;
  int64_t lda;
  double threshold;
  // the fit variant alone
  const double* gamma0;
  int64_t ldg0;
  double* etheta;
  int64_t lde;
  double* ratio;
  uint32_t ratio_bytes;
};

// a stored count as float64: counts_kind 0 float64, 1 int32, 2 int64 (widened exactly)
__device__ __forceinline__ double count_at(const void* counts, int32_t counts_kind, int64_t i) {
  if (counts_kind == 0) return static_cast<const double*>(counts)[i];
  if (counts_kind == 1) return (double)static_cast<const int32_t*>(counts)[i];
  return (double)static_cast<const int64_t*>(counts)[i];
}

// tile[w * Ks + k] = table[id_w, k] for the m words whose ids the lanes hold (lane w: word w)
__device__ __forceinline__ void stage_words(__amdgpu_buffer_rsrc_t table, uint32_t row_bytes, int K, int Ks, int32_t id,
                                            int m, int lane, double* tile) {
  const bool c0 = 2 * lane < K, c1 = 2 * lane + 1 < K;
  for (int w0 = 0; w0 < m; w0 += kStage) {
    f64x2 v[kStage];
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int w = w0 + u;
      const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(id, w & 63);
      v[u] = buf_load_f64x2(table, w < m && c0 ? row * row_bytes + 16u * (uint32_t)lane : kBufOob);
    }
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int w = w0 + u;
      if (w < m) {
        if (c0) tile[w * Ks + 2 * lane] = v[u][0];
        if (c1) tile[w * Ks + 2 * lane + 1] = v[u][1];
      }
    }
  }
}

// kFit false: transform (gamma = 1 at the start; theta, gamma, iterations, the scorer's operands).
// kFit true: the fit's E-step (gamma0 given; etheta, the ratio of every stored nonzero, gamma, iterations).
template <bool kFit>
__global__ void __launch_bounds__(64 * kDocs)
lda_estep_kernel(EStep p) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t d = (int32_t)blockIdx.x * kDocs + wv;
  if (d >= p.B) return;
  const int K = p.K, Ks = tile_stride(K), Kr = topics_even(K);
  double* tile = lds + (size_t)wv * wave_doubles(K);
  double* et = tile + kTile * Ks;
  double* gm = et + Kr;
  double* df = gm + Kr;
  double* rr = df + Kr;
  const int64_t b = p.indptr[d];
  const int64_t e = p.indptr[d + 1];
  const int32_t n = e > b ? (int32_t)(e - b) : 0;
  const int nchunk = (n + kTile - 1) / kTile;
  const __amdgpu_buffer_rsrc_t table = buffer_rsrc(p.table, p.table_bytes);

  const int k0 = lane, k1 = lane + 64;
  const bool on0 = k0 < K, on1 = k1 < K;
  const int r0 = on0 ? k0 : K - 1, r1 = on1 ? k1 : K - 1;   // (a lane without a topic repeats the last one, unstored)
  const bool two = K > 64;

  int32_t id = 0;
  double cnt = 0.0;
  auto load_words = [&](int c) {
    const int32_t w = c * kTile + lane;
    id = w < n ? p.indices[b + w] : 0;
    cnt = w < n ? count_at(p.counts, p.counts_kind, b + w) : 0.0;
  };

  double g0 = 1.0, g1 = 1.0;
  double e0 = exp(psi(1.0) - psi((double)K)), e1 = e0;
  double total = (double)K;   // sum_k gamma_k, ascending
  if constexpr (kFit) {
    g0 = p.gamma0[(int64_t)d * p.ldg0 + r0];
    g1 = p.gamma0[(int64_t)d * p.ldg0 + r1];
    if (on0) gm[k0] = g0;
    if (on1) gm[k1] = g1;
    wave_sync();
    total = 0.0;
    for (int k = 0; k < K; ++k) total += gm[k];
    const double psi_total = psi(total);
    e0 = exp(psi(g0) - psi_total);
    e1 = exp(psi(g1) - psi_total);
  }
  if (on0) et[k0] = e0;
  if (on1) et[k1] = e1;
  if (nchunk == 1) {
    load_words(0);
    stage_words(table, p.row_bytes, K, Ks, id, n, lane, tile);
  }
  wave_sync();

  // phase 1, lane = word (a lane past the chunk's end computes on stale LDS and is not read): c_w / phi_w
  auto ratio_of_lane = [&]() {
    const double* mine = tile + lane * Ks;
    double phi = 0.0;
    for (int k = 0; k < K; ++k) phi = fma(et[k], mine[k], phi);
    phi += kEps;
    return cnt / phi;
  };

  int32_t its = 0;
  for (int it = 0; it < p.max_iter; ++it) {
    double a0 = 0.0, a1 = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      const int m = min(kTile, n - c * kTile);
      if (nchunk > 1) {
        load_words(c);
        stage_words(table, p.row_bytes, K, Ks, id, m, lane, tile);
        wave_sync();
      }
      rr[lane] = ratio_of_lane();
      wave_sync();
      // phase 2, lane = topic
      if (two) {
        for (int w = 0; w < m; ++w) {
          const double r = rr[w];
          a0 = fma(r, tile[w * Ks + r0], a0);
          a1 = fma(r, tile[w * Ks + r1], a1);
        }
      } else {
        for (int w = 0; w < m; ++w) a0 = fma(rr[w], tile[w * Ks + r0], a0);
      }
      wave_sync();   // (the next chunk rewrites tile and rr)
    }
    const double n0 = e0 * a0 + p.alpha, n1 = e1 * a1 + p.alpha;
    if (on0) {
      gm[k0] = n0;
      df[k0] = fabs(g0 - n0);
    }
    if (on1) {
      gm[k1] = n1;
      df[k1] = fabs(g1 - n1);
    }
    wave_sync();
    double change = 0.0;
    total = 0.0;
    for (int k = 0; k < K; ++k) {
      total += gm[k];
      change += df[k];
    }
    const double psi_total = psi(total);
    e0 = exp(psi(n0) - psi_total);
    e1 = exp(psi(n1) - psi_total);
    g0 = n0;
    g1 = n1;
    if (on0) et[k0] = e0;
    if (on1) et[k1] = e1;
    wave_sync();
    ++its;
    if (__builtin_amdgcn_readfirstlane((int)(change / (double)K < p.tol))) break;
  }

  if constexpr (kFit) {
    // once more with the final etheta (in LDS since the last update, or the start): every stored nonzero's ratio
    const __amdgpu_buffer_rsrc_t ratio = buffer_rsrc(p.ratio, p.ratio_bytes);
    for (int c = 0; c < nchunk; ++c) {
      const int m = min(kTile, n - c * kTile);
      if (nchunk > 1) {
        load_words(c);
        stage_words(table, p.row_bytes, K, Ks, id, m, lane, tile);
        wave_sync();
      }
      const double r = ratio_of_lane();
      buf_store_f64(r, ratio, lane < m ? (uint32_t)(b + c * kTile + lane) * 8u : kBufOob);
      wave_sync();   // (the next chunk rewrites tile)
    }
    if (on0) p.etheta[(int64_t)d * p.lde + k0] = e0;
    if (on1) p.etheta[(int64_t)d * p.lde + k1] = e1;
    if (p.gamma) {
      if (on0) p.gamma[(int64_t)d * p.ldth + k0] = g0;
      if (on1) p.gamma[(int64_t)d * p.ldth + k1] = g1;
    }
    if (p.iters && lane == 0) p.iters[d] = its;
    return;
  }

  const double t0 = g0 / total, t1 = g1 / total;
  const int64_t row = (int64_t)d * p.ldth;
  if (p.theta) {
    if (on0) p.theta[row + k0] = t0;
    if (on1) p.theta[row + k1] = t1;
  }
  if (p.gamma) {
    if (on0) p.gamma[row + k0] = g0;
    if (on1) p.gamma[row + k1] = g1;
  }
  if (p.iters && lane == 0) p.iters[d] = its;
  if (!p.x) return;

  // what the scorer reads, as inductive.from_theta makes it from this theta: x = theta / (sum theta + 1e-8)
  // rounded to fp32, over its float64 norm, rounded to fp32; a = theta where theta >= threshold
  if (on0) gm[k0] = t0;
  if (on1) gm[k1] = t1;
  wave_sync();
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += gm[k];
  const double den = s + 1e-8;
  const double q0 = (double)(float)(t0 / den), q1 = (double)(float)(t1 / den);
  if (on0) df[k0] = q0 * q0;
  if (on1) df[k1] = q1 * q1;
  wave_sync();
  double ss = 0.0;
  for (int k = 0; k < K; ++k) ss += df[k];
  double norm = sqrt(ss);
  if (norm == 0.0) norm = 1.0;
  if (on0) {
    p.x[(int64_t)d * p.ldx + k0] = (float)(q0 / norm);
    p.a[(int64_t)d * p.lda + k0] = t0 >= p.threshold ? (float)t0 : 0.0f;
  }
  if (on1) {
    p.x[(int64_t)d * p.ldx + k1] = (float)(q1 / norm);
    p.a[(int64_t)d * p.lda + k1] = t1 >= p.threshold ? (float)t1 : 0.0f;
  }
}

// sum_w row[w], serially and ascending in w, in every lane of the wave: 64 values a load, added one after the
// other (a lane past the row's end holds +0, which leaves the sum as it is)
__device__ __forceinline__ double row_sum_serial(const double* __restrict__ row, int32_t V, int lane) {
  double s = 0.0;
  for (int32_t base = 0; base < V; base += 4 * 64) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = base + 64 * u + lane < V ? row[base + 64 * u + lane] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (base + 64 * u >= V) break;
#pragma unroll
      for (int j = 0; j < 64; ++j) s += readlane_f64(v[u], j);
    }
  }
  return s;
}

// A workgroup per topic: exp(psi(lambda_kw) - psi(sum_w lambda_kw)) into column k of the table.  Every wave
// takes the row sum for itself (row_sum_serial).
__global__ void __launch_bounds__(256)
lda_exp_dirichlet_kernel(const double* __restrict__ lam, int64_t ldc, int32_t V, double* __restrict__ table,
                         int64_t ldt) {
  const int k = blockIdx.x, lane = threadIdx.x & 63;
  const double* row = lam + (int64_t)k * ldc;
  const double psi_row = psi(row_sum_serial(row, V, lane));
  for (int32_t w = threadIdx.x; w < V; w += 256) table[(int64_t)w * ldt + k] = exp(psi(row[w]) - psi_row);
}

__global__ void __launch_bounds__(256)
lda_transpose_kernel(const double* __restrict__ src, int64_t lde, int32_t K, int32_t V, double* __restrict__ table,
                     int64_t ldt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)K * V) return;
  const int32_t w = (int32_t)(i / K), k = (int32_t)(i - (int64_t)w * K);
  table[(int64_t)w * ldt + k] = src[(int64_t)k * lde + w];
}

struct MStep {
  const int32_t* wptr;
  const int32_t* pos;
  const int32_t* doc;
  int64_t nnz;
  int32_t V, K;
  const double* ratio;
  uint32_t ratio_bytes;
  const double* etheta;
  uint32_t et_row_bytes, et_bytes;
  const double* table;
  int64_t ldt;
  double eta;
  double* lambda;
  int64_t ldl;
};

constexpr int kWords = 4;    // words (waves) per workgroup
constexpr int kLoads = 32;   // etheta loads a wave keeps in flight ahead of its add chain (64 VGPRs)

// The M-step's sum for one word: over the entries [b, e) of the word-major index, ascending, of
// etheta[doc, k] * ratio[pos], into s0 (topic lane) and s1 (topic lane + 64, kTwo alone).  Both M-step kernels
// instantiate this one chain.
// A wave takes 64 entries' (doc, ratio) a load, lane = entry, the next 64 while it works on these.  Then, lane =
// topic, the etheta values of the next R entries sit in a ring of R registers (R = kLoads with one topic a lane,
// kLoads / 2 with two): the wave adds the entry in slot u and at once loads the entry R further on into that
// slot, from the next 64 when it lies there, so R entries' loads are in flight all the way down the chain.
template <bool kTwo>
__device__ __forceinline__ void mstep_chain(const MStep& p, int64_t b, int64_t e, int lane, double& s0, double& s1) {
  constexpr int R = kTwo ? kLoads / 2 : kLoads;
  static_assert(64 % R == 0 && 64 / R >= 2, "a ring refilled from the next 64 entries in the last group of these");
  const int K = p.K;
  const int k0 = lane, k1 = lane + 64;
  const bool on0 = k0 < K, on1 = kTwo && k1 < K;
  const __amdgpu_buffer_rsrc_t ratio = buffer_rsrc(p.ratio, p.ratio_bytes);
  const __amdgpu_buffer_rsrc_t et = buffer_rsrc(p.etheta, p.et_bytes);

  int32_t dd = 0, ddn = 0;
  double rr = 0.0, rrn = 0.0;
  auto load_entries = [&](int64_t i0, int32_t& d_out, double& r_out) {   // lane = entry
    const bool live = i0 + lane < e;
    d_out = live ? p.doc[i0 + lane] : 0;
    r_out = buf_load_f64(ratio, live ? (uint32_t)p.pos[i0 + lane] * 8u : kBufOob);
  };
  double a0[R], a1[R];
  // slot u <- etheta[document held by lane l of d, this lane's topics] (nothing is read for a dead entry)
  auto fetch = [&](int u, int32_t d, int l, bool live) {
    const uint32_t row = (uint32_t)__builtin_amdgcn_readlane(d, l) * p.et_row_bytes;
    a0[u] = buf_load_f64(et, live && on0 ? row + 8u * (uint32_t)k0 : kBufOob);
    if (kTwo) a1[u] = buf_load_f64(et, live && on1 ? row + 8u * (uint32_t)k1 : kBufOob);
  };

  s0 = 0.0;
  s1 = 0.0;
  load_entries(b, dd, rr);
  {
    const int m = (int)min((int64_t)64, e - b);
#pragma unroll
    for (int u = 0; u < R; ++u) fetch(u, dd, u, u < m);
  }
  for (int64_t i0 = b; i0 < e; i0 += 64) {
    const int m = (int)min((int64_t)64, e - i0);                       // entries here: 1 .. 64
    const int mn = (int)min((int64_t)64, e - i0 - m);                  // and in the next 64: 0 unless m == 64
    load_entries(i0 + 64, ddn, rrn);
    for (int u0 = 0; u0 < m; u0 += R) {
      const bool wrap = u0 + R >= 64;   // the entries R further on are the next 64's first R
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int j = u0 + u;
        if (j < m) {
          const double r = readlane_f64(rr, j);
          const double q0 = a0[u] * r;   // (rounded, then added: contraction is off in this file)
          s0 = s0 + q0;
          if (kTwo) {
            const double q1 = a1[u] * r;
            s1 = s1 + q1;
          }
        }
        const int l = (j + R) & 63;
        fetch(u, wrap ? ddn : dd, l, wrap ? l < mn : j + R < m);
      }
    }
    dd = ddn;
    rr = rrn;
  }
}

// lambda[k, w] = eta + (sum over the word's entries, ascending document, of etheta[doc, k] * ratio[pos]) * beta[k, w]:
// one wave per word, lane = topic.
template <bool kTwo>
__global__ void __launch_bounds__(64 * kWords)
lda_mstep_kernel(MStep p) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t w = (int32_t)blockIdx.x * kWords + wv;
  if (w >= p.V) return;
  const int k0 = lane, k1 = lane + 64;
  const bool on0 = k0 < p.K, on1 = kTwo && k1 < p.K;
  const int64_t b = max((int64_t)p.wptr[w], (int64_t)0);
  const int64_t e = min((int64_t)p.wptr[w + 1], p.nnz);
  double s0, s1;
  mstep_chain<kTwo>(p, b, e, lane, s0, s1);

  const double* beta = p.table + (int64_t)w * p.ldt;
  if (on0) p.lambda[(int64_t)k0 * p.ldl + w] = p.eta + s0 * beta[k0];
  if (on1) p.lambda[(int64_t)k1 * p.ldl + w] = p.eta + s1 * beta[k1];
}

// The online M-step (_lda.py _em_step(batch_update=False)) of the minibatch of documents [doc_lo, doc_hi), in place:
//     lambda[k, w] = lambda[k, w] * (1 - rho) + rho * (eta + doc_ratio * (S_kw * beta[k, w]))
// with S_kw the chain above over the word's entries whose document lies in the minibatch.  The index is the whole
// matrix's: a word's entries ascend in document, so the minibatch's are one contiguous sub-range, which the wave
// finds with two lower-bound searches on doc (every lane the same search, wave-uniform loads).  Every word is
// blended, with S = 0 where the minibatch does not hold it: sklearn's dense read-modify-write.
struct MStepOnline {
  MStep m;
  int32_t doc_lo, doc_hi;
  double rho, doc_ratio;
};

// the first i in [b, e) with doc[i] >= d, or e
__device__ __forceinline__ int64_t doc_lower_bound(const int32_t* __restrict__ doc, int64_t b, int64_t e, int32_t d) {
  while (b < e) {   // (at most 32 halvings: e - b < 2^31)
    const int64_t mid = b + ((e - b) >> 1);
    if (doc[mid] < d)
      b = mid + 1;
    else
      e = mid;
  }
  return b;
}

template <bool kTwo>
__global__ void __launch_bounds__(64 * kWords)
lda_mstep_online_kernel(MStepOnline q) {
  const MStep& p = q.m;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t w = (int32_t)blockIdx.x * kWords + wv;
  if (w >= p.V) return;
  const int k0 = lane, k1 = lane + 64;
  const bool on0 = k0 < p.K, on1 = kTwo && k1 < p.K;
  const int64_t wb = max((int64_t)p.wptr[w], (int64_t)0);
  const int64_t we = max(min((int64_t)p.wptr[w + 1], p.nnz), wb);
  const int64_t b = doc_lower_bound(p.doc, wb, we, q.doc_lo);
  const int64_t e = doc_lower_bound(p.doc, b, we, q.doc_hi);
  const double keep = 1.0 - q.rho;   // (formed once, from the rho passed in; +0 at rho = 1)
  double s0, s1;
  mstep_chain<kTwo>(p, b, e, lane, s0, s1);

  const double* beta = p.table + (int64_t)w * p.ldt;
  auto blend = [&](int k, double s) {
    double* at = p.lambda + (int64_t)k * p.ldl + w;
    const double ss = s * beta[k];
    const double t = q.doc_ratio * ss;
    const double u = p.eta + t;
    const double v = q.rho * u;
    const double a = *at * keep;
    *at = a + v;
  };
  if (on0) blend(k0, s0);
  if (on1) blend(k1, s1);
}

// ---- The variational bound (sklearn's _approx_bound, score, perplexity): three launches, no atomics, no workspace.

// v of the wave's 64 lanes summed in one fixed tree: lanes 2i and 2i + 1, then those sums in pairs, and so on
// (partners lane ^ 1, 2, 4, 8, 16, 32).  Both partners add the same two numbers, so every lane holds the total.
template <typename T>
__device__ __forceinline__ T wave_tree_sum(T v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// v of the workgroup's threads: wave_tree_sum in every wave, then the waves' sums one after the other in
// ascending wave order; every thread holds the total.  `waves`: LDS for one value a wave.
template <typename T>
__device__ __forceinline__ T block_tree_sum(T v, T* waves) {
  const int nwave = (int)(blockDim.x >> 6);
  v = wave_tree_sum(v);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = waves[0];
  for (int q = 1; q < nwave; ++q) s += waves[q];
  __syncthreads();   // (the caller may hand `waves` to the next sum)
  return s;
}

struct BoundDocs {
  const int32_t* indptr;
  const int32_t* indices;
  const void* counts;
  int32_t counts_kind;
  int32_t B, K;
  const double* table;
  uint32_t row_bytes, table_bytes;
  const double* gamma;
  int64_t ldg;
  double alpha;
  double* doc_bound;
};

// One wave per document, the E-step's geometry and LDS layout.  With l_k = psi(gamma_k) - psi(sum_k gamma_k),
// m = max_k l_k and e_k = exp(l_k - m):
//     words = sum_w c_w (m + log(sum_k e_k table[id_w, k]))     (logsumexp_k(l_k + E[log beta_kw]), theta's side shifted)
//     s1 = sum_k (alpha - gamma_k) l_k      s2 = sum_k (lgamma(gamma_k) - lgamma(alpha))
//     s3 = lgamma(alpha K) - lgamma(sum_k gamma_k)
//     doc_bound = ((words + s1) + s2) + s3
// Orders: every sum over k ascends, in-lane from LDS (the dot product by fma, as the E-step's phi).  The words go
// in stored order in tiles of kTile: lane = word, the tile's 64 terms (+0 past the document's end) by
// wave_tree_sum, the tiles' sums added one after the other.  Nothing depends on B, d or the launch.
__global__ void __launch_bounds__(64 * kDocs)
lda_bound_docs_kernel(BoundDocs p) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t d = (int32_t)blockIdx.x * kDocs + wv;
  if (d >= p.B) return;
  const int K = p.K, Ks = tile_stride(K), Kr = topics_even(K);
  double* tile = lds + (size_t)wv * wave_doubles(K);
  double* et = tile + kTile * Ks;   // l_k, then e_k
  double* gm = et + Kr;             // gamma_k, then s2's addends
  double* df = gm + Kr;             // s1's addends
  const int64_t b = p.indptr[d];
  const int64_t e = p.indptr[d + 1];
  const int32_t n = e > b ? (int32_t)(e - b) : 0;
  const int nchunk = (n + kTile - 1) / kTile;
  const __amdgpu_buffer_rsrc_t table = buffer_rsrc(p.table, p.table_bytes);

  const int k0 = lane, k1 = lane + 64;
  const bool on0 = k0 < K, on1 = k1 < K;
  const int r0 = on0 ? k0 : K - 1, r1 = on1 ? k1 : K - 1;
  const double g0 = p.gamma[(int64_t)d * p.ldg + r0], g1 = p.gamma[(int64_t)d * p.ldg + r1];
  if (on0) gm[k0] = g0;
  if (on1) gm[k1] = g1;
  wave_sync();
  double total = 0.0;
  for (int k = 0; k < K; ++k) total += gm[k];
  const double psi_total = psi(total);
  const double l0 = psi(g0) - psi_total, l1 = psi(g1) - psi_total;
  if (on0) {
    et[k0] = l0;
    df[k0] = (p.alpha - g0) * l0;
  }
  if (on1) {
    et[k1] = l1;
    df[k1] = (p.alpha - g1) * l1;
  }
  wave_sync();
  double mx = et[0], s1 = 0.0;
  for (int k = 0; k < K; ++k) {
    mx = fmax(mx, et[k]);
    s1 += df[k];
  }
  wave_sync();   // (et and gm are rewritten)
  const double lg_alpha = lgamma(p.alpha);
  if (on0) {
    et[k0] = exp(l0 - mx);
    gm[k0] = lgamma(g0) - lg_alpha;
  }
  if (on1) {
    et[k1] = exp(l1 - mx);
    gm[k1] = lgamma(g1) - lg_alpha;
  }
  wave_sync();
  double s2 = 0.0;
  for (int k = 0; k < K; ++k) s2 += gm[k];
  const double s3 = lgamma(p.alpha * (double)K) - lgamma(total);

  double words = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    const int m = min(kTile, n - c * kTile);
    const int32_t w = c * kTile + lane;
    const int32_t id = w < n ? p.indices[b + w] : 0;
    const double cnt = w < n ? count_at(p.counts, p.counts_kind, b + w) : 0.0;
    stage_words(table, p.row_bytes, K, Ks, id, m, lane, tile);
    wave_sync();
    const double* mine = tile + lane * Ks;   // (a lane past the chunk's end computes on stale LDS and adds +0)
    double dot = 0.0;
    for (int k = 0; k < K; ++k) dot = fma(et[k], mine[k], dot);
    const double term = cnt * (mx + log(dot));
    words += wave_tree_sum(lane < m ? term : 0.0);
    wave_sync();   // (the next chunk rewrites tile)
  }
  if (lane == 0) p.doc_bound[d] = ((words + s1) + s2) + s3;
}

constexpr int kTopicThreads = 256;    // the topic term's chunk: addend w belongs to thread w mod 256
constexpr int kFinishThreads = 1024;

// A workgroup per topic.  With L = sum_w lambda_kw (row_sum_serial, as the table's builder takes it):
//     s1 = sum_w (eta - lambda_kw) (psi(lambda_kw) - psi(L))      s2 = sum_w (lgamma(lambda_kw) - lgamma(eta))
//     topic_bound = (s1 + s2) + (lgamma(eta V) - lgamma(L))
// Order of s1 and s2: thread t adds the words t, t + 256, ... in ascending order, then block_tree_sum.
__global__ void __launch_bounds__(kTopicThreads)
lda_bound_topics_kernel(const double* __restrict__ lam, int64_t ldl, int32_t V, double eta,
                        double* __restrict__ topic_bound) {
  __shared__ double waves[kTopicThreads / 64];
  const int k = blockIdx.x, lane = threadIdx.x & 63;
  const double* row = lam + (int64_t)k * ldl;
  const double L = row_sum_serial(row, V, lane);
  const double psi_row = psi(L), lg_eta = lgamma(eta);
  double a1 = 0.0, a2 = 0.0;
  for (int32_t w = threadIdx.x; w < V; w += kTopicThreads) {
    const double x = row[w];
    a1 += (eta - x) * (psi(x) - psi_row);
    a2 += lgamma(x) - lg_eta;
  }
  const double s1 = block_tree_sum(a1, waves);
  const double s2 = block_tree_sum(a2, waves);
  if (threadIdx.x == 0) topic_bound[k] = (s1 + s2) + (lgamma(eta * (double)V) - lgamma(L));
}

// One workgroup: out[0] = bound = doc_ratio * sum_d doc_bound[d] + sum_k topic_bound[k], out[1] = the word count
// sum of counts[indptr[0] .. indptr[B]), out[2] = perplexity = exp(-(bound / (count * doc_ratio))).  Every sum:
// thread t adds the elements t, t + 1024, ... in ascending order, then block_tree_sum; integer counts in int64.
__global__ void __launch_bounds__(kFinishThreads)
lda_bound_finish_kernel(const double* __restrict__ doc_bound, int32_t B, const double* __restrict__ topic_bound,
                        int32_t K, const int32_t* __restrict__ indptr, const void* __restrict__ counts,
                        int32_t counts_kind, double doc_ratio, double* __restrict__ out) {
  __shared__ double waves[kFinishThreads / 64];
  __shared__ long long iwaves[kFinishThreads / 64];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int32_t d = t; d < B; d += kFinishThreads) a += doc_bound[d];
  const double docs = block_tree_sum(a, waves);
  double q = 0.0;
  for (int32_t k = t; k < K; k += kFinishThreads) q += topic_bound[k];
  const double topics = block_tree_sum(q, waves);
  const int64_t lo = indptr[0], hi = indptr[B];
  double count;
  if (counts_kind == 0) {
    double c = 0.0;
    for (int64_t i = lo + t; i < hi; i += kFinishThreads) c += static_cast<const double*>(counts)[i];
    count = block_tree_sum(c, waves);
  } else {
    long long c = 0;
    for (int64_t i = lo + t; i < hi; i += kFinishThreads)
      c += counts_kind == 1 ? (long long)static_cast<const int32_t*>(counts)[i]
                            : (long long)static_cast<const int64_t*>(counts)[i];
    count = (double)block_tree_sum(c, iwaves);
  }
  if (t != 0) return;
  const double scaled = doc_ratio * docs;
  const double bound = scaled + topics;
  const double per_word = bound / (count * doc_ratio);
  out[0] = bound;
  out[1] = count;
  out[2] = exp(-1.0 * per_word);
}

// K in range, the table's rows 16-byte accesses, every byte offset into it below kBufOob
int check_table(const char* who, int32_t K, int32_t V, const void* table, int64_t ldt) {
  if (K < 1 || V < 1) {
    set_error("%s: needs K >= 1 and V >= 1 (K=%d V=%d)", who, K, V);
    return GCNK_EARG;
  }
  if (K > kMaxTopics) {
    set_error("%s: K=%d topics, the kernels take at most %d", who, K, kMaxTopics);
    return GCNK_EUNSUP;
  }
  if (!table || !aligned16(table) || ldt < K || (ldt & 1)) {
    set_error("%s: the table must be non-null, 16-byte aligned, with an even ldt >= K (ldt=%lld K=%d)", who,
              (long long)ldt, K);
    return GCNK_EARG;
  }
  if ((int64_t)V * ldt * 8 >= (int64_t)kBufOob) {
    set_error("%s: a table of %lld bytes is past the 32-bit offsets of its buffer resource (V=%d ldt=%lld)", who,
              (long long)((int64_t)V * ldt * 8), V, (long long)ldt);
    return GCNK_EUNSUP;
  }
  return GCNK_OK;
}

// (NaN and +inf fail)
bool finite_positive(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }

// a document batch: B >= 1, its three arrays, a count kind the kernels widen
int check_documents(const char* who, const int32_t* indptr, const int32_t* indices, const void* counts,
                    int32_t counts_kind, int32_t B) {
  if (B < 1 || !indptr || !indices || !counts) {
    set_error("%s: needs B >= 1 and non-null indptr, indices and counts (B=%d)", who, B);
    return GCNK_EARG;
  }
  if (counts_kind < 0 || counts_kind > 2) {
    set_error("%s: counts_kind %d is not 0 (float64), 1 (int32) or 2 (int64)", who, counts_kind);
    return GCNK_EARG;
  }
  return GCNK_OK;
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int32_t gcnk_lda_max_topics(void) { return kMaxTopics; }

extern "C" int32_t gcnk_lda_tile_words(void) { return kTile; }

extern "C" int32_t gcnk_lda_docs_per_block(void) { return kDocs; }

extern "C" int gcnk_lda_exp_dirichlet_f64(const double* components, int64_t ldc, int32_t K, int32_t V, double* table,
                                          int64_t ldt, void* stream) {
  const char* who = "gcnk_lda_exp_dirichlet_f64";
  const int rc = check_table(who, K, V, table, ldt);
  if (rc) return rc;
  if (!components || ldc < V) {
    set_error("%s: null components or ldc=%lld < V=%d", who, (long long)ldc, V);
    return GCNK_EARG;
  }
  hipLaunchKernelGGL(lda_exp_dirichlet_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, components, ldc, V,
                     table, ldt);
  return launch_check("lda_exp_dirichlet_kernel");
}

extern "C" int gcnk_lda_table_from_exp_f64(const double* exp_topic_word, int64_t lde, int32_t K, int32_t V,
                                           double* table, int64_t ldt, void* stream) {
  const char* who = "gcnk_lda_table_from_exp_f64";
  const int rc = check_table(who, K, V, table, ldt);
  if (rc) return rc;
  if (!exp_topic_word || lde < V) {
    set_error("%s: null exp_topic_word or lde=%lld < V=%d", who, (long long)lde, V);
    return GCNK_EARG;
  }
  const int64_t nblk = ((int64_t)K * V + 255) / 256;
  hipLaunchKernelGGL(lda_transpose_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, exp_topic_word, lde,
                     K, V, table, ldt);
  return launch_check("lda_transpose_kernel");
}

// the refusals both E-step entry points share, then the kernel's common arguments (gamma and iters may be null)
static int estep_args(const char* who, const int32_t* indptr, const int32_t* indices, const void* counts,
                      int32_t counts_kind, int32_t B, int32_t V, int32_t K, const double* table, int64_t ldt,
                      double alpha, double tol, int32_t max_iter, double* gamma, int64_t ldg, int32_t* iters, EStep& p) {
  const int rc = check_table(who, K, V, table, ldt);
  if (rc) return rc;
  const int rd = check_documents(who, indptr, indices, counts, counts_kind, B);
  if (rd) return rd;
  if (max_iter < 0 || max_iter > kMaxIter) {
    set_error("%s: max_iter=%d is outside [0, %d]", who, max_iter, kMaxIter);
    return GCNK_EARG;
  }
  p = EStep{};
  p.indptr = indptr;
  p.indices = indices;
  p.counts = counts;
  p.counts_kind = counts_kind;
  p.B = B;
  p.K = K;
  p.table = table;
  p.row_bytes = (uint32_t)(ldt * 8);
  p.table_bytes = (uint32_t)((int64_t)V * ldt * 8);
  p.alpha = alpha;
  p.tol = tol;
  p.max_iter = max_iter;
  p.gamma = gamma;
  p.ldth = ldg;
  p.iters = iters;
  return GCNK_OK;
}

// kDocs documents a workgroup, each wave with its own slice of the dynamic LDS
template <bool kFit>
static int launch_estep(const char* name, const EStep& p, void* stream) {
  const int lds_bytes = kDocs * wave_doubles(p.K) * (int)sizeof(double);
  const unsigned nblk = (unsigned)(((int64_t)p.B + kDocs - 1) / kDocs);
  return launch_big_lds<lda_estep_kernel<kFit>>(name, dim3(nblk), dim3(64 * kDocs), (size_t)lds_bytes, stream, p);
}

extern "C" int gcnk_lda_estep_f64(const int32_t* indptr, const int32_t* indices, const void* counts,
                                  int32_t counts_kind, int32_t B, int32_t V, int32_t K, const double* table,
                                  int64_t ldt, double alpha, double tol, int32_t max_iter, double* theta, int64_t ldth,
                                  double* gamma, int32_t* iters, float* x, int64_t ldx, float* a, int64_t lda,
                                  double threshold, void* stream) {
  const char* who = "gcnk_lda_estep_f64";
  EStep p;
  const int rc = estep_args(who, indptr, indices, counts, counts_kind, B, V, K, table, ldt, alpha, tol, max_iter, gamma,
                            ldth, iters, p);
  if (rc) return rc;
  if ((x == nullptr) != (a == nullptr)) {
    set_error("%s: x and a are given together or not at all", who);
    return GCNK_EARG;
  }
  if (!theta && !gamma && !iters && !x) {
    set_error("%s: no output requested (theta, gamma, iters, x and a are all null)", who);
    return GCNK_EARG;
  }
  if (((theta || gamma) && ldth < K) || (x && (ldx < K || lda < K))) {
    set_error("%s: an output's leading dimension is shorter than K=%d (ldth=%lld ldx=%lld lda=%lld)", who, K,
              (long long)ldth, (long long)ldx, (long long)lda);
    return GCNK_EARG;
  }
  p.theta = theta;
  p.x = x;
  p.ldx = ldx;
  p.a = a;
  p.lda = lda;
  p.threshold = threshold;
  return launch_estep<false>("lda_estep_kernel", p, stream);
}

extern "C" int32_t gcnk_lda_words_per_block(void) { return kWords; }

extern "C" int gcnk_lda_estep_fit_f64(const int32_t* indptr, const int32_t* indices, const void* counts,
                                      int32_t counts_kind, int32_t B, int32_t V, int32_t K, const double* table,
                                      int64_t ldt, double alpha, double tol, int32_t max_iter, const double* gamma0,
                                      int64_t ldg0, int64_t nnz, double* ratio, double* etheta, int64_t lde,
                                      double* gamma, int64_t ldg, int32_t* iters, void* stream) {
  const char* who = "gcnk_lda_estep_fit_f64";
  EStep p;
  const int rc = estep_args(who, indptr, indices, counts, counts_kind, B, V, K, table, ldt, alpha, tol, max_iter, gamma,
                            ldg, iters, p);
  if (rc) return rc;
  if (!gamma0 || !ratio || !etheta) {
    set_error("%s: gamma0, ratio and etheta must be non-null", who);
    return GCNK_EARG;
  }
  if (ldg0 < K || lde < K || (gamma && ldg < K)) {
    set_error("%s: a leading dimension is shorter than K=%d (ldg0=%lld lde=%lld ldg=%lld)", who, K, (long long)ldg0,
              (long long)lde, (long long)ldg);
    return GCNK_EARG;
  }
  if (nnz < 0) {
    set_error("%s: nnz=%lld is negative", who, (long long)nnz);
    return GCNK_EARG;
  }
  if (nnz * 8 >= (int64_t)kBufOob) {
    set_error("%s: %lld ratios are past the 32-bit offsets of their buffer resource", who, (long long)nnz);
    return GCNK_EUNSUP;
  }
  p.gamma0 = gamma0;
  p.ldg0 = ldg0;
  p.etheta = etheta;
  p.lde = lde;
  p.ratio = ratio;
  p.ratio_bytes = (uint32_t)(nnz * 8);
  return launch_estep<true>("lda_estep_fit_kernel", p, stream);
}

// the refusals both M-step entry points share, then the kernels' common arguments
static int mstep_args(const char* who, const int32_t* wptr, const int32_t* pos, const int32_t* doc, int64_t nnz,
                      const double* ratio, const double* etheta, int64_t lde, int32_t B, int32_t V, int32_t K,
                      const double* table, int64_t ldt, double eta, double* lambda, int64_t ldl, MStep& p) {
  const int rc = check_table(who, K, V, table, ldt);
  if (rc) return rc;
  if (B < 1 || !wptr || !pos || !doc || !ratio || !etheta || !lambda) {
    set_error("%s: needs B >= 1 and non-null wptr, pos, doc, ratio, etheta and lambda (B=%d)", who, B);
    return GCNK_EARG;
  }
  if (lde < K || ldl < V) {
    set_error("%s: lde=%lld < K=%d or ldl=%lld < V=%d", who, (long long)lde, K, (long long)ldl, V);
    return GCNK_EARG;
  }
  if (nnz < 0) {
    set_error("%s: nnz=%lld is negative", who, (long long)nnz);
    return GCNK_EARG;
  }
  if (nnz * 8 >= (int64_t)kBufOob || (int64_t)B * lde * 8 >= (int64_t)kBufOob) {
    set_error("%s: %lld ratios or an etheta of %lld bytes are past the 32-bit offsets of their buffer resources", who,
              (long long)nnz, (long long)((int64_t)B * lde * 8));
    return GCNK_EUNSUP;
  }
  p = MStep{};
  p.wptr = wptr;
  p.pos = pos;
  p.doc = doc;
  p.nnz = nnz;
  p.V = V;
  p.K = K;
  p.ratio = ratio;
  p.ratio_bytes = (uint32_t)(nnz * 8);
  p.etheta = etheta;
  p.et_row_bytes = (uint32_t)(lde * 8);
  p.et_bytes = (uint32_t)((int64_t)B * lde * 8);
  p.table = table;
  p.ldt = ldt;
  p.eta = eta;
  p.lambda = lambda;
  p.ldl = ldl;
  return GCNK_OK;
}

// kWords words a workgroup; K > 64 takes the instantiation with two topics a lane
template <auto kTwoTopics, auto kOneTopic, typename P>
static int launch_mstep(const char* name, const P& p, int32_t V, int32_t K, void* stream) {
  const unsigned nblk = (unsigned)(((int64_t)V + kWords - 1) / kWords);
  if (K > 64)
    hipLaunchKernelGGL(kTwoTopics, dim3(nblk), dim3(64 * kWords), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(kOneTopic, dim3(nblk), dim3(64 * kWords), 0, (hipStream_t)stream, p);
  return launch_check(name);
}

extern "C" int gcnk_lda_mstep_f64(const int32_t* wptr, const int32_t* pos, const int32_t* doc, int64_t nnz,
                                  const double* ratio, const double* etheta, int64_t lde, int32_t B, int32_t V,
                                  int32_t K, const double* table, int64_t ldt, double eta, double* lambda, int64_t ldl,
                                  void* stream) {
  MStep p;
  const int rc = mstep_args("gcnk_lda_mstep_f64", wptr, pos, doc, nnz, ratio, etheta, lde, B, V, K, table, ldt, eta,
                            lambda, ldl, p);
  if (rc) return rc;
  return launch_mstep<lda_mstep_kernel<true>, lda_mstep_kernel<false>>("lda_mstep_kernel", p, V, K, stream);
}

extern "C" int gcnk_lda_mstep_online_f64(const int32_t* wptr, const int32_t* pos, const int32_t* doc, int64_t nnz,
                                         int32_t doc_lo, int32_t doc_hi, const double* ratio, const double* etheta,
                                         int64_t lde, int32_t B, int32_t V, int32_t K, const double* table, int64_t ldt,
                                         double eta, double rho, double doc_ratio, double* lambda, int64_t ldl,
                                         void* stream) {
  const char* who = "gcnk_lda_mstep_online_f64";
  MStepOnline q{};
  const int rc = mstep_args(who, wptr, pos, doc, nnz, ratio, etheta, lde, B, V, K, table, ldt, eta, lambda, ldl, q.m);
  if (rc) return rc;
  if (doc_lo < 0 || doc_hi > B || doc_lo >= doc_hi) {
    set_error("%s: the minibatch [%d, %d) is empty or outside the B=%d documents", who, doc_lo, doc_hi, B);
    return GCNK_EARG;
  }
  if (!(rho > 0.0 && rho <= 1.0)) {   // (a NaN fails both)
    set_error("%s: rho=%g is outside (0, 1]", who, rho);
    return GCNK_EARG;
  }
  if (!finite_positive(doc_ratio)) {
    set_error("%s: doc_ratio=%g is not a finite positive number", who, doc_ratio);
    return GCNK_EARG;
  }
  q.doc_lo = doc_lo;
  q.doc_hi = doc_hi;
  q.rho = rho;
  q.doc_ratio = doc_ratio;
  return launch_mstep<lda_mstep_online_kernel<true>, lda_mstep_online_kernel<false>>("lda_mstep_online_kernel", q, V, K,
                                                                                      stream);
}

// ---- the variational bound's entry points
extern "C" int32_t gcnk_lda_bound_topic_chunk(void) { return kTopicThreads; }

extern "C" int gcnk_lda_bound_docs_f64(const int32_t* indptr, const int32_t* indices, const void* counts,
                                       int32_t counts_kind, int32_t B, int32_t V, int32_t K, const double* table,
                                       int64_t ldt, const double* gamma, int64_t ldg, double alpha, double* doc_bound,
                                       void* stream) {
  const char* who = "gcnk_lda_bound_docs_f64";
  const int rc = check_table(who, K, V, table, ldt);
  if (rc) return rc;
  const int rd = check_documents(who, indptr, indices, counts, counts_kind, B);
  if (rd) return rd;
  if (!gamma || !doc_bound || ldg < K) {
    set_error("%s: gamma and doc_bound must be non-null and ldg >= K (ldg=%lld K=%d)", who, (long long)ldg, K);
    return GCNK_EARG;
  }
  BoundDocs p{};
  p.indptr = indptr;
  p.indices = indices;
  p.counts = counts;
  p.counts_kind = counts_kind;
  p.B = B;
  p.K = K;
  p.table = table;
  p.row_bytes = (uint32_t)(ldt * 8);
  p.table_bytes = (uint32_t)((int64_t)V * ldt * 8);
  p.gamma = gamma;
  p.ldg = ldg;
  p.alpha = alpha;
  p.doc_bound = doc_bound;
  const int lds_bytes = kDocs * wave_doubles(K) * (int)sizeof(double);
  const unsigned nblk = (unsigned)(((int64_t)B + kDocs - 1) / kDocs);
  return launch_big_lds<lda_bound_docs_kernel>("lda_bound_docs_kernel", dim3(nblk), dim3(64 * kDocs), (size_t)lds_bytes,
                                               stream, p);
}

// K within the kernels' topics: GCNK_EARG below 1, GCNK_EUNSUP above kMaxTopics
static int check_topics(const char* who, int32_t K) {
  if (K < 1) {
    set_error("%s: needs K >= 1 (K=%d)", who, K);
    return GCNK_EARG;
  }
  if (K > kMaxTopics) {
    set_error("%s: K=%d topics, the kernels take at most %d", who, K, kMaxTopics);
    return GCNK_EUNSUP;
  }
  return GCNK_OK;
}

extern "C" int gcnk_lda_bound_topics_f64(const double* lambda, int64_t ldl, int32_t K, int32_t V, double eta,
                                         double* topic_bound, void* stream) {
  const char* who = "gcnk_lda_bound_topics_f64";
  const int rc = check_topics(who, K);
  if (rc) return rc;
  if (V < 1 || !lambda || !topic_bound || ldl < V) {
    set_error("%s: needs V >= 1, non-null lambda and topic_bound and ldl >= V (V=%d ldl=%lld)", who, V, (long long)ldl);
    return GCNK_EARG;
  }
  hipLaunchKernelGGL(lda_bound_topics_kernel, dim3((unsigned)K), dim3(kTopicThreads), 0, (hipStream_t)stream, lambda, ldl,
                     V, eta, topic_bound);
  return launch_check("lda_bound_topics_kernel");
}

extern "C" int gcnk_lda_bound_finish_f64(const double* doc_bound, int32_t B, const double* topic_bound, int32_t K,
                                         const int32_t* indptr, const void* counts, int32_t counts_kind,
                                         double doc_ratio, double* out, void* stream) {
  const char* who = "gcnk_lda_bound_finish_f64";
  const int rc = check_topics(who, K);
  if (rc) return rc;
  if (B < 1 || !doc_bound || !topic_bound || !indptr || !counts || !out) {
    set_error("%s: needs B >= 1 and non-null doc_bound, topic_bound, indptr, counts and out (B=%d)", who, B);
    return GCNK_EARG;
  }
  if (counts_kind < 0 || counts_kind > 2) {
    set_error("%s: counts_kind %d is not 0 (float64), 1 (int32) or 2 (int64)", who, counts_kind);
    return GCNK_EARG;
  }
  if (!finite_positive(doc_ratio)) {
    set_error("%s: doc_ratio=%g is not a finite positive number", who, doc_ratio);
    return GCNK_EARG;
  }
  hipLaunchKernelGGL(lda_bound_finish_kernel, dim3(1), dim3(kFinishThreads), 0, (hipStream_t)stream, doc_bound, B,
                     topic_bound, K, indptr, counts, counts_kind, doc_ratio, out);
  return launch_check("lda_bound_finish_kernel");
}
