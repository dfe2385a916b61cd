// The doc-topic graph on the device: (theta, topic similarities, two thresholds) -> the CSR of A-hat.
// Replaces the reference's host path from the topic model's output to the normalised adjacency:
//   build_graph.py:99-133   two Python loops over (document, topic) and (topic, topic) pairs into
//                           an nx.Graph, written as a text edge list (build_graph.py:199);
//   trainer.py:98-151       that text parsed back, max(A, A^T), utils.preprocess_adj with scipy.
// Semantics, the reference's:
//   * doc-topic edge (d, D + k) iff theta[d, k] >= doc_topic_threshold, compared in FLOAT64
//     (build_graph.py:106 `weight < threshold: continue`), weight float32(theta[d, k]) -- what the
//     edge list round-trips through trainer.py:105's dtype=np.float32;
//   * topic-topic edge (D + i, D + j), i < j, iff sim[i, j] > topic_topic_threshold (strict,
//     build_graph.py:124), weight float32(sim[i, j]); only the upper triangle is read and the
//     diagonal never is (build_graph.py:121-122);
//   * A-hat = D^-1/2 (A + I) D^-1/2 with normalize.hip's arithmetic: the identity's 1 and every
//     weight in float64, a row's sum taken SEQUENTIALLY in ascending column order with the
//     diagonal at its sorted place, d = rowsum^-0.5 with inf -> 0, value (d[r] a) d[c] rounded
//     to fp32 once.
// Two departures: every document and every topic is a node (a node without a kept edge is a row
// holding its diagonal alone, A-hat = 1; the reference's nx.Graph never creates such a node and
// numbers the later ones wrongly), and NaN / negative theta is not looked for (a NaN compares
// false and is dropped like any small weight).
//
// The structure is known in advance, so nothing is sorted and no atomic decides a position:
//   document row d   : d | D + k for the kept k, ascending
//   topic row D + k  : the kept documents, ascending | D + j for the kept j, with D + k in place
// A workgroup takes kChunk documents and stages their kept weights in LDS (a dropped entry is
// kDropped: a kept weight is >= +0 because the threshold is > 0).  A lane then owns a document
// (its row, its degree) and, in a second walk, a topic column of its wave's 64 documents: the
// column's kept entries per 64-document segment are counted in one launch, summed over the
// segments in order, and written in a second launch at segment base + running rank.
//   tg_count    segments' column counts, document row counts and degrees
//   tg_columns  the columns' exclusive sums over segments, topic-topic counts, topic row counts
//   (hipcub exclusive sum: the row pointer)
//   tg_fill     column indices and RAW fp32 weights of every row
//   tg_degree   a wave per topic row: its float64 sum in stored order
//   tg_scale    value <- (d[r] a) d[c], in place
#include "gcnk_common.h"

#include <hipcub/hipcub.hpp>

namespace gcnk {
namespace {

constexpr int kChunk = 256;       // documents per workgroup (topic_graph.DOCS_PER_BLOCK)
constexpr int kThreads = 256;
constexpr int kSegment = 64;      // documents per wave: the unit of the column counts
constexpr int kSegPerChunk = kChunk / kSegment;
constexpr int kMaxTopics = 128;   // two columns a lane; the tile of 256 x 129 floats fits the LDS
constexpr float kDropped = -1.0f;

static_assert(kThreads == kChunk && kSegment == 64, "a lane per document, a wave per segment");

// A row-major matrix of fp64 or fp32 elements, read as float64 (fp32 widens exactly).
struct Mat {
  const void* p;
  int64_t ld;
  int32_t f32;
  __device__ __forceinline__ double at(int64_t r, int64_t c) const {
    const int64_t i = r * ld + c;
    return f32 ? (double)static_cast<const float*>(p)[i] : static_cast<const double*>(p)[i];
  }
};

// tile[r * stride + k] = float32(theta[d0 + r, k]) where kept, else kDropped; returns the rows staged
__device__ __forceinline__ int stage_tile(const Mat& theta, int32_t D, int32_t K, int32_t d0, double thr, float* tile,
                                          int stride) {
  const int rows = min(kChunk, D - d0);
  for (int i = threadIdx.x; i < rows * K; i += kThreads) {
    const int r = i / K, k = i - r * K;
    const double t = theta.at(d0 + r, k);
    tile[r * stride + k] = t >= thr ? (float)t : kDropped;
  }
  __syncthreads();
  return rows;
}

__global__ void __launch_bounds__(kThreads)
tg_count_kernel(Mat theta, int32_t D, int32_t K, double thr, int32_t* __restrict__ counts, double* __restrict__ d,
                int32_t* __restrict__ segcnt) {
  extern __shared__ float tile[];
  const int stride = K | 1;
  const int32_t d0 = (int32_t)blockIdx.x * kChunk;
  const int rows = stage_tile(theta, D, K, d0, thr, tile, stride);
  const int t = threadIdx.x;
  if (t < rows) {   // the document's row: its diagonal, then the kept topics in order
    double s = 1.0;
    int32_t n = 1;
    for (int k = 0; k < K; ++k) {
      const float w = tile[t * stride + k];
      if (w >= 0.0f) {
        s += (double)w;
        ++n;
      }
    }
    counts[d0 + t] = n;
    d[d0 + t] = ahat_inv_sqrt_degree(s);
  }
  const int wv = t >> 6, lane = t & 63;
  const int r0 = wv * kSegment, r1 = min(rows, r0 + kSegment);
  for (int k = lane; k < K; k += 64) {
    int32_t n = 0;
    for (int r = r0; r < r1; ++r) n += tile[r * stride + k] >= 0.0f ? 1 : 0;
    segcnt[((int64_t)blockIdx.x * kSegPerChunk + wv) * K + k] = n;
  }
}

__device__ __forceinline__ bool topic_edge(const Mat& sim, int i, int j, double thr) {
  return sim.at(i < j ? i : j, i < j ? j : i) > thr;
}

// One workgroup, a thread per topic: segcnt becomes each segment's base within the column.
__global__ void __launch_bounds__(kMaxTopics)
tg_columns_kernel(Mat sim, int32_t D, int32_t K, double thr, int32_t nseg, int32_t* __restrict__ segcnt,
                  int32_t* __restrict__ doccnt, int32_t* __restrict__ counts, int32_t* __restrict__ edges) {
  __shared__ int32_t s_doc[kMaxTopics], s_top[kMaxTopics];
  const int k = threadIdx.x;
  int32_t docs = 0, tops = 0;
  if (k < K) {
    // 16 segments' counts loaded before the first base is stored: one load round trip per 16
    // segments (a store between two loads of the same array keeps the second load behind it)
    for (int32_t s0 = 0; s0 < nseg; s0 += 16) {
      int32_t c[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) c[u] = s0 + u < nseg ? segcnt[(int64_t)(s0 + u) * K + k] : 0;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        if (s0 + u < nseg) segcnt[(int64_t)(s0 + u) * K + k] = docs;
        docs += c[u];
      }
    }
    if (sim.p)
      for (int j = 0; j < K; ++j)
        if (j != k && topic_edge(sim, k, j, thr)) ++tops;
    doccnt[k] = docs;
    counts[D + k] = docs + 1 + tops;
  }
  s_doc[k] = docs;
  s_top[k] = tops;
  __syncthreads();
  if (k != 0) return;
  counts[D + K] = 0;   // the scan's last element: rowptr[N] = total
  if (!edges) return;
  int32_t nd = 0, nt = 0;
  for (int j = 0; j < K; ++j) {
    nd += s_doc[j];
    nt += s_top[j];
  }
  edges[0] = nd;
  edges[1] = nt / 2;
}

// Workgroups 0 .. nchunk - 1: the document rows and the document part of the topic rows;
// the workgroups after them: the topic block of the topic rows, a wave per row.
__global__ void __launch_bounds__(kThreads)
tg_fill_kernel(Mat theta, Mat sim, int32_t D, int32_t K, double thr_doc, double thr_top, int32_t nchunk,
               const int32_t* __restrict__ rowptr, const int32_t* __restrict__ segbase,
               const int32_t* __restrict__ doccnt, int32_t* __restrict__ colind, float* __restrict__ val) {
  extern __shared__ float tile[];
  const int t = threadIdx.x;
  if ((int32_t)blockIdx.x >= nchunk) {   // a wave per topic row, a lane per column: the rank from a ballot
    const int row = ((int32_t)blockIdx.x - nchunk) * (kThreads / 64) + (t >> 6), lane = t & 63;
    if (row >= K) return;
    int32_t o = rowptr[D + row] + doccnt[row];
    for (int j = lane; j < kMaxTopics; j += 64) {
      bool keep = false;
      float w = 1.0f;
      if (j == row) {
        keep = true;
      } else if (j < K && sim.p) {
        const double s = sim.at(row < j ? row : j, row < j ? j : row);
        keep = s > thr_top;
        w = (float)s;
      }
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int32_t at = o + __popcll(m & ((1ull << lane) - 1ull));
        colind[at] = D + j;
        val[at] = w;
      }
      o += __popcll(m);
    }
    return;
  }
  const int stride = K | 1;
  const int32_t d0 = (int32_t)blockIdx.x * kChunk;
  const int rows = stage_tile(theta, D, K, d0, thr_doc, tile, stride);
  if (t < rows) {
    int32_t o = rowptr[d0 + t];
    colind[o] = d0 + t;
    val[o++] = 1.0f;
    for (int k = 0; k < K; ++k) {
      const float w = tile[t * stride + k];
      if (w >= 0.0f) {
        colind[o] = D + k;
        val[o++] = w;
      }
    }
  }
  const int wv = t >> 6, lane = t & 63;
  const int r0 = wv * kSegment, r1 = min(rows, r0 + kSegment);
  for (int k = lane; k < K; k += 64) {
    int32_t o = rowptr[D + k] + segbase[((int64_t)blockIdx.x * kSegPerChunk + wv) * K + k];
    for (int r = r0; r < r1; ++r) {
      const float w = tile[r * stride + k];
      if (w >= 0.0f) {
        colind[o] = d0 + r;
        val[o++] = w;
      }
    }
  }
}

// A wave per topic row: 64 raw weights a load, every lane adding them one after the other in
// stored order (a lane past the row's end holds +0, which leaves the sum as it is).
__global__ void __launch_bounds__(64)
tg_degree_kernel(int32_t D, const int32_t* __restrict__ rowptr, const float* __restrict__ val,
                 double* __restrict__ d) {
  const int32_t row = D + (int32_t)blockIdx.x;
  const int32_t b = rowptr[row], e = rowptr[row + 1];
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int32_t base = b; base < e; base += 4 * 64) {   // four loads in flight ahead of the 256 adds
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = base + 64 * u + lane < e ? val[base + 64 * u + lane] : 0.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (base + 64 * u >= e) break;
#pragma unroll
      for (int j = 0; j < 64; ++j) s += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[u]), j));
    }
  }
  if (lane == 0) d[row] = ahat_inv_sqrt_degree(s);
}

// Workgroups 0 .. ndocblk - 1: a thread per document row; then a workgroup per topic row.
__global__ void __launch_bounds__(kThreads)
tg_scale_kernel(int32_t D, int32_t ndocblk, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                const double* __restrict__ d, float* __restrict__ val) {
  if ((int32_t)blockIdx.x < ndocblk) {
    const int32_t r = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;
    if (r >= D) return;
    const double dr = d[r];
    for (int32_t i = rowptr[r], e = rowptr[r + 1]; i < e; ++i) val[i] = ahat_value(dr, (double)val[i], d[colind[i]]);
    return;
  }
  const int32_t r = D + ((int32_t)blockIdx.x - ndocblk);
  const double dr = d[r];
  for (int32_t i = rowptr[r] + (int32_t)threadIdx.x, e = rowptr[r + 1]; i < e; i += kThreads)
    val[i] = ahat_value(dr, (double)val[i], d[colind[i]]);
}

// A thread per pair i <= j: the dot product and both squared norms in one ascending walk.
__global__ void __launch_bounds__(kThreads)
cosine_kernel(Mat emb, int32_t K, int32_t dim, double* __restrict__ sim, int64_t lds) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (int64_t)K * K) return;
  const int32_t i = (int32_t)(idx / K), j = (int32_t)(idx - (int64_t)i * K);
  if (j < i) return;
  double dot = 0.0, ni = 0.0, nj = 0.0;
  for (int32_t t = 0; t < dim; ++t) {
    const double a = emb.at(i, t), b = emb.at(j, t);
    dot = fma(a, b, dot);
    ni = fma(a, a, ni);
    nj = fma(b, b, nj);
  }
  const double den = sqrt(ni) * sqrt(nj);
  const double s = den > 0.0 ? dot / den : 0.0;   // a zero row is similar to nothing
  sim[(int64_t)i * lds + j] = s;
  sim[(int64_t)j * lds + i] = s;
}

size_t scan_temp_bytes(int32_t n) {
  size_t bytes = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int32_t*)nullptr, (int32_t*)nullptr, n + 1) !=
      hipSuccess)
    return 0;
  return bytes;
}

inline int64_t up256(int64_t b) { return (b + 255) & ~255LL; }

struct Layout {
  int64_t d, counts, segcnt, doccnt, scan, total;
  int32_t nchunk, nseg;
};

Layout layout(int32_t D, int32_t K) {
  Layout l;
  const int64_t N = (int64_t)D + K;
  l.nchunk = (int32_t)(((int64_t)D + kChunk - 1) / kChunk);
  l.nseg = l.nchunk * kSegPerChunk;
  l.d = 0;
  l.counts = l.d + up256(N * 8);
  l.segcnt = l.counts + up256((N + 1) * 4);
  l.doccnt = l.segcnt + up256((int64_t)l.nseg * K * 4);
  l.scan = l.doccnt + up256((int64_t)K * 4);
  l.total = l.scan + (int64_t)scan_temp_bytes((int32_t)N);
  return l;
}

// D, K in range and the int32 CSR large enough for every entry the inputs could keep
int check_shape(const char* who, int32_t D, int32_t K, int32_t has_sim, int64_t* bound) {
  if (D < 1 || K < 1) {
    set_error("%s: needs D >= 1 and K >= 1 (D=%d K=%d)", who, D, K);
    return GCNK_EARG;
  }
  if (K > kMaxTopics) {
    set_error("%s: K=%d topics, the kernels take at most %d", who, K, kMaxTopics);
    return GCNK_EUNSUP;
  }
  const int64_t N = (int64_t)D + K;
  const int64_t nnz = N + 2 * (int64_t)D * K + (has_sim ? (int64_t)K * (K - 1) : 0);
  if (N + nnz >= (int64_t)INT32_MAX) {
    set_error("%s: N + nnz bound = %lld exceeds int32 CSR (D=%d K=%d)", who, (long long)(N + nnz), D, K);
    return GCNK_EUNSUP;
  }
  *bound = nnz;
  return GCNK_OK;
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int32_t gcnk_topic_graph_chunk(void) { return kChunk; }

extern "C" int32_t gcnk_topic_graph_max_topics(void) { return kMaxTopics; }

extern "C" int64_t gcnk_topic_graph_nnz_bound(int32_t D, int32_t K, int32_t has_sim) {
  int64_t bound = 0;
  const int rc = check_shape("gcnk_topic_graph_nnz_bound", D, K, has_sim, &bound);
  return rc ? rc : bound;
}

extern "C" int64_t gcnk_topic_graph_workspace_bytes(int32_t D, int32_t K) {
  int64_t bound = 0;
  const int rc = check_shape("gcnk_topic_graph_workspace_bytes", D, K, 1, &bound);
  return rc ? rc : layout(D, K).total;
}

extern "C" int gcnk_topic_graph_build(const void* theta, int32_t theta_f32, int64_t ldt, const void* sim,
                                      int32_t sim_f32, int64_t lds, int32_t D, int32_t K,
                                      double doc_topic_threshold, double topic_topic_threshold, int32_t* rowptr,
                                      int32_t* colind, float* val, int64_t capacity, int32_t* edges, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  const char* who = "gcnk_topic_graph_build";
  int64_t bound = 0;
  const int rc0 = check_shape(who, D, K, sim != nullptr, &bound);
  if (rc0) return rc0;
  if (!(doc_topic_threshold > 0.0) || !(topic_topic_threshold > 0.0)) {
    set_error("%s: thresholds must be > 0 (doc-topic %g, topic-topic %g): a threshold of 0 keeps explicit zeros", who,
              doc_topic_threshold, topic_topic_threshold);
    return GCNK_EARG;
  }
  if (!theta || !rowptr || !colind || !val) {
    set_error("%s: null theta or output pointer", who);
    return GCNK_EARG;
  }
  if ((theta_f32 | sim_f32) & ~1) {
    set_error("%s: element type flags must be 0 (fp64) or 1 (fp32)", who);
    return GCNK_EARG;
  }
  if (ldt < K || (sim && lds < K)) {
    set_error("%s: leading dimension shorter than K=%d (theta %lld, sim %lld)", who, K, (long long)ldt,
              (long long)lds);
    return GCNK_EARG;
  }
  if (capacity < bound) {
    set_error("%s: colind / val hold %lld entries, the inputs may keep %lld (gcnk_topic_graph_nnz_bound)", who,
              (long long)capacity, (long long)bound);
    return GCNK_EARG;
  }
  if (!workspace) {
    set_error("%s: null workspace", who);
    return GCNK_EARG;
  }
  const Layout l = layout(D, K);
  if (workspace_bytes < l.total) {
    set_error("%s: needs %lld B of workspace, got %lld", who, (long long)l.total, (long long)workspace_bytes);
    return GCNK_EARG;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* d = (double*)(ws + l.d);
  int32_t* counts = (int32_t*)(ws + l.counts);
  int32_t* segcnt = (int32_t*)(ws + l.segcnt);
  int32_t* doccnt = (int32_t*)(ws + l.doccnt);
  const int32_t N = D + K;
  const Mat th{theta, ldt, theta_f32}, sm{sim, lds, sim_f32};
  const int lds_b = kChunk * (K | 1) * (int)sizeof(float);
  int rc = launch_big_lds<tg_count_kernel>("tg_count_kernel", dim3((unsigned)l.nchunk), dim3(kThreads), (size_t)lds_b,
                                           stream, th, D, K, doc_topic_threshold, counts, d, segcnt);
  if (rc) return rc;
  hipLaunchKernelGGL(tg_columns_kernel, dim3(1), dim3(kMaxTopics), 0, s, sm, D, K, topic_topic_threshold, l.nseg,
                     segcnt, doccnt, counts, edges);
  rc = launch_check("tg_columns_kernel");
  if (rc) return rc;
  size_t tmp_bytes = (size_t)(l.total - l.scan);
  rc = hip_check(hipcub::DeviceScan::ExclusiveSum(ws + l.scan, tmp_bytes, counts, rowptr, N + 1, s),
                 "topic graph scan");
  if (rc) return rc;
  const int32_t ntopblk = (K + kThreads / 64 - 1) / (kThreads / 64);
  rc = launch_big_lds<tg_fill_kernel>("tg_fill_kernel", dim3((unsigned)(l.nchunk + ntopblk)), dim3(kThreads),
                                      (size_t)lds_b, stream, th, sm, D, K, doc_topic_threshold, topic_topic_threshold,
                                      l.nchunk, rowptr, segcnt, doccnt, colind, val);
  if (rc) return rc;
  hipLaunchKernelGGL(tg_degree_kernel, dim3((unsigned)K), dim3(64), 0, s, D, rowptr, val, d);
  rc = launch_check("tg_degree_kernel");
  if (rc) return rc;
  const int32_t ndocblk = (D + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(tg_scale_kernel, dim3((unsigned)(ndocblk + K)), dim3(kThreads), 0, s, D, ndocblk, rowptr, colind,
                     d, val);
  return launch_check("tg_scale_kernel");
}

extern "C" int gcnk_topic_cosine_f64(const void* emb, int32_t emb_f32, int64_t lde, int32_t K, int32_t dim,
                                     double* sim, int64_t lds, void* stream) {
  const char* who = "gcnk_topic_cosine_f64";
  if (K < 1 || dim < 1 || !emb || !sim || lde < dim || lds < K || (emb_f32 & ~1)) {
    set_error("%s: bad argument (K=%d dim=%d lde=%lld lds=%lld)", who, K, dim, (long long)lde, (long long)lds);
    return GCNK_EARG;
  }
  if ((int64_t)K * K >= (int64_t)INT32_MAX) {
    set_error("%s: K=%d rows, K * K exceeds int32", who, K);
    return GCNK_EUNSUP;
  }
  const int64_t nblk = ((int64_t)K * K + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(cosine_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, (hipStream_t)stream,
                     Mat{emb, lde, emb_f32}, K, dim, sim, lds);
  return launch_check("cosine_kernel");
}
