// Held-graph scoring for gfx950: the logits of documents that are NOT in the
// training graph, as the rows they would have in the transductive forward
// (GCN.forward, layer.py:164-190) with the hub (topic) nodes' state held as the
// training graph left it.
//
// Structure used (the one factor.py checks): a document row of A-hat holds its
// diagonal and hub columns only, and a document row of X is supported on the
// columns k0 .. k0 + Kc.  So with S_T = X[hubs] W1 and S2_T = (H1 W2)[hubs] of
// the training graph, document d with features x[d, :Kc] and raw hub edge
// weights a[d, :H] has
//   deg    = 1 + sum_j a[d, j]                (float64, j ascending)
//   dd     = deg^-1/2,  c_self = fp32(dd dd),  c_j = fp32((dd a[d, j]) dh[j])
//   z[n]   = c_self sum_k x[d, k] W1[k0 + k, n] + sum_j c_j S_T[j, n] + b1[n]
//   out[p] = c_self sum_n relu(z[n]) W2[n, p] + sum_j c_j S2_T[j, p] + b2[p]
// -- the coefficients are A-hat's arithmetic (ahat_value: float64, rounded to
// fp32 once), dh[j] = D^-1/2 of hub j.  No document depends on another: one
// launch, no hand-off between workgroups, no atomics, bitwise reproducible.
//
// One workgroup = 32 documents as one block of hub_block.h (8 waves: 2 row
// strips x 4 quarters of the F columns):
//   0. every operand in one round of loads: the block's x / a / dh values into
//      registers, B = [W1[k0 : k0 + Kc]; S_T] into LDS by 16-B DMA (rows of F
//      floats; in chunks of rows where it exceeds the LDS left over: Kc + H = 256
//      at F = 256 is 256 KB), the wave's W2, S2_T, b1, b2 fragments into
//      registers; deg and the coefficients while the DMA is in flight, the
//      operand row [c_self x | c | 0] into LDS;
//   1. Z = [c_self x | c] B on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains),
//      K = Kc + H;
//   2. + b1, ReLU in registers (a NaN stays a NaN, as th.relu keeps it), the
//      tile through LDS to the A layout;
//   3. s2 = h W2 and e = c S2_T on MFMA (K split over the four quarters, summed
//      in a fixed order), out = c_self s2 + e + b2, the argmax per row from LDS.
// Rows past B, columns past F / P and a missing b1 / b2 go through buffer
// resources (device_mem.h): no compares in the loops.
#include "hub_block.h"

#include <algorithm>
#include <type_traits>

namespace gcnk {
namespace {

constexpr int kMaxKc = 128, kMaxHubs = 128;
constexpr int kOutLd = kHubProjMax + 1;   // s_out row stride
constexpr int kLdsFloats = 160 * 1024 / 4;
// Columns of an operand row [c_self x (Kc) | c (H) | 0 ...] that the kernel writes: phase 3 reads the c
// columns up to Kc + 16 KHQ, phase 1 every column up to Kc + H rounded up to 4 -- which lies up to 3
// columns past Kc + 16 KHQ where H = 16 KHQ and Kc % 4 != 0 (and K % 4 != 0 in general)
__host__ __device__ constexpr int operand_cols(int kc, int h, int khq) {
  return kc + 16 * khq > ((kc + h + 3) & ~3) ? kc + 16 * khq : ((kc + h + 3) & ~3);
}

struct ScoreArgs {
  int32_t B, F, Kc, H, P, k0;
  const float* x; int64_t ldx;      // [B x Kc]
  const float* a; int64_t lda;      // [B x H]
  const float* W1; int64_t ldw1;    // rows k0 .. k0 + Kc - 1 are read
  const float* S; int64_t lds;      // S_T [H x F]
  const float* W2; int64_t ldw2;    // [F x P]
  const float* S2; int64_t lds2;    // S2_T [H x P]
  const double* dh;                 // [H]
  const float* b1; const float* b2; // nullable
  float* out; int64_t ldo;          // [B x P]
  int32_t* labels;                  // nullable
  int32_t ch;                       // rows of B staged at a time (a multiple of 4)
  int32_t kpa;                      // s_A row stride (floats)
  int32_t r1;                       // floats of the region s_B / s_Z share
};

// NaN-keeping ReLU: th.relu(NaN) is NaN (fmaxf would return 0)
__device__ __forceinline__ float relu_keep_nan(float v) { return !(v <= 0.f) ? v : 0.f; }

// NTQ: 16-column tiles of F per wave (F <= 64 NTQ); NP: n-tiles of P; KHQ: k-steps of
// the hub sum c S2_T per quarter (H <= 16 KHQ)
template <int NTQ, int NP, int KHQ>
__global__ void __launch_bounds__(kHubThreads)
score_docs_kernel(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int strip = wv & 1, quarter = wv >> 1;
  const int c = lane & 15, q = lane >> 4;
  const int F = a.F, Q = F / 4, Kc = a.Kc, H = a.H, P = a.P;
  const int K = Kc + H, Kp = (K + 3) & ~3;
  constexpr int Fp = 64 * NTQ, Fz = hub_z_stride(NTQ);
  constexpr int kq = Fp / 16;                 // k-steps of h W2 per quarter
  const int kpa = a.kpa;
  const int64_t d0 = (int64_t)blockIdx.x * kHubRows;
  const int rows_here = (int)min<int64_t>(kHubRows, a.B - d0);   // >= 1
  // LDS: region1 = s_B [<= ch][F] + hub_bpad zeros (phase 1), then s_Z [kHubRows][Fz]
  //      | s_A [kHubRows][kpa]: the operand rows [c_self x (Kc) | c (H) | 0 .. operand_cols], kpa = 4 (mod 64)
  //      | s_red (two projected sums) | s_out [kHubRows][kOutLd] | s_cs [kHubRows] | s_dd [kHubRows] (double)
  float* s_B = smem;
  float* s_Z = smem;
  float* s_A = smem + a.r1;
  float* s_red = s_A + kHubRows * kpa;
  float* s_out = s_red + hub_red_floats(NP, 2);
  float* s_cs = s_out + kHubRows * kOutLd;
  double* s_dd = reinterpret_cast<double*>(s_cs + kHubRows);

  // ---- 0. loads.  First the block's x / a / dh values (the coefficients wait for
  //      these only), 16 threads per document, thread c16 the columns c16 + 16 i.
  //      Resources over the block's own rows: a row past B lies past them and
  //      reads 0 -- a document without features or edges, whose results the
  //      output resources drop.
  const int r = tid >> 4, c16 = tid & 15;
  float xv[kMaxKc / 16], av[KHQ];
  double dv[KHQ];
  {
    const __amdgpu_buffer_rsrc_t rx = buffer_rsrc(a.x + d0 * a.ldx, (uint32_t)(((rows_here - 1) * a.ldx + Kc) * 4));
    const __amdgpu_buffer_rsrc_t ra = buffer_rsrc(a.a + d0 * a.lda, (uint32_t)(((rows_here - 1) * a.lda + H) * 4));
    const __amdgpu_buffer_rsrc_t rd = buffer_rsrc(a.dh, (uint32_t)(H * 8));
    const uint32_t xo = (uint32_t)(r * a.ldx) * 4u, ao = (uint32_t)(r * a.lda) * 4u;
#pragma unroll
    for (int i = 0; i < KHQ; ++i) {
      const int j = c16 + 16 * i;
      av[i] = buf_load_f32(ra, j < H ? ao + 4u * j : kBufOob);
    }
#pragma unroll
    for (int i = 0; i < kMaxKc / 16; ++i) {
      const int k = c16 + 16 * i;
      xv[i] = buf_load_f32(rx, k < Kc ? xo + 4u * k : kBufOob);
    }
#pragma unroll
    for (int i = 0; i < KHQ; ++i)   // (a hub past H: offset past the resource, 0)
      dv[i] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rd, 8 * (c16 + 16 * i), 0, 0));
  }
  // B's rows g0 .. g0 + rows - 1 (g < Kc: W1[k0 + g], else S_T[g - Kc]) into s_B
  // by 16-B DMA, and the zeros behind them: the rows up to a multiple of 4 (k past
  // K: the operand rows are 0 there, and 0 x a stale NaN is a NaN) and the pad
  auto stage = [&](int g0) __attribute__((always_inline)) {
    const int rows4 = min(a.ch, Kp - g0), rows = min(rows4, K - g0);
    for (int e = rows * F + tid; e < rows4 * F + hub_bpad(F, NTQ); e += kHubThreads) s_B[e] = 0.f;
    const int n4 = rows * Q;
    for (int e0 = wv * 64; e0 < n4; e0 += kHubThreads) {
      const int e = e0 + lane;
      if (e < n4) {
        const int rr = e / Q, g = g0 + rr, q4 = 4 * (e - rr * Q);
        const float* src = g < Kc ? a.W1 + (int64_t)(a.k0 + g) * a.ldw1 + q4 : a.S + (int64_t)(g - Kc) * a.lds + q4;
        lds_dma16(src, s_B + 4 * e0);
      }
    }
  };
  stage(0);
  // Phase 3's B fragments of W2 (rows past F read 0) and S2_T (rows past H),
  // b1 / b2 the same way (a missing one: the zero-byte resource).
  float bw[NP][kq], bs[NP][KHQ], b1v[NTQ], b2v[NP];
  const HubDeal deal = hub_deal(strip, quarter, lane, F, NTQ);   // phase 1's tiles
  const int c0 = deal.c0;
  {
    const __amdgpu_buffer_rsrc_t rw = buffer_rsrc(a.W2, (uint32_t)(((F - 1) * a.ldw2 + P) * 4));
    const __amdgpu_buffer_rsrc_t rs = buffer_rsrc(a.S2, (uint32_t)(((H - 1) * a.lds2 + P) * 4));
    const __amdgpu_buffer_rsrc_t rb1 = buffer_rsrc_if(a.b1 != nullptr, a.b1 ? a.b1 : a.W1, (uint32_t)(F * 4));
    const __amdgpu_buffer_rsrc_t rb2 = buffer_rsrc_if(a.b2 != nullptr, a.b2 ? a.b2 : a.W1, (uint32_t)(P * 4));
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int col = 16 * t + c;
      hub_proj_frags(bw[t], rw, 4 * quarter * kq + q, (int)a.ldw2, col, P);
      hub_proj_frags(bs[t], rs, 4 * quarter * KHQ + q, (int)a.lds2, col, P);
      b2v[t] = buf_load_f32(rb2, col < P ? 4u * col : kBufOob);
    }
#pragma unroll
    for (int i = 0; i < NTQ; ++i) b1v[i] = buf_load_f32(rb1, 4u * (c0 + kHubTileStep * i));   // (a column past F: past the resource)
  }
  // the raw edge weights into the operand row's c columns (0 from H to 16 KHQ) and
  // zeros into the columns phase 1 reads past them (at most 3: operand_cols),
  // then deg = 1 + sum_j a[d, j] by one thread per document, j ascending
  float* arow = s_A + r * kpa;
#pragma unroll
  for (int i = 0; i < KHQ; ++i) arow[Kc + c16 + 16 * i] = av[i];
  if (Kc + 16 * KHQ + c16 < operand_cols(Kc, H, KHQ)) arow[Kc + 16 * KHQ + c16] = 0.f;
  __syncthreads();
  if (c16 == 0) {
    double s = 0.0;
    for (int j = 0; j < H; ++j) s += (double)arow[Kc + j];
    s_dd[r] = pow(1.0 + s, -0.5);   // (deg >= 1 for the non-negative weights of the contract: no inf -> 0 step)
  }
  __syncthreads();
  {
    const double dd = s_dd[r];
    const float cs = ahat_value(dd, 1.0, dd);
#pragma unroll
    for (int i = 0; i < KHQ; ++i) arow[Kc + c16 + 16 * i] = ahat_value(dd, (double)av[i], dv[i]);
#pragma unroll
    for (int i = 0; i < kMaxKc / 16; ++i)
      if (c16 + 16 * i < Kc) arow[c16 + 16 * i] = cs * xv[i];
    if (c16 == 0) s_cs[r] = cs;
  }

  // ---- 1. Z = [c_self x | c] B for this wave's strip and its tiles of F
  f32x4 acc[NTQ];
#pragma unroll
  for (int i = 0; i < NTQ; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const int nt = deal.nt;
    const float* sa = s_A + (16 * strip + c) * kpa + q;
    for (int g0 = 0; g0 < Kp; g0 += a.ch) {
      if (g0 > 0) {
        __syncthreads();   // the previous chunk's readers
        stage(g0);
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's DMA has landed
      __syncthreads();
      const int ns = min(a.ch, Kp - g0) >> 2;
      const float* sb = s_B + q * F + c0;
      auto run = [&](auto ntc) __attribute__((always_inline)) {
        constexpr int NT = decltype(ntc)::value;
#pragma unroll 2
        for (int s = 0; s < ns; ++s) {
          const float af = sa[g0 + 4 * s];
          const float* br = sb + 4 * s * F;
          float bf[NT];
#pragma unroll
          for (int i = 0; i < NT; ++i) bf[i] = br[kHubTileStep * i];
#pragma unroll
          for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[i], acc[i], 0, 0, 0);
        }
      };
      if (nt == NTQ) {
        run(std::integral_constant<int, NTQ>{});
      } else if (nt == NTQ - 1) {
        run(std::integral_constant<int, NTQ - 1>{});
      } else {   // narrow F: fewer real tiles, uniform tests
        for (int s = 0; s < ns; ++s) {
          const float af = sa[g0 + 4 * s];
          const float* br = sb + 4 * s * F;
#pragma unroll
          for (int i = 0; i < NTQ - 2; ++i)
            if (i < nt) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, br[kHubTileStep * i], acc[i], 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();  // s_B is overwritten by s_Z below

  // ---- 2. + b1, ReLU in registers; C/D map of the 16x16 f32 MFMA: reg rr -> row
  //      (lane >> 4) * 4 + rr, col lane & 15.  Columns past F are stored as 0:
  //      they meet W2's rows past F, which read 0.
#pragma unroll
  for (int i = 0; i < NTQ; ++i) {
    const bool live = c0 + kHubTileStep * i < F;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      s_Z[(16 * strip + 4 * q + rr) * Fz + c0 + kHubTileStep * i] = live ? relu_keep_nan(acc[i][rr] + b1v[i]) : 0.f;
  }
  __syncthreads();

  // ---- 3. s2 = h W2 (K = F) and e = c S2_T (K = H) on MFMA: strip x quarter of
  //      each sum, NP n-tiles of P, quarters added in order
  f32x4 pc[NP], pe[NP];
  {
    float hv[kq], cv[KHQ];
    const float* zr = s_Z + (16 * strip + c) * Fz + 4 * quarter * kq + q;
    const float* cr = s_A + (16 * strip + c) * kpa + Kc + 4 * quarter * KHQ + q;
#pragma unroll
    for (int j = 0; j < kq; ++j) hv[j] = zr[4 * j];
#pragma unroll
    for (int j = 0; j < KHQ; ++j) cv[j] = cr[4 * j];
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      f32x4 p0 = f32x4{0.f, 0.f, 0.f, 0.f}, p1 = p0, e0 = p0;
#pragma unroll
      for (int j = 0; j < kq; j += 2) {
        p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[j], bw[t][j], p0, 0, 0, 0);
        p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[j + 1], bw[t][j + 1], p1, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < KHQ; ++j) e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[j], bs[t][j], e0, 0, 0, 0);
      pc[t] = p0 + p1;
      pe[t] = e0;
    }
  }
  auto red = [&](int t, int kind, int qq) __attribute__((always_inline)) {
    return reinterpret_cast<f32x4*>(s_red + (((((t * 2 + kind) * 3 + qq) * 2 + strip) * 64) + lane) * 4);
  };
  if (quarter > 0)
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      *red(t, 0, quarter - 1) = pc[t];
      *red(t, 1, quarter - 1) = pe[t];
    }
  __syncthreads();
  if (quarter == 0) {
    const __amdgpu_buffer_rsrc_t ro = buffer_rsrc(a.out + d0 * a.ldo, (uint32_t)(((rows_here - 1) * a.ldo + P) * 4));
    const f32x4 cs4 = *reinterpret_cast<const f32x4*>(s_cs + 16 * strip + 4 * q);
#pragma unroll
    for (int t = 0; t < NP; ++t) {
#pragma unroll
      for (int qq = 0; qq < 3; ++qq) {
        pc[t] += *red(t, 0, qq);
        pe[t] += *red(t, 1, qq);
      }
      const int p = 16 * t + c;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = 16 * strip + 4 * q + rr;
        const float o = fmaf(cs4[rr], pc[t][rr], pe[t][rr]) + b2v[t];
        buf_store_f32(o, ro, p < P ? (uint32_t)((row * a.ldo + p) * 4) : kBufOob);   // (a row past B: past the resource)
        s_out[row * kOutLd + p] = o;
      }
    }
  }
  if (!a.labels) return;   // (uniform)
  __syncthreads();
  // the label (label_step)
  if (tid < rows_here) {
    const float* o = s_out + tid * kOutLd;
    int best = 0;
    float bv = o[0];
    for (int p = 1; p < P; ++p) {
      label_step(bv, best, o[p], p);
    }
    a.labels[d0 + tid] = best;
  }
}

// What a shape launches: the one place these rules live.  Returns 0, 1 for bad
// sizes, or 3 where the shape is outside the kernel's range.
struct ScoreRoute {
  int ntq, np, khq, ch, kpa, r1, wd;
  int64_t lds_bytes;
};

int score_route(int32_t F, int32_t Kc, int32_t H, int32_t P, ScoreRoute& rt) {
  rt = ScoreRoute{};
  if (F <= 0 || Kc <= 0 || H <= 0 || P <= 0) return 1;
  if (F % 4 || F > 256 || Kc > kMaxKc || H > kMaxHubs || P > kHubProjMax) return 3;
  rt.ntq = hub_pick_ntq(F); rt.np = hub_pick_np(P); rt.khq = H <= 64 ? 4 : 8;
  rt.wd = operand_cols(Kc, H, rt.khq);             // operand row: c_self x | c | zeros
  rt.kpa = 64 * ((rt.wd - 4 + 63) / 64) + 4;       // = 4 (mod 64): conflict-free A-layout reads
  const int fixed = kHubRows * rt.kpa + hub_red_floats(rt.np, 2) + kHubRows * kOutLd + kHubRows + 2 * kHubRows;
  const int kp = (Kc + H + 3) & ~3, pad = hub_bpad(F, rt.ntq);
  // B whole where it fits beside the rest, else in chunks of rows
  rt.ch = std::min(kp, ((kLdsFloats - fixed - pad) / F) & ~3);
  if (rt.ch < 4) return 3;
  rt.r1 = hub_region1_floats(rt.ch, F, rt.ntq);
  rt.lds_bytes = 4 * (int64_t)(rt.r1 + fixed);
  return rt.lds_bytes <= 4 * kLdsFloats ? 0 : 3;
}

template <int NTQ, int NP, int KHQ>
int launch_score(const ScoreArgs& a, int64_t lds_b, void* stream) {
  return launch_big_lds<score_docs_kernel<NTQ, NP, KHQ>>("score_docs_kernel", dim3((unsigned)hub_blocks(a.B)),
                                                         dim3(kHubThreads), (size_t)lds_b, stream, a);
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int gcnk_score_docs_route(int32_t F, int32_t Kc, int32_t H, int32_t P, int64_t* out8) {
  ScoreRoute rt;
  const int bad = out8 ? score_route(F, Kc, H, P, rt) : 1;
  if (bad == 1) {
    set_error("gcnk_score_docs_route: null out8 or bad sizes (F=%d Kc=%d H=%d P=%d)", F, Kc, H, P);
    return GCNK_EARG;
  }
  if (bad) {
    set_error("gcnk_score_docs_route: unsupported (F=%d %% 4, F <= 256, Kc=%d <= 128, H=%d <= 128, P=%d <= 32)", F,
              Kc, H, P);
    return GCNK_EUNSUP;
  }
  out8[0] = rt.ntq; out8[1] = rt.np; out8[2] = rt.khq; out8[3] = rt.ch; out8[4] = rt.kpa; out8[5] = rt.wd;
  out8[6] = rt.lds_bytes; out8[7] = 1;  // workgroups per 32 documents
  return GCNK_OK;
}

extern "C" int gcnk_score_docs_f32(int32_t B, int32_t F, int32_t Kc, int32_t H, int32_t P, int32_t k0, const float* x,
                                   int64_t ldx, const float* a, int64_t lda, const float* W1, int64_t ldw1,
                                   const float* S_T, int64_t lds, const float* W2, int64_t ldw2, const float* S2_T,
                                   int64_t lds2, const double* dh, const float* b1, const float* b2, float* out,
                                   int64_t ldo, int32_t* labels, void* stream) {
  if (B < 0 || F <= 0 || Kc <= 0 || H <= 0 || P <= 0 || k0 < 0) {
    set_error("gcnk_score_docs_f32: bad sizes (B=%d F=%d Kc=%d H=%d P=%d k0=%d)", B, F, Kc, H, P, k0);
    return GCNK_EARG;
  }
  if (B == 0) return GCNK_OK;
  if (!x || !a || !W1 || !S_T || !W2 || !S2_T || !dh || !out) {
    set_error("gcnk_score_docs_f32: null operand");
    return GCNK_EARG;
  }
  if (ldx < Kc || lda < H || ldw1 < F || lds < F || ldw2 < P || lds2 < P || ldo < P) {
    set_error("gcnk_score_docs_f32: leading dimension shorter than the row");
    return GCNK_EARG;
  }
  ScoreRoute rt;
  // 16-B rows of x, a, W1, S_T; 32-bit buffer offsets inside a block's rows and over the rows of W2 / S2_T
  // that phase 3 addresses (rows 0 .. 64 NTQ - 1 and 0 .. 16 KHQ - 1, past F and H too; a lane turned off
  // starts from kBufOob and steps as far again, below 2^32)
  const int64_t lim = (int64_t)kBufOob / 4;
  if (score_route(F, Kc, H, P, rt) || ldx % 4 || lda % 4 || ldw1 % 4 || lds % 4 || !aligned16(x) || !aligned16(a) ||
      !aligned16(W1) || !aligned16(S_T) || (reinterpret_cast<uintptr_t>(dh) & 7u) || kHubRows * ldx >= lim ||
      kHubRows * lda >= lim || kHubRows * ldo >= lim || 64 * rt.ntq * ldw2 >= lim || 16 * rt.khq * lds2 >= lim) {
    set_error("gcnk_score_docs_f32: unsupported shape (F=%d %% 4, F <= 256, Kc=%d <= 128, H=%d <= 128, P=%d <= 32, "
              "16-B aligned rows of x / a / W1 / S_T)", F, Kc, H, P);
    return GCNK_EUNSUP;
  }
  ScoreArgs s;
  s.B = B; s.F = F; s.Kc = Kc; s.H = H; s.P = P; s.k0 = k0;
  s.x = x; s.ldx = ldx; s.a = a; s.lda = lda; s.W1 = W1; s.ldw1 = ldw1; s.S = S_T; s.lds = lds;
  s.W2 = W2; s.ldw2 = ldw2; s.S2 = S2_T; s.lds2 = lds2; s.dh = dh; s.b1 = b1; s.b2 = b2;
  s.out = out; s.ldo = ldo; s.labels = labels;
  s.ch = rt.ch; s.kpa = rt.kpa; s.r1 = rt.r1;
#define GCNK_SCORE_CASE(NTQ_)                                                                          \
  if (rt.ntq == NTQ_) {                                                                                \
    if (rt.np == 1)                                                                                    \
      return rt.khq == 4 ? launch_score<NTQ_, 1, 4>(s, rt.lds_bytes, stream)                           \
                         : launch_score<NTQ_, 1, 8>(s, rt.lds_bytes, stream);                          \
    return rt.khq == 4 ? launch_score<NTQ_, 2, 4>(s, rt.lds_bytes, stream)                             \
                       : launch_score<NTQ_, 2, 8>(s, rt.lds_bytes, stream);                            \
  }
  GCNK_SCORE_CASE(2) GCNK_SCORE_CASE(3) GCNK_SCORE_CASE(4)
#undef GCNK_SCORE_CASE
  set_error("gcnk_score_docs_f32: no kernel for F=%d", F);
  return GCNK_EUNSUP;
}
