// The hub-factor block, stated once: the record the doc-topic kernels exchange and the geometry of the two
// MFMA kernels that work a block at a time (hubfactor_gc1_kernel, score_docs_kernel).
#pragma once

#include "gcnk_common.h"

namespace gcnk {

// The block record (written by factor_build.hip, read by factor.hip and factor_gc2.hip; factor.py sizes it,
// tests/hub_records.py packs it by hand).  Block b holds the rows perm[32 b .. 32 b + 31] of the block order: the
// host spreads the hub rows (long item lists) over the blocks, U's rows are in that order, outputs go to the row ids.
//   word 0 .. 32    item offsets of the block's 32 rows and the end, block-relative
//   word 33 .. 35   pad (the row ids start a 16-byte piece)
//   word 36 .. 67   the 32 output row ids, -1 past M
//   word 68 ..      the rows' A_H items in CSR order, two words each: {hub index, fp32 value bits}
// Every record of a factor has the same length rec_words: a multiple of 4 (16-byte DMA pieces), at least the head.
constexpr int kHubRows = 32;      // rows per block
constexpr int kHubRecRow = 36;    // first row-id word
constexpr int kHubRecHead = 68;   // words before the items
using HubItem = int2;             // {hub, value bits}
__host__ __device__ constexpr bool hub_rec_words_ok(int w) { return w >= kHubRecHead && w % 4 == 0; }
__host__ __device__ constexpr int64_t hub_blocks(int64_t M) { return (M + kHubRows - 1) / kHubRows; }

// The MFMA block: 32 rows on 512 threads, 8 waves as 2 row strips of 16 x 4 quarters.  Wave w holds strip w & 1 and
// quarter w >> 1; in a 16x16x4 fp32 MFMA lane l holds A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15] and
// C/D register r = [row 4 (l >> 4) + r][col l & 15].
//   phase 1  Z [32 x F] = A B, B staged in LDS as rows of F floats: a wave takes up to NTQ 16-column tiles of F
//   then     Z through LDS (s_Z, which overlays the staged B) to rows of hub_z_stride floats
//   last     a projection [32 x F] [F x P]: a quarter sums its quarter of K = 64 NTQ on two accumulator chains
//            (even and odd k-steps, added last); quarters 1 .. 3 leave their partials in s_red, slot
//            [n-tile or sum][quarter - 1][strip][lane][4], and quarter 0 adds the three in order to its own
constexpr int kHubThreads = 512;
constexpr int kHubProjMax = 32;    // projection width: P <= 32 (NP = 1 or 2 MFMA n-tiles)
constexpr int kHubTileStep = 64;   // columns between a wave's consecutive tiles
__host__ __device__ constexpr int hub_pick_ntq(int f) { return f <= 128 ? 2 : f <= 192 ? 3 : 4; }   // F <= 64 NTQ
__host__ __device__ constexpr int hub_pick_np(int p) { return p <= 16 ? 1 : 2; }                    // P <= 16 NP
// zero floats after the staged rows of B: the last n-tile of a wave reads up to column 64 NTQ - 1 of the last k-row
// (the pad, 64 NTQ - F and at least 64, is sized for every tile up to that column, which the kernels once computed)
__host__ __device__ constexpr int hub_bpad(int f, int ntq) { return 64 * ntq - f > 64 ? 64 * ntq - f : 64; }
// s_Z row stride: 16-B rows, conflict-free MFMA-layout accesses
__host__ __device__ constexpr int hub_z_stride(int ntq) { return 64 * ntq + 4; }
// floats of the LDS region that `brows` staged rows of B (and their pad) share with s_Z
__host__ __device__ constexpr int hub_region1_floats(int brows, int f, int ntq) {
  const int b = brows * f + hub_bpad(f, ntq), z = kHubRows * hub_z_stride(ntq);
  return b > z ? b : z;
}
// floats of s_red for `sums` projected sums of NP n-tiles: quarters 1 .. 3 x strips x lanes x a C/D fragment
__host__ __device__ constexpr int hub_red_floats(int np, int sums = 1) { return np * sums * 3 * 2 * 64 * 4; }

// Phase 1's tile deal.  The phase is bound by MFMA issue, so n-tiles that hold no column of F are not computed.
// The T = ceil(F / 16) real tiles are dealt round-robin over the column quarters, in opposite directions in the two
// strips (tile g of strip 0 to quarter g % 4, of strip 1 to quarter 3 - g % 4): whether the eight waves sit on the
// four SIMDs by wave id modulo 4 or in pairs, no SIMD carries more than ceil(T / 2) tiles a k-step (R8: 7, 7, 6, 6
// in place of 8 each).  The wave's tile i covers columns 16 qe + 64 i ..; the lane's column of it is c0 + 64 i; nt
// (wave-uniform) of the NTQ slots hold a real tile.  A slot without one keeps its zero accumulator.
struct HubDeal { int qe, c0, nt; };
__device__ __forceinline__ HubDeal hub_deal(int strip, int quarter, int lane, int F, int ntq) {
  const int qe = strip ? 3 - quarter : quarter;
  const int T = (F + 15) >> 4;
  return HubDeal{qe, qe * 16 + (lane & 15), __builtin_amdgcn_readfirstlane(min(max((T - qe + 3) >> 2, 0), ntq))};
}

// The lane's B fragments of a projection operand X [rows x P] (leading dimension ld floats) for the k-steps
// row0, row0 + 4, ...: b[j] = X[row0 + 4 j][col], through a buffer resource the caller makes over exactly X's
// floats.  A row past the operand lies past the resource and reads 0 with no compare.  A column col >= P would land
// inside the next row, so its lane starts from an offset past the resource, chosen once.  (The host checks that
// every offset formed here fits 32 bits.)
template <int N>
__device__ __forceinline__ void hub_proj_frags(float (&b)[N], __amdgpu_buffer_rsrc_t r, int row0, int ld, int col,
                                               int P) {
  const int kstep = 16 * ld;   // bytes between the lane's consecutive k (4 rows of ld floats)
  int off = col < P ? (row0 * ld + col) * 4 : (int)kBufOob;
#pragma unroll
  for (int j = 0; j < N; ++j, off += kstep) b[j] = buf_load_f32(r, off);
}

}  // namespace gcnk
