// The SpMM plan format and the row kernel's launch geometry, stated once for
// the host planner (spmm_plan.cpp), the kernels and launches (spmm.hip) and
// the C-ABI comment (gcnk.h).  Plain C++: no HIP header needed.
#pragma once

#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define GCNK_HD __host__ __device__
#else
#define GCNK_HD
#endif
#define GCNK_LOCAL __attribute__((visibility("hidden")))  // shared between libgcnk's files, not exported

namespace gcnk {

// Thread-local error text returned by gcnk_last_error() (abi.cpp).
void set_error(const char* fmt, ...);

constexpr int32_t kMagic = 0x474e4b35;  // "GNK5"
constexpr int kRB = 64;                 // tile rows per dense block (4 waves x 16)
constexpr int kKC = 64;                 // condensed columns per tile chunk (16 MFMA k-steps)
constexpr int kMaxColTiles = 64;        // row-kernel column tiles per launch (arrival counters per heavy row)
constexpr int kMaxSeg = 64;             // slots per heavy entry (bounds a last arriver's combine)
constexpr int kMaxSegRow = kMaxSeg * kMaxSeg;  // segments per heavy row (two combine levels)

// ---------------------------------------------------------------------------
// Plan header (16 int32, first words of the plan; gcnk_spmm_plan_query):
//   0 magic 'GNK5'  1 M  2 K  3 groups (lane groups per wavefront, 64 / LPR)
//   4 ipc  5 row units  6 heavy segments (heavy region, padded)
//   7 heavy rows of > 1 segment  8 tile chunks  9 multi-chunk blocks  10 slabs
//   11 tile blocks  12 diagonal kept aside | segp << 1 | tops << 30  13 nnz
//   14 partial slots  15 chunk items of single-chunk tile blocks (listed first)
enum : int {
  kHdrMagic = 0, kHdrM, kHdrK, kHdrGroups, kHdrIpc, kHdrNunits, kHdrNhunits, kHdrNheavy,
  kHdrNtile, kHdrNred, kHdrNslabs, kHdrNtblk, kHdrFlags, kHdrNnz, kHdrNslots, kHdrNsingle,
  kHdrWords
};
// word 12: bit 0 the tile rows' diagonal is kept aside; bits 1-29 segp, the
// stride (items) of the heavy units' padded item copies (0: none); bit 30 tops,
// some row has more than kMaxSeg segments (a top heavy entry)
GCNK_HD inline bool has_diag(const int32_t* h) { return h[kHdrFlags] & 1; }
GCNK_HD inline int32_t segp(const int32_t* h) { return ((uint32_t)h[kHdrFlags] >> 1) & ((1u << 29) - 1); }
GCNK_HD inline bool tops(const int32_t* h) { return ((uint32_t)h[kHdrFlags] >> 30) & 1; }
inline bool plan_magic(const int32_t* h) { return h && h[kHdrMagic] == kMagic; }
inline int32_t flags_word(bool diag, int64_t segp_, bool tops_) {
  return (diag ? 1 : 0) | (int32_t)(segp_ << 1) | (tops_ ? 1 << 30 : 0);
}

// Body (int32 words after the header): items int2[nnz] {col, value bits} in
//   CSR order | units int4[nunits] {row (-1: empty), nz begin, nz end, heavy
//   entry * 64 + slot or -1}: the heavy region first, then light rows, each
//   laid out so that the units of workgroup b belong to XCD class b % 8 |
//   heavy int4[nheavy] {row, first partial slot, slots, -1 (a row of <=
//   kMaxSeg segments), or for a row of more (tops): one entry per group of <=
//   kMaxSeg segments with .w = the top entry's slot for the group's sum, and
//   the top entry, .w = -2} | tile part (descriptors, condensed columns, A
//   fragments, reduce rows int4[64 * nred] {row (-1: none), first slab, slabs,
//   diagonal value bits}, row lists, extracted diagonal float[64 * ntblk] in
//   block order) | (segp > 0) the heavy units' items, padded:
//   int2[nhunits][segp], col -1 past a unit's end.
struct GCNK_LOCAL Layout {
  int64_t M, nnz, nunits, nhunits, nheavy, nslots, ntile, nred, ntblk, has_diag, segp, tops;
  int64_t items, units, heavy, tdesc, tcols, tfrag, red, trows, dval, hitems, total;
  GCNK_HD explicit Layout(const int32_t* h) {
    M = h[kHdrM]; nunits = h[kHdrNunits]; nhunits = h[kHdrNhunits]; nheavy = h[kHdrNheavy]; ntile = h[kHdrNtile];
    nred = h[kHdrNred]; ntblk = h[kHdrNtblk];
    has_diag = gcnk::has_diag(h); segp = gcnk::segp(h); tops = gcnk::tops(h);
    nnz = h[kHdrNnz]; nslots = h[kHdrNslots];
    items = kHdrWords;
    units = (items + 2 * nnz + 3) & ~3LL;
    heavy = units + 4 * nunits;
    tdesc = (heavy + 4 * nheavy + 3) & ~3LL;
    tcols = tdesc + 4 * ntile;
    tfrag = (tcols + (int64_t)kKC * ntile + 3) & ~3LL;
    red = tfrag + (int64_t)kRB * kKC * ntile;
    trows = red + 4 * nred * kRB;
    dval = trows + (int64_t)kRB * ntblk;
    hitems = (dval + (has_diag ? (int64_t)kRB * ntblk : 0) + 3) & ~3LL;
    total = hitems + 2 * nhunits * segp;   // padded heavy items int2[nhunits][segp]
  }
};

// floats per row of a tile slab (workspace): F padded to whole 16-column n-tiles
inline int64_t tile_fpad(int32_t F) { return ((int64_t)F + 15) & ~15LL; }

inline int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// Lanes per group from F alone (a plan does not depend on pointer alignment,
// which only picks VEC at launch): the smallest power of two covering the row
// in VEC-wide vectors, at most 64 (a whole wavefront per row and column tile).
inline int choose_lpr(int32_t F, int lanes_hint) {
  if (lanes_hint > 0) return next_pow2(lanes_hint > 64 ? 64 : lanes_hint);
  const int Wv = (F % 4 == 0) ? F / 4 : F;
  return Wv <= 64 ? next_pow2(Wv < 1 ? 1 : Wv) : 64;
}

// ---------------------------------------------------------------------------
// Launch geometry of the row kernel for lane groups of `lpr` lanes.  The
// planner lays the units out for it and the kernel walks them by it: the two
// must agree, or the answer is wrong without an error.
constexpr int kNarrowMin = 2;  // narrowest group on 256-thread workgroups (1 lane: one-wave workgroups,
                               // so a light launch still spans the chip)
struct RowGeom {
  int block;      // threads per workgroup
  int wpb;        // wavefronts per workgroup
  int sg;         // lane groups per workgroup
  bool wg_heavy;  // a heavy segment spans the workgroup (else one wavefront)
  int gs;         // lane groups sharing a heavy segment
  int hpb;        // heavy units per workgroup
  int lpb;        // light units per workgroup (one per lane group)
  constexpr int64_t seg(int32_t ipc) const { return (int64_t)ipc * gs; }  // nonzeros per heavy segment
};
GCNK_HD constexpr RowGeom row_geom(int lpr) {
  const bool wg = lpr >= kNarrowMin;
  const int block = wg ? 256 : 64, wpb = block / 64, sg = block / lpr;
  return RowGeom{block, wpb, sg, wg, (64 / lpr) * (wg ? wpb : 1), wg ? 1 : wpb, sg};
}

inline int choose_block(int lpr) { return row_geom(lpr).block; }

// ---------------------------------------------------------------------------
// The planner (spmm_plan.cpp), for the entry points that copy from or to the
// device.  build_image: the plan image for host CSR arrays; plan_size: its
// bytes, without making it (or a negative error code).
GCNK_LOCAL int build_image(const int32_t* rp, const int32_t* ci, const float* vv, int32_t M, int32_t K, int64_t nnz,
                           int32_t ipc, int32_t groups, float dense_threshold, std::vector<int32_t>& img);
GCNK_LOCAL int64_t plan_size(const int32_t* rp, const int32_t* ci, int32_t M, int32_t K, int64_t nnz, int32_t ipc,
                             int32_t groups, float dense_threshold);
GCNK_LOCAL bool plan_args_ok(const int32_t* rowptr, const int32_t* colind, int32_t M, int32_t K, int64_t nnz,
                             int32_t ipc, int32_t groups);

}  // namespace gcnk
