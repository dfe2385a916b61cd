// Host planner of the CSR SpMM (spmm.hip): host CSR arrays -> plan image
// (format: spmm_plan.h).  Plain C++, no device: builds with any host compiler.
#include "spmm_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/gcnk.h"

namespace gcnk {
namespace {

struct HostPlan {
  int32_t hdr[kHdrWords];
  std::vector<int32_t> units, heavy;  // row-kernel units (int4 each), heavy rows (int4 each)
  std::vector<int32_t> tdesc, tcols, red, trows;
  std::vector<float> tfrag, dval;  // dval: extracted diagonal of tile rows in block order (64 per block, or empty)
};

// what the tile half leaves for the header
struct TileCounts {
  int32_t ntile = 0, nred = 0, nslabs = 0, ntblk = 0, nsingle = 0;
  bool any_diag = false;
};

// rowptr / colind validity (host arrays): monotone row pointers, in-range columns.
int check_csr(const int32_t* rp, const int32_t* ci, int32_t M, int32_t K, int64_t nnz) {
  if ((int64_t)rp[M] != nnz || rp[0] != 0) {
    set_error("gcnk_spmm_plan: rowptr[0]=%d rowptr[M]=%d inconsistent with nnz=%lld", rp[0], rp[M], (long long)nnz);
    return GCNK_EARG;
  }
  for (int32_t r = 0; r < M; ++r)
    if (rp[r + 1] < rp[r]) {
      set_error("gcnk_spmm_plan: rowptr decreases at row %d", r);
      return GCNK_EARG;
    }
  for (int64_t k = 0; k < nnz; ++k)
    if (ci[k] < 0 || ci[k] >= K) {
      set_error("gcnk_spmm_plan: column index %d out of range [0, %d) at nonzero %lld", ci[k], K, (long long)k);
      return GCNK_EARG;
    }
  return GCNK_OK;
}

// ---- dense blocks (tile path; vv null: layout only).  Rows are grouped by
//      degree class (factor-8 buckets of the off-diagonal degree), in row order
//      within a class, 64 per block, so rows of one shape share blocks (R8:
//      document rows vs topic rows).  A block goes to the MFMA tile path when its
//      nonzeros fill at least dense_threshold of its condensed column set and
//      each condensed column is used at least twice on average; its rows'
//      diagonal entries (r < K) are taken out of the column set and added in the
//      epilogue (dval[r] * B[r,:]).  tile_row[r] = 1 for the rows it takes.
TileCounts plan_tiles(const int32_t* rp, const int32_t* ci, const float* vv, int32_t M, int32_t K,
                      float dense_threshold, HostPlan& hp, std::vector<char>& tile_row) {
  const bool want_values = vv != nullptr;
  tile_row.assign((size_t)M, 0);
  TileCounts t;
  hp.dval.clear();
  // the diagonal is kept aside for square operands (A-hat's self loops); a
  // rectangular operand (X) has no diagonal to speak of
  auto is_diag = [&](int32_t r, int64_t k) { return M == K && ci[(size_t)k] == r; };
  if (!(dense_threshold <= 1.0f && M > 0)) return t;
  std::vector<std::vector<int32_t>> cls(33);
  for (int32_t r = 0; r < M; ++r) {
    int64_t deg = 0;
    for (int64_t k = rp[r]; k < rp[r + 1]; ++k) deg += !is_diag(r, k);
    int bw = 0;
    while (bw < 63 && (deg >> bw) != 0) ++bw;
    cls[(size_t)(bw / 3)].push_back(r);
  }
  std::vector<int32_t> cmap((size_t)K, -1);
  std::vector<int32_t> seen((size_t)K, -1);  // block stamp per column: distinct count without a sort
  int32_t stampv = 0;
  std::vector<int32_t> cols;
  std::vector<float> dv((size_t)M, 0.f);
  for (const std::vector<int32_t>& rows : cls) {
    for (size_t i0 = 0; i0 < rows.size(); i0 += kRB, ++stampv) {
      const size_t i1 = std::min(rows.size(), i0 + kRB);
      int64_t bnnz = 0, ncols = 0;
      for (size_t i = i0; i < i1; ++i) {
        const int32_t r = rows[i];
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k)
          if (!is_diag(r, k)) {
            int32_t& sv = seen[(size_t)ci[(size_t)k]];
            ncols += sv != stampv;
            sv = stampv;
            ++bnnz;
          }
      }
      if (bnnz == 0) continue;
      const int64_t nrows = (int64_t)(i1 - i0);
      // the density test needs only the counts; the sorted column set is built
      // for the blocks that pass it (a sparse operand -- 1M/20M -- has none)
      if ((double)bnnz < (double)dense_threshold * (double)nrows * (double)ncols || bnnz < 2 * ncols) continue;
      cols.clear();
      for (size_t i = i0; i < i1; ++i) {
        const int32_t r = rows[i];
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k)
          if (!is_diag(r, k)) cols.push_back(ci[(size_t)k]);
      }
      std::sort(cols.begin(), cols.end());
      cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
      const int32_t nch = (int32_t)((ncols + kKC - 1) / kKC);
      const int32_t first_slab = nch > 1 ? t.nslabs : -1;
      const int32_t blk = t.ntblk++;
      for (int64_t c = 0; c < ncols; ++c) cmap[(size_t)cols[(size_t)c]] = (int32_t)c;
      const size_t base_item = (size_t)t.ntile;
      for (int32_t ch = 0; ch < nch; ++ch) {
        // a chunk whose condensed columns are one contiguous run (R8's X: the
        // 50 topic columns; 64-column pieces of the dense topic rows) is
        // described by its first column and length (y bits 8.., w), so the
        // kernel stages its B rows without waiting for the column list
        const int64_t c0 = (int64_t)ch * kKC;
        const int32_t kc = (int32_t)std::min<int64_t>(kKC, ncols - c0);
        bool contig = true;
        for (int32_t k = 1; k < kc && contig; ++k) contig = cols[(size_t)(c0 + k)] == cols[(size_t)c0] + k;
        // y: rows | contiguous run << 8 | condensed width << 16 (the kernel's k-steps)
        hp.tdesc.insert(hp.tdesc.end(), {blk, (int32_t)nrows | (contig ? kc << 8 : 0) | kc << 16,
                                         nch > 1 ? first_slab + ch : -1, contig ? cols[(size_t)c0] : 0});
        for (int k = 0; k < kKC; ++k) {
          const int64_t cc = (int64_t)ch * kKC + k;
          hp.tcols.push_back(cc < ncols ? cols[(size_t)cc] : -1);
        }
      }
      for (int64_t rl = 0; rl < kRB; ++rl) hp.trows.push_back(rl < nrows ? rows[i0 + (size_t)rl] : -1);
      hp.tfrag.resize(hp.tfrag.size() + (size_t)nch * kRB * kKC, 0.f);
      for (size_t i = i0; i < i1; ++i) {
        const int32_t r = rows[i];
        const int32_t rl = (int32_t)(i - i0), tw = rl / 16, lr = rl % 16;
        tile_row[(size_t)r] = 1;
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
          if (is_diag(r, k)) {
            t.any_diag = true;
            if (want_values) dv[(size_t)r] += vv[(size_t)k];
            continue;
          }
          if (!want_values) continue;
          const int32_t cc = cmap[(size_t)ci[(size_t)k]];
          const int32_t ch = cc / kKC, kk = cc % kKC;
          const int32_t st = kk / 4, kq = kk % 4;
          const int32_t ln = kq * 16 + lr;
          hp.tfrag[(((base_item + ch) * 4 + tw) * 64 + ln) * 16 + st] += vv[(size_t)k];
        }
      }
      for (int64_t c = 0; c < ncols; ++c) cmap[(size_t)cols[(size_t)c]] = -1;
      if (nch > 1) {  // one reduce entry per row: the reduce kernel needs no other plan read
        for (int64_t rl = 0; rl < kRB; ++rl) {
          const int32_t r = rl < nrows ? rows[i0 + (size_t)rl] : -1;
          hp.red.insert(hp.red.end(), {r, first_slab, nch, r >= 0 ? __builtin_bit_cast(int32_t, dv[(size_t)r]) : 0});
        }
        ++t.nred;
        t.nslabs += nch;
      }
      t.ntile += nch;
    }
  }
  // chunk items of single-chunk blocks first, then the multi-chunk ones (which
  // also need the reduce launch): the two runs can be launched separately
  // (gcnk_spmm_csr_f32_part), e.g. on two streams
  {
    const int32_t ntile = t.ntile;
    std::vector<int32_t> order;
    for (int32_t i = 0; i < ntile; ++i)
      if (hp.tdesc[(size_t)i * 4 + 2] < 0) order.push_back(i);
    t.nsingle = (int32_t)order.size();
    for (int32_t i = 0; i < ntile; ++i)
      if (hp.tdesc[(size_t)i * 4 + 2] >= 0) order.push_back(i);
    std::vector<int32_t> td((size_t)ntile * 4), tc((size_t)ntile * kKC);
    std::vector<float> tf((size_t)ntile * kRB * kKC);
    for (int32_t j = 0; j < ntile; ++j) {
      const size_t i = (size_t)order[(size_t)j];
      std::copy(hp.tdesc.begin() + i * 4, hp.tdesc.begin() + i * 4 + 4, td.begin() + (size_t)j * 4);
      std::copy(hp.tcols.begin() + i * kKC, hp.tcols.begin() + (i + 1) * kKC, tc.begin() + (size_t)j * kKC);
      if (!hp.tfrag.empty())
        std::copy(hp.tfrag.begin() + i * kRB * kKC, hp.tfrag.begin() + (i + 1) * kRB * kKC,
                  tf.begin() + (size_t)j * kRB * kKC);
    }
    hp.tdesc.swap(td);
    hp.tcols.swap(tc);
    if (!hp.tfrag.empty()) hp.tfrag.swap(tf);
  }
  if (t.any_diag) {  // block order, so kernels index it by (block, row in block) without the row list
    hp.dval.assign((size_t)t.ntblk * kRB, 0.f);
    for (size_t i = 0; i < hp.trows.size(); ++i)
      if (hp.trows[i] >= 0) hp.dval[i] = dv[(size_t)hp.trows[i]];
  }
  return t;
}

// ---- row units over the rows the tile half left (tile_row[r] == 0), and the
//      header.  Launch geometry from `groups` = 64 / LPR (RowGeom).
//      (light_sort false: the layout and counts only -- enough for the plan's size)
int plan_rows(const int32_t* rp, const int32_t* ci, int32_t M, int32_t K, int64_t nnz, int32_t ipc, int32_t groups,
              const std::vector<char>& tile_row, const TileCounts& t, HostPlan& hp, bool light_sort) {
  if (groups < 1 || groups > 64 || (groups & (groups - 1))) {
    set_error("gcnk_spmm_plan: groups %d is not a power of two in [1, 64]", groups);
    return GCNK_EARG;
  }
  const int lpr = 64 / groups;
  const RowGeom g = row_geom(lpr);
  const int64_t seg = g.seg(ipc);  // nonzeros per segment
  // light-row limit: a whole-wavefront group reads a light row's items with one
  // 64-lane vector load, so at most 64 nonzeros, and at most 2 * ipc (a longer
  // row is walked by a 4-wavefront workgroup as a heavy segment); ipc otherwise
  const int64_t light_max = lpr == 64 ? std::min<int64_t>(2 * (int64_t)ipc, 64) : ipc;
  // XCD classes.  Workgroups b and b + 8 land on one XCD (round-robin dispatch;
  // speed only, never correctness), so every unit of workgroup b is given
  // class b % 8: a light row by its row index, a heavy segment by the column
  // range it gathers (heavy rows are first cut where their sorted column
  // indices cross a class boundary).  Each XCD's L2 then serves 1/8 of B
  // instead of every XCD fetching the rows its segments happen to need
  // (R8 Â: the topic rows gather all document rows).
  constexpr int NX = 8;
  auto cls = [](int64_t i, int64_t n) { return n > 0 ? (int)(i * NX / n) : 0; };
  std::vector<std::vector<int32_t>> hq(NX), lq(NX);  // int4 units per class
  int32_t nheavy = 0;
  int64_t nslots = 0;
  bool any_top = false;
  hp.units.clear();
  hp.heavy.clear();
  std::vector<int64_t> rb, rcl;  // runs of one column class: start, class
  int64_t rr_class = 0;
  for (int32_t r = 0; r < M; ++r) {
    if (tile_row[(size_t)r]) continue;
    const int64_t b = rp[r], e = rp[r + 1], deg = e - b;
    if (deg <= light_max) {
      lq[(size_t)cls(r, M)].insert(lq[(size_t)cls(r, M)].end(), {r, (int32_t)b, (int32_t)e, -1});
      continue;
    }
    rb.clear();
    rcl.clear();
    // cut at column-class boundaries only when the runs average half a segment or
    // more (a 20-nonzero row must not become 8 tiny segments)
    if (deg * 2 >= seg * NX)
      for (int64_t k = b; k < e; ++k) {
        const int c = cls(ci[(size_t)k], K);
        if (rcl.empty() || rcl.back() != c) { rb.push_back(k); rcl.push_back(c); }
      }
    if (rb.empty() || (int64_t)rb.size() > NX) {  // short row, or columns not sorted: one run,
      rb.assign(1, b);                              // classes dealt round-robin (balance)
      rcl.assign(1, (int64_t)(rr_class++ % NX));
    }
    rb.push_back(e);
    const int64_t nruns = (int64_t)rcl.size();
    // segments of `seg` nonzeros (longer only past kMaxSegRow of them, ~200k
    // nonzeros at R8's widths): a row of more than kMaxSeg segments gets two
    // combine levels instead of longer segments, so a power-law hub is walked
    // by many short segments, not by 64 long ones
    int64_t sr = seg, nseg = 0;
    for (;;) {
      nseg = 0;
      for (int64_t i = 0; i < nruns; ++i) nseg += (rb[(size_t)i + 1] - rb[(size_t)i] + sr - 1) / sr;
      if (nseg <= kMaxSegRow) break;
      sr *= 2;
    }
    if (nseg == 1) {
      hq[(size_t)rcl[0]].insert(hq[(size_t)rcl[0]].end(), {r, (int32_t)b, (int32_t)e, -1});
      continue;
    }
    // heavy entries: one (nseg <= kMaxSeg), or a top entry over ng groups of
    // consecutive segments (group g: segments [g nseg / ng, (g + 1) nseg / ng))
    const int64_t ng = nseg <= kMaxSeg ? 1 : (nseg + kMaxSeg - 1) / kMaxSeg;
    int64_t top_slot = -1;
    if (ng > 1) {
      ++nheavy;
      hp.heavy.insert(hp.heavy.end(), {r, (int32_t)nslots, (int32_t)ng, -2});
      top_slot = nslots;
      nslots += ng;
      any_top = true;
    }
    std::vector<int32_t> seg_w((size_t)nseg);
    for (int64_t gi = 0; gi < ng; ++gi) {
      const int64_t s0 = gi * nseg / ng, s1 = (gi + 1) * nseg / ng;
      const int32_t hid = nheavy++;
      hp.heavy.insert(hp.heavy.end(), {r, (int32_t)nslots, (int32_t)(s1 - s0), ng > 1 ? (int32_t)(top_slot + gi) : -1});
      for (int64_t sgi = s0; sgi < s1; ++sgi) seg_w[(size_t)sgi] = (int32_t)((int64_t)hid * 64 + (sgi - s0));
      nslots += s1 - s0;
    }
    int64_t sgi = 0;
    for (int64_t i = 0; i < nruns; ++i) {
      const int64_t pb = rb[(size_t)i], len = rb[(size_t)i + 1] - pb, np = (len + sr - 1) / sr;
      std::vector<int32_t>& q = hq[(size_t)rcl[(size_t)i]];
      for (int64_t s = 0; s < np; ++s, ++sgi)
        q.insert(q.end(), {r, (int32_t)(pb + len * s / np), (int32_t)(pb + len * (s + 1) / np), seg_w[(size_t)sgi]});
    }
  }
  // lay out rounds of NX workgroups, workgroup 8k + c taking `per` units of class c
  // (empty units pad short classes)
  auto layout = [&](std::vector<std::vector<int32_t>>& qs, int per) {
    size_t rounds = 0;
    for (const auto& q : qs) rounds = std::max(rounds, (q.size() / 4 + per - 1) / per);
    for (size_t k = 0; k < rounds; ++k)
      for (int c = 0; c < NX; ++c)
        for (int j = 0; j < per; ++j) {
          const size_t i = (k * per + j) * 4;
          if (i < qs[(size_t)c].size())
            hp.units.insert(hp.units.end(), qs[(size_t)c].begin() + i, qs[(size_t)c].begin() + i + 4);
          else
            hp.units.insert(hp.units.end(), {-1, 0, 0, -1});
        }
  };
  // light rows of a class ordered by their off-diagonal column lists, so the
  // rows one workgroup (one CU's L1) gathers for share their B rows (R8: the
  // document rows of one topic set); each row still writes its own C row
  // (ordered by a key of the first two off-diagonal columns, the full lists only
  // on equal keys, then by position: the order of a stable sort by the lists;
  // 1M/20M: 0.49 -> 0.05 s per build)
  if (light_sort)
    for (std::vector<int32_t>& q : lq) {
      const size_t n = q.size() / 4;
      std::vector<size_t> ord(n);
      for (size_t i = 0; i < n; ++i) ord[i] = i;
      std::vector<uint64_t> key(n);
      for (size_t i = 0; i < n; ++i) {
        const int32_t r = q[4 * i];
        uint64_t c[2] = {0, 0};  // column + 1, 0 past the list's end (a prefix sorts first)
        int got = 0;
        for (int32_t k = q[4 * i + 1]; k < q[4 * i + 2] && got < 2; ++k)
          if (ci[(size_t)k] != r) c[got++] = (uint64_t)ci[(size_t)k] + 1;
        key[i] = c[0] << 32 | c[1];
      }
      auto less_list = [&](size_t x, size_t y) {
        const int32_t rx = q[4 * x], ry = q[4 * y];
        int32_t kx = q[4 * x + 1], ky = q[4 * y + 1];
        const int32_t ex = q[4 * x + 2], ey = q[4 * y + 2];
        for (;;) {
          while (kx < ex && ci[(size_t)kx] == rx) ++kx;
          while (ky < ey && ci[(size_t)ky] == ry) ++ky;
          if (kx >= ex || ky >= ey) return kx >= ex && ky < ey;
          if (ci[(size_t)kx] != ci[(size_t)ky]) return ci[(size_t)kx] < ci[(size_t)ky];
          ++kx;
          ++ky;
        }
      };
      std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) {
        if (key[x] != key[y]) return key[x] < key[y];
        if (less_list(x, y)) return true;
        if (less_list(y, x)) return false;
        return x < y;
      });
      std::vector<int32_t> sorted(q.size());
      for (size_t i = 0; i < n; ++i) std::copy(q.begin() + 4 * ord[i], q.begin() + 4 * ord[i] + 4, sorted.begin() + 4 * i);
      q.swap(sorted);
    }
  layout(hq, g.hpb);
  const int64_t nh = (int64_t)hp.units.size() / 4;
  // padded item copies of the heavy units (whole-wavefront groups), so a heavy
  // workgroup loads its items at an address it knows from its index: stride =
  // the longest unit, rounded up to 4 items
  int64_t segp = 0;
  if (lpr == 64)
    for (int64_t u = 0; u < nh; ++u)
      if (hp.units[(size_t)(4 * u)] >= 0)
        segp = std::max<int64_t>(segp, (int64_t)hp.units[(size_t)(4 * u + 2)] - hp.units[(size_t)(4 * u + 1)]);
  segp = (segp + 3) & ~3LL;
  if (segp >= (1 << 28) || 2 * nh * segp >= (int64_t)INT32_MAX) segp = 0;   // (never for real plans: the kernel then
                                                                            // reads the items through the unit word)
  layout(lq, g.lpb);
  const int64_t nunits = (int64_t)hp.units.size() / 4;
  if (nunits >= (int64_t)INT32_MAX || nslots >= (int64_t)INT32_MAX || nheavy >= (1 << 25)) {
    set_error("gcnk_spmm_plan: %lld row units / %lld partial slots exceed the plan's int32 fields",
              (long long)nunits, (long long)nslots);
    return GCNK_EUNSUP;
  }
  int32_t* h = hp.hdr;
  h[kHdrMagic] = kMagic; h[kHdrM] = M; h[kHdrK] = K; h[kHdrGroups] = groups; h[kHdrIpc] = ipc;
  h[kHdrNunits] = (int32_t)nunits; h[kHdrNhunits] = (int32_t)nh; h[kHdrNheavy] = nheavy;
  h[kHdrNtile] = t.ntile; h[kHdrNred] = t.nred; h[kHdrNslabs] = t.nslabs; h[kHdrNtblk] = t.ntblk;
  h[kHdrFlags] = flags_word(t.any_diag, segp, any_top);
  h[kHdrNnz] = (int32_t)nnz; h[kHdrNslots] = (int32_t)nslots; h[kHdrNsingle] = t.nsingle;
  return GCNK_OK;
}

// Row-unit + dense-tile plan from host CSR arrays (vv null: layout only).
int host_plan(const int32_t* rp, const int32_t* ci, const float* vv, int32_t M, int32_t K, int64_t nnz, int32_t ipc,
              int32_t groups, float dense_threshold, HostPlan& hp, bool light_sort = true) {
  std::vector<char> tile_row;
  const TileCounts t = plan_tiles(rp, ci, vv, M, K, dense_threshold, hp, tile_row);
  return plan_rows(rp, ci, M, K, nnz, ipc, groups, tile_row, t, hp, light_sort);
}

// Full classic plan image (header, packed items, units, heavy rows, tile part).
void classic_image(const HostPlan& hp, const int32_t* ci, const float* vv, int64_t nnz, std::vector<int32_t>& img) {
  const Layout L(hp.hdr);
  img.assign((size_t)L.total, 0);
  std::copy(hp.hdr, hp.hdr + kHdrWords, img.begin());
  for (int64_t k = 0; k < nnz; ++k) {
    img[(size_t)(L.items + 2 * k)] = ci[k];
    img[(size_t)(L.items + 2 * k + 1)] = vv ? __builtin_bit_cast(int32_t, vv[k]) : 0;
  }
  auto put = [&](int64_t off, const int32_t* p, size_t n) { std::copy(p, p + n, img.begin() + off); };
  auto putf = [&](int64_t off, const std::vector<float>& v) {
    for (size_t i = 0; i < v.size(); ++i) img[(size_t)off + i] = __builtin_bit_cast(int32_t, v[i]);
  };
  put(L.units, hp.units.data(), hp.units.size());
  put(L.heavy, hp.heavy.data(), hp.heavy.size());
  put(L.tdesc, hp.tdesc.data(), hp.tdesc.size());
  put(L.tcols, hp.tcols.data(), hp.tcols.size());
  putf(L.tfrag, hp.tfrag);
  put(L.red, hp.red.data(), hp.red.size());
  put(L.trows, hp.trows.data(), hp.trows.size());
  putf(L.dval, hp.dval);
  for (int64_t u = 0; u < L.nhunits && L.segp > 0; ++u) {
    const int32_t r = hp.units[(size_t)(4 * u)], b = hp.units[(size_t)(4 * u + 1)], e = hp.units[(size_t)(4 * u + 2)];
    for (int64_t i = 0; i < L.segp; ++i) {
      const size_t o = (size_t)(L.hitems + 2 * (u * L.segp + i));
      const bool in = r >= 0 && b + i < e;
      img[o] = in ? ci[b + i] : -1;
      img[o + 1] = in && vv ? __builtin_bit_cast(int32_t, vv[b + i]) : 0;
    }
  }
}

}  // namespace

// The row-unit + tile plan image for host CSR arrays.
int build_image(const int32_t* rp, const int32_t* ci, const float* vv, int32_t M, int32_t K, int64_t nnz, int32_t ipc,
                int32_t groups, float dense_threshold, std::vector<int32_t>& img) {
  int rc = check_csr(rp, ci, M, K, nnz);
  if (rc) return rc;
  HostPlan hp;
  if ((rc = host_plan(rp, ci, vv, M, K, nnz, ipc, groups, std::fabs(dense_threshold), hp))) return rc;
  classic_image(hp, ci, vv, nnz, img);
  return GCNK_OK;
}

// Bytes of the plan build_image would make, without making it: the size
// follows from its header (no light-row sort, no image).
int64_t plan_size(const int32_t* rp, const int32_t* ci, int32_t M, int32_t K, int64_t nnz, int32_t ipc, int32_t groups,
                  float dense_threshold) {
  int rc = check_csr(rp, ci, M, K, nnz);
  if (rc) return rc;
  HostPlan hp;
  if ((rc = host_plan(rp, ci, nullptr, M, K, nnz, ipc, groups, std::fabs(dense_threshold), hp, false))) return rc;
  return Layout(hp.hdr).total * 4;
}

bool plan_args_ok(const int32_t* rowptr, const int32_t* colind, int32_t M, int32_t K, int64_t nnz, int32_t ipc,
                  int32_t groups) {
  return rowptr && M >= 0 && K >= 0 && nnz >= 0 && nnz < INT32_MAX && ipc > 0 && groups > 0 && (nnz == 0 || colind);
}

}  // namespace gcnk

using namespace gcnk;

// Lane groups per wavefront (64 / LPR): identifies the launch geometry a plan
// is laid out for (heavy segments are shared by these groups, or by the 4
// wavefronts of a workgroup too where RowGeom says so).
extern "C" int32_t gcnk_spmm_groups(int32_t F, int32_t lanes_hint) { return 64 / choose_lpr(F, lanes_hint); }

extern "C" int32_t gcnk_spmm_default_ipc(int32_t M, int64_t nnz, int32_t F, int32_t lanes_hint) {
  (void)M;
  // each lane group's share of a heavy segment (the light-row limit is 2 * ipc
  // at 64 lanes, ipc below).  Narrow groups: 8 (one U = 8 gather batch), but 16
  // for 2-lane groups with workgroup-wide heavy segments.  Whole-wavefront
  // groups: heavy segments of 4 * ipc nonzeros over a 4-wavefront workgroup,
  // sized with the operand so the heavy segments stay a few per CU: ipc ~ nnz /
  // 5760 in [12, 32], a multiple of 4.  (The sweeps: DESIGN.md, "Settled
  // schedule choices".)
  const int lpr = choose_lpr(F, lanes_hint);
  if (lpr != 64) return row_geom(lpr).wg_heavy && lpr == 2 ? 16 : 8;
  int64_t ipc = (nnz / 5760 + 2) / 4 * 4;
  return (int32_t)std::min<int64_t>(32, std::max<int64_t>(12, ipc));
}

extern "C" int64_t gcnk_spmm_plan_bytes_host(const int32_t* rowptr, const int32_t* colind, int32_t M, int32_t K,
                                             int64_t nnz, int32_t ipc, int32_t groups, float dense_threshold) {
  if (!plan_args_ok(rowptr, colind, M, K, nnz, ipc, groups)) {
    set_error("gcnk_spmm_plan_bytes: bad argument");
    return GCNK_EARG;
  }
  return plan_size(rowptr, colind, M, K, nnz, ipc, groups, dense_threshold);
}

extern "C" int gcnk_spmm_plan_build_host(const int32_t* rowptr, const int32_t* colind, const float* val, int32_t M,
                                         int32_t K, int64_t nnz, int32_t ipc, int32_t groups, float dense_threshold,
                                         int32_t* plan, int64_t plan_bytes) {
  if (!plan_args_ok(rowptr, colind, M, K, nnz, ipc, groups) || !plan || (nnz > 0 && !val)) {
    set_error("gcnk_spmm_plan_build_host: bad argument");
    return GCNK_EARG;
  }
  std::vector<int32_t> img;
  const int rc = build_image(rowptr, colind, val, M, K, nnz, ipc, groups, dense_threshold, img);
  if (rc) return rc;
  if (plan_bytes < (int64_t)img.size() * 4) {
    set_error("gcnk_spmm_plan_build_host: plan buffer %lld B < %lld B", (long long)plan_bytes,
              (long long)img.size() * 4);
    return GCNK_EARG;
  }
  std::copy(img.begin(), img.end(), plan);
  return GCNK_OK;
}

extern "C" int64_t gcnk_spmm_workspace_bytes(const int32_t* hdr, int32_t F) {
  if (!plan_magic(hdr) || F < 0) return GCNK_EARG;
  const int64_t ld = ((int64_t)F + 3) & ~3LL;
  const int64_t rows = (int64_t)hdr[kHdrNslots] * ld * 4;
  const int64_t slabs = (int64_t)hdr[kHdrNslabs] * kRB * tile_fpad(F) * 4;
  return ((rows + 255) & ~255LL) + slabs;
}

extern "C" int64_t gcnk_spmm_counter_bytes(const int32_t* hdr) {
  if (!plan_magic(hdr)) return GCNK_EARG;
  return (int64_t)hdr[kHdrNheavy] * kMaxColTiles * 4;
}
