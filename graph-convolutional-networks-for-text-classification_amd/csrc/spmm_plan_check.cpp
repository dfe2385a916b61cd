// Stand-alone check of the host planner for a sanitizer build (make plan-sanitize:
// host compiler, -fsanitize=address,undefined, no HIP, no GPU).  Links only
// spmm_plan.cpp and abi.cpp.  It builds the boundary matrices of
// tests/test_plan_host.py (the same integer arithmetic, described there) over
// groups x ipc x dense_threshold and checks that the size query is exactly the
// image: the build into a heap buffer of that size writes its last word (and,
// under AddressSanitizer, nothing past it); a buffer one word short is refused.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/gcnk.h"
#include "spmm_plan.h"

namespace {
using Cols = std::vector<int32_t>;
struct Csr {
  const char* name;
  int32_t K;
  Cols rp, ci;
  std::vector<float> v;
  Csr(const char* name_, int32_t K_, const std::vector<Cols>& rows) : name(name_), K(K_), rp{0} {
    for (const Cols& r : rows) {
      ci.insert(ci.end(), r.begin(), r.end());
      rp.push_back((int32_t)ci.size());
    }
    for (int64_t k = 0; k < (int64_t)ci.size(); ++k) v.push_back((float)((k * 7919) % 1009 - 504) / 64.0f);
  }
};

Cols uniq(Cols v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}
Cols seq(int n, int mul, int add, int mod) {  // (add + mul * j) % mod, j < n
  Cols v;
  for (int j = 0; j < n; ++j) v.push_back((add + mul * j) % mod);
  return v;
}
Cols with(Cols v, int32_t c) {
  v.push_back(c);
  return v;
}
Cols alternating(int n, int half, int mul, int add) {  // unsorted: (j % 2) * half + mul * j + add
  Cols v;
  for (int j = 0; j < n; ++j) v.push_back((j % 2) * half + mul * j + add);
  return v;
}

Csr boundary_rows() {
  const int N = 4096;
  std::vector<Cols> rows{seq(N / 2, 2, 0, N), with(seq(N / 2, 2, 0, N), N - 1)};
  const int degs[] = {8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 64, 65};
  for (int i = 0; i < 12; ++i) rows.push_back(uniq(seq(degs[i], 61, (i + 2) * 37, N)));
  rows.push_back(alternating(300, 2048, 1, 0));
  rows.push_back({});
  for (int r = 16; r < N; ++r) rows.push_back(uniq({r, (r * 7) % N, (r * 13 + 5) % N}));
  return Csr("boundary_rows", N, rows);
}
Csr tile_blocks() {
  std::vector<Cols> rows;
  for (int r = 0; r < 64; ++r) rows.push_back(uniq(with(seq(50, 1, 256, 512), r)));
  for (int r = 64; r < 128; ++r) rows.push_back(uniq(with(seq(200, 1, 128, 512), r)));
  for (int r = 128; r < 192; ++r) rows.push_back(uniq(with(seq(40, 2, 0, 512), r)));
  for (int r = 192; r < 400; ++r) rows.push_back({r});
  rows.resize(512);
  return Csr("tile_blocks", 512, rows);
}
Csr rect_long_row() {
  const int K = 140000;
  return Csr("rect_long_row", K, {seq(K, 1, 0, K), {}, {5, 70000, 139999}, alternating(70, 70000, -3, 207), {0}});
}

bool check(const Csr& c) {
  const int32_t M = (int32_t)c.rp.size() - 1;
  const int64_t nnz = (int64_t)c.ci.size();
  for (int groups : {1, 2, 8, 32, 64})
    for (int ipc : {8, 12, 32})
      for (float dense : {0.25f, 2.0f}) {
        auto build = [&](int32_t* img, int64_t bytes) {
          return gcnk_spmm_plan_build_host(c.rp.data(), c.ci.data(), c.v.data(), M, c.K, nnz, ipc, groups, dense, img, bytes);
        };
        const int64_t nbytes = gcnk_spmm_plan_bytes_host(c.rp.data(), c.ci.data(), M, c.K, nnz, ipc, groups, dense);
        const char* what = "size query";
        if (nbytes >= 64 && nbytes % 4 == 0) {
          Cols img((size_t)(nbytes / 4), -7);  // exactly the reported size: a write past it is AddressSanitizer's
          what = build(img.data(), nbytes) != GCNK_OK ? "build"
                 : !gcnk::plan_magic(img.data()) || img.back() == -7 ? "image shorter than its size"
                 : gcnk::Layout(img.data()).total * 4 != nbytes ? "header disagrees with the size"
                 : build(img.data(), nbytes - 4) != GCNK_EARG ? "a short buffer was accepted"
                 : gcnk_spmm_workspace_bytes(img.data(), 200) < 0 || gcnk_spmm_counter_bytes(img.data()) < 0
                     ? "workspace / counter size" : nullptr;
        }
        if (what) {
          std::fprintf(stderr, "FAIL %s groups %d ipc %d dense %g: %s (%s)\n", c.name, groups, ipc, dense, what,
                       gcnk_last_error());
          return false;
        }
      }
  return true;
}
}  // namespace

int main() {
  const Csr cases[] = {boundary_rows(), tile_blocks(), rect_long_row(), Csr("no_rows", 7, {}),
                       Csr("no_nonzeros", 3, std::vector<Cols>(5))};
  for (const Csr& c : cases)
    if (!check(c)) return 1;
  std::printf("spmm_plan_check: 5 matrices x 30 plans ok\n");
  return 0;
}
