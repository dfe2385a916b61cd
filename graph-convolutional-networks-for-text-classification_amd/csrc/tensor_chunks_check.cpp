// Stand-alone check of tensor_chunks.h for the host compiler and a sanitizer build (make
// chunks-sanitize: -fsanitize=address,undefined, no HIP, no GPU; tests/test_tensor_chunks.py
// builds it plain).  Span and its edge rule are the kernels' own code (one body for host and
// device), so the model below walks every workgroup of a table the way adam_kernel and
// keep_kernel do -- the tensor selected by their loop, 16-B pieces i = tid + T * it, the edge
// lanes, or the scalar loop where head < 0 -- at both kernels' (chunk, threads) and checks:
//   every element of every tensor is moved exactly once, by exactly one workgroup;
//   16-B pieces are 16-B aligned in every buffer, and head is the least that makes them so;
//   first is non-decreasing and first[nt .. MAXT] is the number of chunks;
//   an empty tensor has no chunk, a tensor of at most `head` elements exactly one;
//   append refuses the first chunk past 2^31 - 1.
#include <cstdio>
#include <vector>

#include "tensor_chunks.h"

namespace {
using namespace gcnk::chunks;
constexpr int kMaxT = 8, kPieces = 2;
const int kOff[5] = {0, 4, 8, 12, 1};

struct Fail {};
void require(bool ok, const char* what, int chunk, int combo, int i) {
  if (ok) return;
  std::fprintf(stderr, "FAIL chunk %d offsets #%d tensor %d: %s\n", chunk, combo, i, what);
  throw Fail();
}

// tensors `numel` (nt of them), tensor i's buffer b at fake address 4096 * (1 + i * nbuf + b) + off[b]
template <int CHUNK>
void check_table(const int64_t* numel, int nt, const int* off, int nbuf, int combo) {
  constexpr int T = CHUNK / (4 * kPieces);   // adam: 2048 / 256, keep: 8192 / 1024
  auto addr = [&](int i, int b) { return (uintptr_t)4096 * (uintptr_t)(1 + i * nbuf + b) + (uintptr_t)off[b]; };
  Table<kMaxT> tab = {};
  int64_t total = 0;
  for (int i = 0; i < nt; ++i) {
    const void* p[4] = {};
    for (int b = 0; b < nbuf; ++b) p[b] = reinterpret_cast<const void*>(addr(i, b));
    const int32_t head = nbuf == 2 ? head_of({p[0], p[1]}) : head_of({p[0], p[1], p[2], p[3]});
    int32_t want = -1;   // the least h in 0..3 that puts element h on a 16-B boundary in every buffer
    for (int h = 3; h >= 0; --h) {
      bool all = true;
      for (int b = 0; b < nbuf; ++b) all = all && (addr(i, b) + 4 * h) % 16 == 0;
      if (all) want = h;
    }
    require(head == want, "head", CHUNK, combo, i);
    require(append<CHUNK>(tab, i, numel[i], head, total), "append refused", CHUNK, combo, i);
  }
  for (int i = 0; i < kMaxT; ++i) require(tab.first[i] <= tab.first[i + 1], "first decreases", CHUNK, combo, i);
  for (int i = nt; i <= kMaxT; ++i) require(tab.first[i] == total, "closing fill", CHUNK, combo, i);
  for (int i = 0; i < nt; ++i) {
    const int32_t n = tab.first[i + 1] - tab.first[i];
    require(numel[i] > 0 || n == 0, "an empty tensor has a chunk", CHUNK, combo, i);
    require(numel[i] == 0 || tab.head[i] < numel[i] || n == 1, "an all-head tensor needs one chunk", CHUNK, combo, i);
  }

  std::vector<std::vector<unsigned char>> moved;
  for (int i = 0; i < nt; ++i) moved.emplace_back((size_t)numel[i], 0);
  for (int32_t blk = 0; blk < (int32_t)total; ++blk) {
    int ti = 0;   // the kernels' selection loop
    for (int i = 1; i < kMaxT; ++i)
      if (blk >= tab.first[i]) ti = i;
    require(ti < nt, "a workgroup selects no tensor", CHUNK, combo, ti);
    const Span<CHUNK> s(blk - tab.first[ti], tab.head[ti], blk < tab.first[kMaxT], numel[ti]);
    auto move = [&](int64_t e) {
      require(e >= 0 && e < numel[ti], "an element outside the tensor", CHUNK, combo, ti);
      moved[ti][(size_t)e] += 1;
    };
    for (int tid = 0; tid < T; ++tid) {
      if (s.head < 0) {
        for (int64_t e = s.e0 + tid; e < s.e1; e += T) move(e);
        continue;
      }
      for (int it = 0; it < kPieces; ++it) {
        const int32_t i4 = tid + T * it;
        if (i4 >= s.n4) continue;
        for (int b = 0; b < nbuf; ++b)
          require((addr(ti, b) + 4 * (uintptr_t)(s.e0 + 4 * (int64_t)i4)) % 16 == 0, "a 16-B piece is not aligned", CHUNK, combo, ti);
        for (int j = 0; j < 4; ++j) move(s.e0 + 4 * (int64_t)i4 + j);
      }
      const int64_t e = s.edge(tid);
      if (e >= 0) move(e);
    }
  }
  for (int i = 0; i < nt; ++i)
    for (unsigned char c : moved[i]) require(c == 1, "an element moved never or twice", CHUNK, combo, i);
}

template <int CHUNK>
int check_chunk() {
  const int64_t C = CHUNK;
  const int64_t numels[9] = {0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 7};
  int tables = 0;
  for (int nbuf : {2, 4}) {
    int ncombo = 1;
    for (int b = 0; b < nbuf; ++b) ncombo *= 5;
    for (int combo = 0; combo < ncombo; ++combo) {
      int off[4];
      for (int b = 0, c = combo; b < nbuf; ++b, c /= 5) off[b] = kOff[c % 5];
      // eight of the nine sizes, every rotation for two buffers, one (moving with the offsets) for four
      for (int r = 0; r < 9; ++r) {
        if (nbuf == 4 && r != combo % 9) continue;
        int64_t n[kMaxT];
        for (int i = 0; i < kMaxT; ++i) n[i] = numels[(i + r) % 9];
        check_table<CHUNK>(n, kMaxT, off, nbuf, combo);
        ++tables;
      }
      const int64_t few[3] = {2 * C + 7, 0, 1};   // nt < MAXT: the closing fill is what ends tensor 2
      check_table<CHUNK>(few, 3, off, nbuf, combo);
      ++tables;
    }
  }
  // a launch of empty tensors only: its one workgroup has no work
  Table<kMaxT> tab = {};
  int64_t total = 0;
  require(append<CHUNK>(tab, 0, 0, 0, total) && total == 0, "empty tensor", CHUNK, -1, 0);
  const Span<CHUNK> s(0, tab.head[0], 0 < tab.first[kMaxT], 0);
  require(!s.work && s.len == 0 && s.n4 == 0, "span without work", CHUNK, -1, 0);
  // the 2^31 guard
  total = 0;
  require(append<CHUNK>(tab, 0, C * (int64_t)INT32_MAX, 0, total) && total == INT32_MAX, "2^31 - 1 chunks", CHUNK, -1, 0);
  require(!append<CHUNK>(tab, 1, 1, 0, total), "2^31 chunks accepted", CHUNK, -1, 1);
  return tables;
}
}  // namespace

int main() {
  try {
    const int a = check_chunk<2048>(), k = check_chunk<8192>();
    std::printf("tensor_chunks_check: %d + %d tables ok\n", a, k);
  } catch (const Fail&) {
    return 1;
  }
  return 0;
}
