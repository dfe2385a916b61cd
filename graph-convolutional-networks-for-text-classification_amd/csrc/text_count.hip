// Counting words on the device: CountVectorizer(token_pattern=r'\S+', lowercase=False).transform against a fitted
// vocabulary (include/gcnk_text.h states the text, the table and the result; text_table.h the table's layout).
//
//   tokens   a wave per document, 64 bytes a step: a ballot of the token bytes gives the token starts, the lane of
//            a start hashes its token (FNV-1a) to its end and probes the table, byte for byte; a counted token
//            stores its key  document << vbits | word  into the key slot (byte + document) / 2, which no other
//            token start can have
//   sort     hipCUB's radix sort of the key slots over the bits in use (an empty slot, all ones, sorts last)
//   runs     a run's first key is marked, an inclusive scan numbers the runs, each run's first position is kept
//   rows     indptr[d] by a binary search for the first key of a document >= d
//   emit     (after the host read nnz) indices and counts from the runs' positions
// Integers alone, no atomics: the result does not depend on the order anything ran in.
#include <hipcub/hipcub.hpp>

#include "gcnk_common.h"
#include "text_table.h"

namespace gcnk {
namespace {

using namespace text;

constexpr int kWaves = 4;                       // documents a workgroup of 256 takes
constexpr uint64_t kNoKey = ~(uint64_t)0;       // an empty key slot

struct Table {   // the device table's parts (Layout) and the sizes the host states
  const uint2* slots;
  const uint32_t* offsets;
  const uint8_t* blob;
  uint32_t mask, V, max_word, blob_bytes;
};

inline int bits_of(uint64_t x) {   // the bits of x, at least 1
  int b = 1;
  while (b < 63 && (x >> b)) ++b;
  return b;
}

// The word id of the token bytes[p .. p + len) with hash h, or kEmpty.
__device__ __forceinline__ uint32_t lookup(const Table& t, const uint8_t* __restrict__ bytes, int64_t p, uint32_t len,
                                           uint32_t h) {
  uint32_t s = h & t.mask;
  for (uint32_t n = 0; n <= t.mask; ++n, s = (s + 1) & t.mask) {
    const uint2 slot = t.slots[s];   // {hash, word id}
    if (slot.y == kEmpty) return kEmpty;
    if (slot.x != h || slot.y >= t.V) continue;
    const uint32_t b = t.offsets[slot.y], e = t.offsets[slot.y + 1];
    if (e < b || e > t.blob_bytes || e - b != len) continue;   // (a damaged table reads nothing outside the blob)
    uint32_t i = 0;
    while (i < len && t.blob[b + i] == bytes[p + i]) ++i;
    if (i == len) return slot.y;
  }
  return kEmpty;
}

__global__ void __launch_bounds__(64 * kWaves) text_tokens_kernel(const uint8_t* __restrict__ bytes, int64_t N,
                                                                  const int64_t* __restrict__ offsets, int32_t B,
                                                                  Table t, int vbits, uint64_t* __restrict__ keys,
                                                                  int64_t nkeys) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (d >= B) return;   // (wave-uniform)
  int64_t lo = offsets[d], hi = offsets[d + 1];
  lo = lo < 0 ? 0 : (lo > N ? N : lo);
  hi = hi < lo ? lo : (hi > N ? N : hi);
  uint64_t carry = 0;   // the piece before ended inside a token
  for (int64_t base = lo; base < hi; base += 64) {
    const int64_t p = base + lane;
    const uint32_t c = p < hi ? bytes[p] : 0x20u;
    const uint64_t tok = __ballot(!is_space(c));
    const uint64_t starts = tok & ~((tok << 1) | carry);
    carry = tok >> 63;
    if ((starts >> lane) & 1) {   // (the wave meets again before the next ballot)
      // this lane's token: hashed to its end, given up once it is longer than every word
      uint32_t h = fnv1a_step(kFnvBasis, c), len = 1;
      for (int64_t q = p + 1; q < hi && len <= t.max_word; ++q) {
        const uint32_t cq = bytes[q];
        if (is_space(cq)) break;
        h = fnv1a_step(h, cq);
        ++len;
      }
      const uint32_t id = len <= t.max_word ? lookup(t, bytes, p, len, h) : kEmpty;
      const int64_t at = (p + d) >> 1;
      if (id != kEmpty && at < nkeys) keys[at] = ((uint64_t)d << vbits) | id;
    }
  }
}

__global__ void __launch_bounds__(256) text_heads_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                         int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  head[i] = k != kNoKey && (i == 0 || k != keys[i - 1]);
}

// first[j] = the position of run j's first key, first[runs] = the number of keys
__global__ void __launch_bounds__(256) text_runs_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                        const int32_t* __restrict__ head,
                                                        const int32_t* __restrict__ run, int32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || keys[i] == kNoKey) return;
  if (head[i]) first[run[i] - 1] = (int32_t)i;
  if (i == n - 1 || keys[i + 1] == kNoKey) first[run[i]] = (int32_t)(i + 1);
}

__global__ void __launch_bounds__(256) text_rows_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                        const int32_t* __restrict__ run, int32_t B, int vbits,
                                                        int32_t* __restrict__ indptr) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d > B) return;
  const uint64_t want = (uint64_t)d << vbits;   // (below kNoKey: d <= B < 2^31, vbits <= 30)
  int64_t lo = 0, hi = n;                       // the first key >= want
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  indptr[d] = lo ? run[lo - 1] : 0;
}

__global__ void __launch_bounds__(256) text_emit_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                        const int32_t* __restrict__ first, int64_t nnz, int vbits,
                                                        int32_t* __restrict__ indices, double* __restrict__ counts) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nnz) return;
  const int64_t i = first[j], e = first[j + 1];
  const bool ok = i >= 0 && i < n && e > i && e <= n;   // (an nnz the count did not give reads nothing outside)
  indices[j] = ok ? (int32_t)(keys[i] & (((uint64_t)1 << vbits) - 1)) : 0;
  counts[j] = ok ? (double)(e - i) : 0.0;
}

// The workspace: byte offsets of its parts for (N, B, V), and the sort's bits.
struct Ws {
  int64_t nkeys, keys_in, keys_out, head, run, first, tmp, total;
  size_t tmp_bytes;
  int vbits, bits;
  Ws(int64_t N, int32_t B, int32_t V) {
    auto a = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    nkeys = (N + B) / 2 + 1;
    vbits = bits_of((uint64_t)V - 1);
    bits = vbits + bits_of((uint64_t)B);   // (document B's keys would be the first past the last: an empty slot's bits)
    size_t sort_b = 0, scan_b = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, sort_b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)nkeys,
                                            0, bits);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, scan_b, (const int32_t*)nullptr, (int32_t*)nullptr, (int)nkeys);
    tmp_bytes = sort_b > scan_b ? sort_b : scan_b;
    keys_in = 0;
    keys_out = keys_in + a(nkeys * 8);
    head = keys_out + a(nkeys * 8);
    run = head + a(nkeys * 4);
    first = run + a(nkeys * 4);
    tmp = first + a((nkeys + 1) * 4);
    total = tmp + a((int64_t)tmp_bytes);
  }
};

// The refusals of (N, B, V) every entry point here shares.
int check_shape(const char* who, int64_t N, int32_t B, int32_t V) {
  if (N < 0 || B < 0) {
    set_error("%s: N = %lld bytes in B = %d documents", who, (long long)N, B);
    return GCNK_EARG;
  }
  if (const int rc = check_sizes(who, V, 0)) return rc;
  if (N + (int64_t)B >= ((int64_t)1 << 32) - 2) {
    set_error("%s: N + B = %lld gives a token bound of 2^31 or more (an int32 CSR holds fewer)", who,
              (long long)(N + (int64_t)B));
    return GCNK_EUNSUP;
  }
  return GCNK_OK;
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int64_t gcnk_text_token_bound(int64_t N, int32_t B) {
  const int rc = check_shape("gcnk_text_token_bound", N, B, 1);
  return rc ? rc : (N + B) / 2 + 1;
}

extern "C" int64_t gcnk_text_workspace_bytes(int64_t N, int32_t B, int32_t V) {
  const int rc = check_shape("gcnk_text_workspace_bytes", N, B, V);
  return rc ? rc : Ws(N, B, V).total;
}

extern "C" int gcnk_text_count(const uint8_t* bytes, int64_t N, const int64_t* offsets, int32_t B, const void* table,
                               int64_t table_bytes, int32_t V, int32_t slots, int32_t max_word_bytes,
                               int64_t blob_bytes, int32_t* indptr, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  const char* who = "gcnk_text_count";
  if (const int rc = check_shape(who, N, B, V)) return rc;
  if (const int rc = check_sizes(who, V, blob_bytes)) return rc;
  if (!offsets || !table || !indptr || (N > 0 && !bytes)) {
    set_error("%s: null pointer", who);
    return GCNK_EARG;
  }
  const Layout L(slots_for(V), V, blob_bytes);
  if ((reinterpret_cast<uintptr_t>(table) & 7u) || slots != (int32_t)slots_for(V) || table_bytes != L.total ||
      max_word_bytes < 1 || max_word_bytes > blob_bytes) {
    set_error("%s: the table (%lld B at %p, %d slots, longest word %d B) is not gcnk_text_table_build's for V = %d and "
              "blob_bytes = %lld: 8-byte aligned, %lld B, %u slots", who, (long long)table_bytes, table, slots,
              max_word_bytes, V, (long long)blob_bytes, (long long)L.total, slots_for(V));
    return GCNK_EARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (B == 0 || N == 0) return hip_check(hipMemsetAsync(indptr, 0, ((size_t)B + 1) * 4, s), "text_count memset");
  const Ws W(N, B, V);
  if (!workspace || workspace_bytes < W.total) {
    set_error("%s: workspace %lld B < %lld B", who, (long long)workspace_bytes, (long long)W.total);
    return GCNK_EARG;
  }
  char* w = (char*)workspace;
  uint64_t* keys_in = (uint64_t*)(w + W.keys_in);
  uint64_t* keys = (uint64_t*)(w + W.keys_out);
  int32_t* head = (int32_t*)(w + W.head);
  int32_t* run = (int32_t*)(w + W.run);
  int32_t* first = (int32_t*)(w + W.first);
  const char* tb = (const char*)table;
  const Table t = {(const uint2*)(tb + L.slots), (const uint32_t*)(tb + L.offsets), (const uint8_t*)(tb + L.blob),
                   (uint32_t)slots - 1, (uint32_t)V, (uint32_t)max_word_bytes, (uint32_t)blob_bytes};
  int rc = hip_check(hipMemsetAsync(keys_in, 0xff, (size_t)W.nkeys * 8, s), "text_count key fill");
  if (rc) return rc;
  hipLaunchKernelGGL(text_tokens_kernel, dim3(blocks((int64_t)B * 64)), dim3(64 * kWaves), 0, s, bytes, N, offsets, B,
                     t, W.vbits, keys_in, W.nkeys);
  if ((rc = launch_check("text_tokens_kernel"))) return rc;
  size_t tmp_bytes = W.tmp_bytes;
  rc = hip_check(hipcub::DeviceRadixSort::SortKeys(w + W.tmp, tmp_bytes, keys_in, keys, (int)W.nkeys, 0, W.bits, s),
                 "text_count radix sort");
  if (rc) return rc;
  hipLaunchKernelGGL(text_heads_kernel, dim3(blocks(W.nkeys)), dim3(256), 0, s, keys, W.nkeys, head);
  if ((rc = launch_check("text_heads_kernel"))) return rc;
  tmp_bytes = W.tmp_bytes;
  rc = hip_check(hipcub::DeviceScan::InclusiveSum(w + W.tmp, tmp_bytes, head, run, (int)W.nkeys, s), "text_count scan");
  if (rc) return rc;
  hipLaunchKernelGGL(text_runs_kernel, dim3(blocks(W.nkeys)), dim3(256), 0, s, keys, W.nkeys, head, run, first);
  if ((rc = launch_check("text_runs_kernel"))) return rc;
  hipLaunchKernelGGL(text_rows_kernel, dim3(blocks((int64_t)B + 1)), dim3(256), 0, s, keys, W.nkeys, run, B, W.vbits,
                     indptr);
  return launch_check("text_rows_kernel");
}

extern "C" int gcnk_text_emit(int64_t N, int32_t B, int32_t V, int64_t nnz, int32_t* indices, double* counts,
                              const void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "gcnk_text_emit";
  if (const int rc = check_shape(who, N, B, V)) return rc;
  const int64_t bound = (N + B) / 2 + 1;
  if (nnz < 0 || nnz > bound || (nnz > 0 && (B == 0 || N == 0))) {
    set_error("%s: nnz = %lld outside 0 .. the token bound %lld", who, (long long)nnz, (long long)bound);
    return GCNK_EARG;
  }
  if (nnz == 0) return GCNK_OK;
  if (!indices || !counts) {
    set_error("%s: null pointer", who);
    return GCNK_EARG;
  }
  const Ws W(N, B, V);
  if (!workspace || workspace_bytes < W.total) {
    set_error("%s: workspace %lld B < %lld B", who, (long long)workspace_bytes, (long long)W.total);
    return GCNK_EARG;
  }
  const char* w = (const char*)workspace;
  hipLaunchKernelGGL(text_emit_kernel, dim3(blocks(nnz)), dim3(256), 0, (hipStream_t)stream,
                     (const uint64_t*)(w + W.keys_out), W.nkeys, (const int32_t*)(w + W.first), nnz, W.vbits, indices,
                     counts);
  return launch_check("text_emit_kernel");
}
