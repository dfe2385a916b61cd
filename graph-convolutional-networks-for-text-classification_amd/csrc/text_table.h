// The vocabulary table of the word counter, stated once for the host builder (text_table.cpp), the kernels
// (text_count.hip) and the C-ABI comment (include/gcnk_text.h, which says the same in words).  Plain C++: no HIP
// header needed.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define GCNK_TEXT_HD __host__ __device__
#else
#define GCNK_TEXT_HD
#endif

namespace gcnk {

// Thread-local error text returned by gcnk_last_error() (abi.cpp).
void set_error(const char* fmt, ...);

namespace text {

constexpr uint32_t kMagic = 0x54584b47u;   // "GKXT"
constexpr uint32_t kEmpty = 0xffffffffu;   // the word id of an empty slot
constexpr uint32_t kFnvBasis = 2166136261u, kFnvPrime = 16777619u;
constexpr int32_t kMaxWords = 1 << 29;     // slots = 2^30 at most: slot indices and 8-byte slot offsets stay in 32 / 64 bits
enum : int { kHdrMagic = 0, kHdrV, kHdrSlots, kHdrMaxWord, kHdrBlobBytes, kHdrWords = 8 };

// one byte of 32-bit FNV-1a
GCNK_TEXT_HD inline uint32_t fnv1a_step(uint32_t h, uint32_t byte) { return (h ^ byte) * kFnvPrime; }

// the ten ASCII bytes Python's \s matches on str
GCNK_TEXT_HD inline bool is_space(uint32_t c) { return c == 0x20u || c - 0x09u <= 4u || c - 0x1cu <= 3u; }

// the least power of two >= 2 V, at least 4 (V in 1 .. kMaxWords)
GCNK_TEXT_HD inline uint32_t slots_for(int32_t V) {
  uint32_t s = 4;
  while (s < 2u * (uint32_t)V) s <<= 1;
  return s;
}

// byte offsets of the table's parts, and its size
struct Layout {
  int64_t slots, offsets, blob, total;
  GCNK_TEXT_HD Layout(uint32_t nslots, int32_t V, int64_t blob_bytes) {
    slots = 4 * kHdrWords;
    offsets = slots + 8 * (int64_t)nslots;
    blob = offsets + 4 * ((int64_t)V + 1);
    total = (blob + blob_bytes + 7) & ~(int64_t)7;
  }
};

// The refusals of (V, blob_bytes) that the builder and the counter share -> GCNK_OK or the code, the reason set.
int check_sizes(const char* who, int32_t V, int64_t blob_bytes);

}  // namespace text
}  // namespace gcnk
