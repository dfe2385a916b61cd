// Host builder of the word counter's vocabulary table (text_count.hip reads it; format: text_table.h and
// include/gcnk_text.h).  Plain C++, no device: builds with any host compiler.
#include "text_table.h"

#include <cstring>

#include "../../include/gcnk.h"

namespace gcnk {
namespace text {

int check_sizes(const char* who, int32_t V, int64_t blob_bytes) {
  if (V < 1 || blob_bytes < 0) {
    set_error("%s: a vocabulary of %d words in %lld bytes (at least one word is needed)", who, V, (long long)blob_bytes);
    return GCNK_EARG;
  }
  if (V > kMaxWords || blob_bytes >= ((int64_t)1 << 31)) {
    set_error("%s: %d words in %lld bytes exceed the table's 2^29 words / 2^31 bytes", who, V, (long long)blob_bytes);
    return GCNK_EUNSUP;
  }
  return GCNK_OK;
}

}  // namespace text
}  // namespace gcnk

using namespace gcnk;
using namespace gcnk::text;

extern "C" int32_t gcnk_text_table_slots(int32_t V) {
  const int rc = check_sizes("gcnk_text_table_slots", V, 0);
  return rc ? rc : (int32_t)slots_for(V);
}

extern "C" int64_t gcnk_text_table_bytes(int64_t blob_bytes, int32_t V) {
  const int rc = check_sizes("gcnk_text_table_bytes", V, blob_bytes);
  return rc ? rc : Layout(slots_for(V), V, blob_bytes).total;
}

extern "C" int gcnk_text_table_build(const uint8_t* blob, int64_t blob_bytes, const int64_t* word_offsets, int32_t V,
                                     void* table, int64_t table_bytes) {
  const char* who = "gcnk_text_table_build";
  if (!blob || !word_offsets || !table) {
    set_error("%s: null pointer", who);
    return GCNK_EARG;
  }
  if (const int rc = check_sizes(who, V, blob_bytes)) return rc;
  const uint32_t nslots = slots_for(V), mask = nslots - 1;
  const Layout L(nslots, V, blob_bytes);
  if (table_bytes != L.total) {
    set_error("%s: table of %lld B, gcnk_text_table_bytes gives %lld B", who, (long long)table_bytes, (long long)L.total);
    return GCNK_EARG;
  }
  if (word_offsets[0] != 0 || word_offsets[V] != blob_bytes) {
    set_error("%s: word_offsets run from %lld to %lld, not from 0 to blob_bytes = %lld", who, (long long)word_offsets[0],
              (long long)word_offsets[V], (long long)blob_bytes);
    return GCNK_EARG;
  }
  for (int32_t w = 0; w < V; ++w) {
    if (word_offsets[w + 1] <= word_offsets[w] || word_offsets[w + 1] > blob_bytes) {
      set_error("%s: word %d is empty or its offsets do not ascend within the blob (%lld .. %lld)", who, w,
                (long long)word_offsets[w], (long long)word_offsets[w + 1]);
      return GCNK_EARG;
    }
  }
  uint8_t* out = static_cast<uint8_t*>(table);
  std::memset(out, 0, (size_t)L.total);
  // (filled through memcpy: `table` need not be aligned on the host)
  auto put = [&](int64_t at, uint32_t v) { std::memcpy(out + at, &v, 4); };
  auto get = [&](int64_t at) { uint32_t v; std::memcpy(&v, out + at, 4); return v; };
  for (uint32_t s = 0; s < nslots; ++s) put(L.slots + 8 * (int64_t)s + 4, kEmpty);
  int64_t longest = 0;
  for (int32_t w = 0; w < V; ++w) {
    const int64_t b = word_offsets[w], len = word_offsets[w + 1] - b;
    longest = len > longest ? len : longest;
    uint32_t h = kFnvBasis;
    for (int64_t i = 0; i < len; ++i) h = fnv1a_step(h, blob[b + i]);
    uint32_t s = h & mask;
    for (;; s = (s + 1) & mask) {   // (slots >= 2 V: an empty slot is always met)
      const uint32_t id = get(L.slots + 8 * (int64_t)s + 4);
      if (id == kEmpty) break;
      const int64_t ob = word_offsets[id], olen = word_offsets[id + 1] - ob;
      if (get(L.slots + 8 * (int64_t)s) == h && olen == len && std::memcmp(blob + ob, blob + b, (size_t)len) == 0) {
        set_error("%s: words %u and %d are the same %lld bytes", who, id, w, (long long)len);
        return GCNK_EARG;
      }
    }
    put(L.slots + 8 * (int64_t)s, h);
    put(L.slots + 8 * (int64_t)s + 4, (uint32_t)w);
    put(L.offsets + 4 * (int64_t)w, (uint32_t)b);
  }
  put(L.offsets + 4 * (int64_t)V, (uint32_t)blob_bytes);
  put(4 * kHdrMagic, kMagic);
  put(4 * kHdrV, (uint32_t)V);
  put(4 * kHdrSlots, nslots);
  put(4 * kHdrMaxWord, (uint32_t)longest);
  put(4 * kHdrBlobBytes, (uint32_t)blob_bytes);
  std::memcpy(out + L.blob, blob, (size_t)blob_bytes);
  return GCNK_OK;
}
