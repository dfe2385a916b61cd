// Stand-alone check of the vocabulary table builder (text_table.cpp) for the host compiler and a sanitizer build
// (make table-sanitize: -fsanitize=address,undefined, no HIP, no GPU).  The tables are built into heap blocks of
// exactly gcnk_text_table_bytes, at an odd address too, so a write past either end is the sanitizer's to see, and
// are then read back by a model of the lookup that include/gcnk_text.h describes:
//   every word is found under its own id, by hash AND bytes, within `slots` probes; a prefix, an extension and a
//   case variant of a word are not found; words of equal hash ("costarring" / "liquid") keep their own ids;
//   slots, sizes, the header and the longest word are what the header says; known FNV-1a answers;
//   an empty word, a duplicate, V < 1, offsets that do not span the blob and a wrong table size are refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gcnk.h"
#include "text_table.h"

namespace {
using namespace gcnk::text;

struct Fail {};
void require(bool ok, const char* what, int at = -1) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (%d): %s\n", what, at, gcnk_last_error());
  throw Fail();
}

uint32_t fnv(const std::string& s) {
  uint32_t h = kFnvBasis;
  for (unsigned char c : s) h = fnv1a_step(h, c);
  return h;
}

struct Packed {
  std::vector<uint8_t> blob;
  std::vector<int64_t> off;
  explicit Packed(const std::vector<std::string>& words) : off(1, 0) {
    for (const auto& w : words) {
      blob.insert(blob.end(), w.begin(), w.end());
      off.push_back((int64_t)blob.size());
    }
    if (blob.empty()) blob.push_back(0);   // (a pointer to hand over)
  }
};

uint32_t word32(const uint8_t* t, int64_t at) {
  uint32_t v;
  std::memcpy(&v, t + at, 4);
  return v;
}

// the lookup of gcnk_text.h on a built table: the word id, or kEmpty
uint32_t find(const uint8_t* t, const std::string& tok) {
  const uint32_t V = word32(t, 4 * kHdrV), nslots = word32(t, 4 * kHdrSlots);
  const Layout L(nslots, (int32_t)V, word32(t, 4 * kHdrBlobBytes));
  const uint32_t h = fnv(tok);
  for (uint32_t n = 0, s = h & (nslots - 1); n < nslots; ++n, s = (s + 1) & (nslots - 1)) {
    const uint32_t sh = word32(t, L.slots + 8 * (int64_t)s), id = word32(t, L.slots + 8 * (int64_t)s + 4);
    if (id == kEmpty) return kEmpty;
    if (sh != h) continue;
    const uint32_t b = word32(t, L.offsets + 4 * (int64_t)id), e = word32(t, L.offsets + 4 * ((int64_t)id + 1));
    if (e - b == tok.size() && std::memcmp(t + L.blob + b, tok.data(), tok.size()) == 0) return id;
  }
  return kEmpty;
}

int build(const std::vector<std::string>& words, std::vector<uint8_t>* out, int shift = 0) {
  const Packed p(words);
  const int32_t V = (int32_t)words.size();
  const int64_t bytes = gcnk_text_table_bytes(p.off.back(), V);
  if (bytes < 0) return (int)bytes;
  // exactly `bytes` on the heap, `shift` bytes into the block: the builder takes any alignment
  uint8_t* raw = static_cast<uint8_t*>(std::malloc((size_t)bytes + (size_t)shift));
  const int rc = gcnk_text_table_build(p.blob.data(), p.off.back(), p.off.data(), V, raw + shift, bytes);
  out->assign(raw + shift, raw + shift + bytes);
  std::free(raw);
  return rc;
}

int check_words(const std::vector<std::string>& words, int shift) {
  std::vector<uint8_t> t;
  require(build(words, &t, shift) == GCNK_OK, "build");
  const int32_t V = (int32_t)words.size();
  uint32_t want_slots = 4;
  size_t longest = 0, blob = 0;
  while (want_slots < 2u * (uint32_t)V) want_slots *= 2;
  for (const auto& w : words) longest = w.size() > longest ? w.size() : longest, blob += w.size();
  require(word32(t.data(), 0) == kMagic && word32(t.data(), 4) == (uint32_t)V, "header");
  require(word32(t.data(), 8) == want_slots && gcnk_text_table_slots(V) == (int32_t)want_slots, "slots");
  require(word32(t.data(), 12) == longest && word32(t.data(), 16) == blob, "longest word / blob bytes");
  require((int64_t)t.size() == (int64_t)((32 + 8 * (size_t)want_slots + 4 * ((size_t)V + 1) + blob + 7) / 8 * 8), "size");
  uint32_t used = 0;
  for (uint32_t s = 0; s < want_slots; ++s) used += word32(t.data(), 32 + 8 * (int64_t)s + 4) != kEmpty;
  require(used == (uint32_t)V, "a slot per word");
  for (int32_t w = 0; w < V; ++w) {
    require(find(t.data(), words[w]) == (uint32_t)w, "a word is not found under its id", w);
    const std::string longer = words[w] + "s", shorter = words[w].substr(0, words[w].size() - 1);
    std::string upper = words[w];
    upper[0] = (char)(upper[0] ^ 0x20);
    for (const std::string& other : {longer, shorter, upper}) {
      bool is_word = false;
      for (const auto& x : words) is_word = is_word || x == other;
      require(is_word || find(t.data(), other) == kEmpty, "a string that is no word is found", w);
    }
  }
  return V;
}

void refused(const std::vector<std::string>& words, int code, const char* what) {
  std::vector<uint8_t> t;
  require(build(words, &t) == code, what);
  require(std::strstr(gcnk_last_error(), "gcnk_text_table") != nullptr, "the refusal names its entry point");
}
}  // namespace

int main() {
  try {
    require(fnv("") == 0x811c9dc5u && fnv("a") == 0xe40c292cu && fnv("foobar") == 0xbf9cf968u, "FNV-1a known answers");
    require(fnv("costarring") == fnv("liquid") && fnv("declinate") == fnv("macallums"), "the colliding pairs collide");
    int words = 0;
    std::vector<std::string> many;
    for (int i = 0; i < 3000; ++i) many.push_back("w" + std::to_string(i * 7919 % 3001) + (i % 3 ? "" : "\xc3\xa9"));
    const std::vector<std::vector<std::string>> vocabularies = {
        {"oil"}, {"oil", "price"}, {"a", "b", "c"}, {"costarring", "liquid", "declinate", "macallums", "oil"},
        {"caf\xc3\xa9", "cafe", std::string("nul\0in", 6), "del\x7fin", "Oil", "oil", "OIL"}, many};
    for (const auto& v : vocabularies)
      for (int shift : {0, 1, 3}) words += check_words(v, shift);
    refused({}, GCNK_EARG, "an empty vocabulary is accepted");
    refused({"oil", ""}, GCNK_EARG, "an empty word is accepted");
    refused({"", "oil"}, GCNK_EARG, "an empty first word is accepted");
    refused({"oil", "price", "oil"}, GCNK_EARG, "a duplicate word is accepted");
    refused({"liquid", "costarring", "liquid"}, GCNK_EARG, "a duplicate behind a colliding word is accepted");
    // offsets that do not span the blob, a wrong size, null pointers
    const Packed p({"oil", "price"});
    std::vector<uint8_t> t((size_t)gcnk_text_table_bytes(8, 2) + 8);
    int64_t off[3] = {0, 3, 8};
    require(gcnk_text_table_build(p.blob.data(), 8, off, 2, t.data(), (int64_t)t.size() - 8) == GCNK_OK, "plain build");
    require(gcnk_text_table_build(p.blob.data(), 8, off, 2, t.data(), (int64_t)t.size()) == GCNK_EARG, "a wrong table size");
    require(gcnk_text_table_build(p.blob.data(), 8, off, 2, nullptr, (int64_t)t.size() - 8) == GCNK_EARG, "a null table");
    require(gcnk_text_table_build(nullptr, 8, off, 2, t.data(), (int64_t)t.size() - 8) == GCNK_EARG, "a null blob");
    require(gcnk_text_table_build(p.blob.data(), 8, nullptr, 2, t.data(), (int64_t)t.size() - 8) == GCNK_EARG, "null offsets");
    off[0] = 1;
    require(gcnk_text_table_build(p.blob.data(), 8, off, 2, t.data(), (int64_t)t.size() - 8) == GCNK_EARG, "offsets from 1");
    off[0] = 0, off[2] = 7;
    require(gcnk_text_table_build(p.blob.data(), 8, off, 2, t.data(), (int64_t)t.size() - 8) == GCNK_EARG, "offsets short of the blob");
    off[1] = 9, off[2] = 8;
    require(gcnk_text_table_build(p.blob.data(), 8, off, 2, t.data(), (int64_t)t.size() - 8) == GCNK_EARG, "descending offsets");
    require(gcnk_text_table_bytes(8, 0) == GCNK_EARG && gcnk_text_table_bytes(-1, 2) == GCNK_EARG, "sizes of no vocabulary");
    require(gcnk_text_table_bytes((int64_t)1 << 31, 2) == GCNK_EUNSUP && gcnk_text_table_slots((1 << 29) + 1) == GCNK_EUNSUP,
            "sizes past the table's");
    require(gcnk_text_table_slots(1) == 4 && gcnk_text_table_slots(2) == 4 && gcnk_text_table_slots(3) == 8 &&
                gcnk_text_table_slots(1 << 29) == (1 << 30), "slots");
    std::printf("text_table_check: %d words ok\n", words);
  } catch (const Fail&) {
    return 1;
  }
  return 0;
}
