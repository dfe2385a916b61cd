/*
 * gcnk_text.h — the part of libgcnk.so's C-ABI that counts words: sklearn's
 * CountVectorizer.transform of unseen text against a fitted vocabulary.
 * include/gcnk.h includes this file, so a C caller sees one ABI; it is a file
 * of its own in gcnk.h's form (_lib.py reads every public header with the same
 * reader): a header per family.
 */
#ifndef GCNK_TEXT_H_
#define GCNK_TEXT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Counting words on the device (csrc/text_count.hip, csrc/text_table.cpp;
 * additions within ABI 13): CountVectorizer(token_pattern=r'\S+',
 * lowercase=False).transform as the reference configures it
 * (topic_model.py:93-102,159), against a fitted vocabulary, as the sorted
 * CSR (indptr int32 [B+1], indices int32 [nnz] ascending in a row, counts
 * float64 [nnz]) that gcnk_lda_estep_f64 and its kin take.
 *
 * Text.  `bytes` [N] are the documents' UTF-8 bytes one after the other with
 * nothing between them; document d is bytes[offsets[d] .. offsets[d+1]),
 * offsets int64 [B+1] on the device, ascending, offsets[0] >= 0, offsets[B] <=
 * N (an offset outside [0, N] is clamped into it and a descending pair reads as
 * an empty document: no load ever leaves [0, N)).  A token is a maximal run,
 * inside one document, of bytes outside {0x09..0x0D, 0x1C..0x1F, 0x20}, the
 * ASCII characters Python's \s matches; every other byte, 0x00, 0x7F and >=
 * 0x80 included, is a token byte.  A token counts iff its bytes equal a
 * vocabulary word's bytes.  (The 19 non-ASCII code points of \s are the
 * caller's: text_count.py maps them to a space before it encodes.)
 *
 * The vocabulary table (host, text_table.cpp; built once per vocabulary and
 * uploaded as it is).  Words are `blob` [blob_bytes], word w the bytes
 * blob[word_offsets[w] .. word_offsets[w+1]), word_offsets int64 [V+1] with
 * word_offsets[0] = 0 and word_offsets[V] = blob_bytes.  The table, in
 * little-endian 32-bit words unless said otherwise:
 *     header   8 words: 0x54584b47 ("GKXT"), V, slots, max_word_bytes (the
 *              longest word), blob_bytes, 0, 0, 0
 *     slots    `slots` pairs {hash, word id}; an empty slot is {0, 0xffffffff}
 *     offsets  V + 1 words: word_offsets
 *     blob     blob_bytes bytes, then zero bytes up to a multiple of 8
 * so gcnk_text_table_bytes = 32 + 8 slots + 4 (V + 1) + blob_bytes rounded up
 * to 8.  slots = gcnk_text_table_slots(V): the least power of two >= 2 V, at
 * least 4.  hash = 32-bit FNV-1a of the word's bytes: h = 2166136261, then for
 * each byte h = (h ^ byte) * 16777619 mod 2^32.  Words are inserted in id
 * order, word w into the first empty slot of (hash + i) mod slots, i = 0, 1,
 * ...  A lookup walks the same slots until the empty one and takes slot s iff
 * its hash is the token's AND the word's length is the token's AND every byte
 * is equal: a hash match alone is never a match.  A token longer than
 * max_word_bytes is dropped unhashed.
 *   gcnk_text_table_build refuses (GCNK_EARG) V < 1, an empty or a duplicate
 *   word, offsets that do not ascend from 0 to blob_bytes, a table_bytes other
 *   than gcnk_text_table_bytes, and (GCNK_EUNSUP) blob_bytes >= 2^31 or V >
 *   2^29.  Host only: no HIP call, no device.
 *
 * Counting is two entry points on one stream with ONE host read between them
 * (indptr[B] = nnz, which sizes the exact outputs); neither synchronises.
 *   gcnk_text_count   a wave per document walks it in 64-byte pieces: a ballot
 *       of the token bytes gives the token starts (the piece before carries
 *       its last bit; a document starts with none), the lane of a token start
 *       hashes its token to the end and probes the table.  A counted token at
 *       byte p of document d stores the key d << vbits | word id into key slot
 *       (p + d) / 2 of gcnk_text_token_bound(N, B) = (N + B) / 2 + 1 slots that
 *       were filled with ones (two token starts are two bytes apart, and a
 *       document apart too when in different documents).  vbits: the bits of V
 *       - 1, at least 1.  The keys go through hipCUB's radix sort over the
 *       bits in use, a run-length pass marks each run's first key, an
 *       inclusive scan numbers the runs, and indptr[d] is the number of the
 *       first run of a document >= d (a binary search per row).  Every step is
 *       deterministic: no atomics, integers alone.
 *   gcnk_text_emit    indices[j] and counts[j] = the length of run j, from the
 *       workspace gcnk_text_count left, for the nnz the host read.
 * GCNK_EARG: a null pointer (bytes may be null when N = 0, indices and counts
 * when nnz = 0), N < 0, B < 0, V < 1, a table that is not 8-byte aligned, a
 * slots / table_bytes that is not what V and blob_bytes give, max_word_bytes <
 * 1, nnz < 0 or nnz above the token bound, a workspace smaller than
 * gcnk_text_workspace_bytes(N, B, V).  GCNK_EUNSUP: N + B >= 2^32 - 2 (a token
 * bound of 2^31 or more, and with it nnz), V > 2^29.  Every refusal comes
 * before any HIP call, with its reason in gcnk_last_error.  B = 0 or N = 0
 * writes a zero indptr and needs no workspace.
 * ------------------------------------------------------------------------- */
int32_t gcnk_text_table_slots(int32_t V);
int64_t gcnk_text_table_bytes(int64_t blob_bytes, int32_t V);
int gcnk_text_table_build(const uint8_t* blob, int64_t blob_bytes, const int64_t* word_offsets, int32_t V, void* table,
                          int64_t table_bytes);
int64_t gcnk_text_token_bound(int64_t N, int32_t B);
int64_t gcnk_text_workspace_bytes(int64_t N, int32_t B, int32_t V);
int gcnk_text_count(const uint8_t* bytes, int64_t N, const int64_t* offsets, int32_t B, const void* table,
                    int64_t table_bytes, int32_t V, int32_t slots, int32_t max_word_bytes, int64_t blob_bytes,
                    int32_t* indptr, void* workspace, int64_t workspace_bytes, void* stream);
int gcnk_text_emit(int64_t N, int32_t B, int32_t V, int64_t nnz, int32_t* indices, double* counts,
                   const void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GCNK_TEXT_H_ */
