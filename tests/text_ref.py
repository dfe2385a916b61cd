"""Pure-Python restatement of CountVectorizer(token_pattern=r'\\S+', lowercase=False).transform as
include/gcnk_text.h states it -- bytes and a dictionary in, three arrays out -- and of the header's hash and
vocabulary table.  Written from the header's words alone: nothing here calls the library.  tests/test_text_ref.py
pins it to sklearn's recorded output (tests/golden/text_r8_small.npz) and, where sklearn is installed, to
CountVectorizer.transform itself; the GPU tests take their expected arrays from it.  No GPU."""
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "text_r8_small.npz")

ASCII_SPACE = (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F, 0x20)      # \s on str below 0x80
NON_ASCII_SPACE = (0x85, 0xA0, 0x1680, 0x2000, 0x2001, 0x2002, 0x2003, 0x2004, 0x2005, 0x2006, 0x2007, 0x2008, 0x2009,
                   0x200A, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000)               # \s on str from 0x80 up
_IS_SPACE = bytes(1 if b in ASCII_SPACE else 0 for b in range(256))
MAGIC, EMPTY = 0x54584B47, 0xFFFFFFFF


def encode(texts):
    """texts -> (bytes, offsets [B+1]): a text that is not ASCII has its non-ASCII \\s code points replaced by a
    space, every text is UTF-8, nothing stands between two documents.  UnicodeEncodeError on a lone surrogate."""
    parts = []
    for t in texts:
        if not t.isascii():
            t = "".join(" " if ord(ch) in NON_ASCII_SPACE else ch for ch in t)
        parts.append(t.encode("utf-8"))
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    for i, p in enumerate(parts):
        offsets[i + 1] = offsets[i] + len(p)
    return b"".join(parts), offsets


def tokens(data):
    """The maximal runs of non-white-space bytes of one document's bytes."""
    out, start = [], None
    for i, b in enumerate(data):
        if _IS_SPACE[b]:
            if start is not None:
                out.append(data[start:i])
                start = None
        elif start is None:
            start = i
    if start is not None:
        out.append(data[start:])
    return out


def count(data, offsets, vocabulary):
    """(indptr int32 [B+1], indices int32 [nnz] ascending in a row, counts float64 [nnz]) of the documents
    data[offsets[d] : offsets[d+1]] against ``vocabulary``: {word's UTF-8 bytes: id}."""
    indptr, indices, counts = [0], [], []
    for d in range(len(offsets) - 1):
        row = {}
        for tok in tokens(bytes(data[int(offsets[d]):int(offsets[d + 1])])):
            w = vocabulary.get(tok)
            if w is not None:
                row[w] = row.get(w, 0) + 1
        for w in sorted(row):
            indices.append(w)
            counts.append(float(row[w]))
        indptr.append(len(indices))
    return np.asarray(indptr, np.int32), np.asarray(indices, np.int32), np.asarray(counts, np.float64)


def vocabulary_of(words):
    """{UTF-8 bytes: id} of words (str) in id order."""
    return {w.encode("utf-8"): i for i, w in enumerate(words)}


def transform(texts, words):
    """``count`` of str texts against str words in id order."""
    return count(*encode(texts), vocabulary_of(words))


def fnv1a(data):
    h = 2166136261
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def slots_for(V):
    s = 4
    while s < 2 * V:
        s *= 2
    return s


def table(words):
    """The vocabulary table of gcnk_text.h for ``words`` (bytes, in id order) as a uint8 array: header, slots,
    offsets, blob, zero padding to a multiple of 8."""
    V, slots = len(words), slots_for(len(words))
    blob = b"".join(words)
    pairs = [(0, EMPTY)] * slots
    for w, word in enumerate(words):
        h = fnv1a(word)
        s = h % slots
        while pairs[s][1] != EMPTY:
            s = (s + 1) % slots
        pairs[s] = (h, w)
    offs, at = [], 0
    for word in words:
        offs.append(at)
        at += len(word)
    offs.append(at)
    out = struct.pack("<8I", MAGIC, V, slots, max(len(w) for w in words), len(blob), 0, 0, 0)
    out += b"".join(struct.pack("<2I", *p) for p in pairs)
    out += struct.pack(f"<{V + 1}I", *offs) + blob
    out += b"\0" * (-len(out) % 8)
    return np.frombuffer(out, dtype=np.uint8)


def lookup(tab, token):
    """The word id of ``token`` (bytes) in a table (uint8 array) by the header's rule, or None."""
    raw = tab.tobytes()
    _, V, slots, longest, blob_bytes = struct.unpack_from("<5I", raw, 0)
    at_slots, at_offs = 32, 32 + 8 * slots
    at_blob = at_offs + 4 * (V + 1)
    if len(token) > longest:
        return None
    h = fnv1a(token)
    for i in range(slots):
        sh, w = struct.unpack_from("<2I", raw, at_slots + 8 * ((h + i) % slots))
        if w == EMPTY:
            return None
        b, e = struct.unpack_from("<2I", raw, at_offs + 4 * w)
        if sh == h and raw[at_blob + b:at_blob + e] == token:
            return w
    return None


def colliding_pair():
    """Two distinct ASCII strings with the same 32-bit FNV-1a hash, found by a birthday search over the 10^6
    six-letter strings on a .. j (about 116 pairs are expected; strings of up to four bytes do not collide at all).
    The first pair in sorted hash order is returned."""
    n, length = 10, 6
    h = np.full((n,) * length, 2166136261, dtype=np.uint64)
    for k in range(length):   # letter k varies along axis k
        letters = (np.arange(n, dtype=np.uint64) + np.uint64(ord("a"))).reshape([n if a == k else 1 for a in range(length)])
        h = ((h ^ letters) * np.uint64(16777619)) & np.uint64(0xFFFFFFFF)
    h = h.reshape(-1)
    order = np.argsort(h, kind="stable")
    same = np.nonzero(h[order][1:] == h[order][:-1])[0]
    assert same.size, "no collision among the 10^6 strings"
    word = lambda flat: "".join(chr(ord("a") + int(d)) for d in np.unravel_index(flat, (n,) * length))   # noqa: E731
    a, b = word(order[same[0]]), word(order[same[0] + 1])
    assert a != b and fnv1a(a.encode()) == fnv1a(b.encode())
    return a, b


def golden():
    """The fixture as a dict of arrays, with ``texts`` (the 300 documents) and ``words`` (the vocabulary in id
    order) decoded."""
    z = dict(np.load(GOLDEN))
    data, off = z["text_bytes"].tobytes(), z["text_offsets"]
    z["texts"] = [data[off[i]:off[i + 1]].decode("utf-8") for i in range(len(off) - 1)]
    blob, woff = z["vocab_bytes"].tobytes(), z["vocab_offsets"]
    z["words"] = [blob[woff[i]:woff[i + 1]].decode("utf-8") for i in range(len(woff) - 1)]
    return z


# The adversarial texts of the issue, against ADVERSARIAL_WORDS
ADVERSARIAL_WORDS = ["oil", "price", "caf\u00e9", "a", "nul\0in", "del\x7fin", "prices", "oi", "crude"]
ADVERSARIAL_TEXTS = (
    ["", "   ", "a", " a", "a ", "oil price oil"]
    + [f"oil{chr(b)}price" for b in ASCII_SPACE] + [f"oil{chr(b) * 2}price{chr(b)}" for b in ASCII_SPACE]
    + [f"oil{chr(cp)}price" for cp in (0x85, 0xA0, 0x3000)] + [f"oil{chr(cp)}price" for cp in NON_ASCII_SPACE]
    + ["caf\u00e9", "cafe caf\u00e9 caf\u00e9s", "le caf\u00e9 oil", "nul\0in oil nul", "\0 nul\0in\0",
       "del\x7fin del\x7f in \x7f",
       "x" * 5000 + " oil", "oil " + "x" * 5000, "x" * 5000,
       "Oil OIL oil oIl", "oi oil oils oilprice pric price prices crud crude cruder",
       "\u00e9 \u4e2d\u6587 oil \U0001f600 price", "oil\u200bprice", "oil price\u180e oil"])
