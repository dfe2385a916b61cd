"""Counting words on the device (csrc/text_count.hip): sklearn's
``CountVectorizer.transform`` of unseen text against a fitted vocabulary, as the
reference configures it (topic_model.py:93-102,159): ``token_pattern=r'\\S+'``,
``lowercase=False``, the word analyzer, unigrams, no stop words, no accent
stripping, ``binary=False``.

    counter = TextCounter.from_sklearn(vectorizer, "cuda")     # or TextCounter(words in id order)
    indptr, indices, counts = counter(new_texts)               # == doc_term(vectorizer.transform(new_texts), "cuda")
    scorer.predict(*inf.scorer_operands(indptr, indices, counts, 0.02))

The three arrays are equal element for element to the host path's (int32, int32
ascending in a row, float64) and go unchanged into ``TopicInferencer``,
``fit_topics``, ``OnlineTopics.partial_fit`` and ``TopicBound``.

``counter(texts)`` is ``count(*pack(texts))``.  ``pack`` is the host half: it maps
the 19 non-ASCII white-space code points of Python's ``\\s`` to a space in every
text that is not ASCII, encodes to UTF-8, and uploads the bytes and the documents'
offsets in one copy.  ``count`` is the device half (include/gcnk_text.h): a wave
per document finds the tokens -- maximal runs of bytes outside the ten ASCII
white-space bytes -- hashes each and looks it up byte for byte in the vocabulary
table; the (document, word) keys are sorted by hipCUB's radix sort and run-length
counted.  One host read per call (nnz, which sizes the exact outputs); integers
alone and no atomics, so a result is bitwise reproducible.

Still on the host: fitting the vocabulary (``min_df`` / ``max_df``), and ``pack``'s
join and encode.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .sparse import require_device

# the code points of Python's \s on str beyond ASCII: mapped to a space before encoding, after which byte equality
# is string equality and the ten ASCII white-space bytes are the only separators
NON_ASCII_SPACE = (0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000)
_TO_SPACE = {cp: " " for cp in NON_ASCII_SPACE}

# CountVectorizer's settings this restates: (attribute, the one supported value)
SUPPORTED = (("input", "content"), ("token_pattern", r"\S+"), ("lowercase", False), ("ngram_range", (1, 1)),
             ("stop_words", None), ("strip_accents", None), ("tokenizer", None), ("preprocessor", None),
             ("analyzer", "word"), ("binary", False))


def _utf8(s, what):
    if not isinstance(s, str):
        raise RuntimeError(f"{what} must be a str, got {type(s).__name__}")
    try:
        return s.encode("utf-8")
    except UnicodeEncodeError as e:
        raise RuntimeError(f"{what} cannot be encoded as UTF-8 ({e.reason} at {e.start})") from None


def vocabulary_words(vocabulary):
    """The words in id order from a sequence of words, or from a ``str -> id`` mapping whose ids
    are exactly 0 .. V-1 (sklearn's ``vocabulary_``)."""
    if hasattr(vocabulary, "items"):
        V = len(vocabulary)
        words = [None] * V
        for w, i in vocabulary.items():
            j = int(i)
            if j != i or not 0 <= j < V or words[j] is not None:
                raise RuntimeError(f"TextCounter: the vocabulary's ids must be exactly 0 .. {V - 1}, each once (got {i!r} "
                                   f"for {w!r})")
            words[j] = w
        return words
    if isinstance(vocabulary, (str, bytes)):
        raise RuntimeError("TextCounter: the vocabulary is a sequence of words or a str -> id mapping, not one string")
    return list(vocabulary)


def build_table(words):
    """gcnk_text_table_build on the host (no device) -> (table uint8 ndarray, V, slots, max_word_bytes, blob_bytes).
    RuntimeError on no word, an empty or duplicate word, a word that is no str or cannot be encoded."""
    enc = [_utf8(w, f"vocabulary word {i}") for i, w in enumerate(words)]
    V = len(enc)
    blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum([len(b) for b in enc], out=off[1:])
    nbytes = int(off[-1])
    lib = _lib.load()
    size = int(lib.gcnk_text_table_bytes(nbytes, V))
    if size < 0:
        _lib.check(size, "gcnk_text_table_bytes")
    table = np.zeros(size, dtype=np.uint8)
    _lib.check(lib.gcnk_text_table_build(blob.ctypes.data_as(ctypes.c_void_p), nbytes, off.ctypes.data_as(ctypes.c_void_p),
                                         V, table.ctypes.data_as(ctypes.c_void_p), size), "gcnk_text_table_build")
    hdr = table[:32].view(np.uint32)
    return table, V, int(hdr[2]), int(hdr[3]), nbytes


def pack_host(texts):
    """The host half without the upload: (bytes uint8 [N], offsets int64 [B+1]) as numpy arrays."""
    if isinstance(texts, (str, bytes)):
        raise RuntimeError("TextCounter: texts is a sequence of str, not one string (as CountVectorizer.transform)")
    texts = list(texts)
    for i, t in enumerate(texts):
        if not isinstance(t, str):
            raise RuntimeError(f"text {i} must be a str, got {type(t).__name__}")
    joined = "".join(texts)
    if joined.isascii():   # one encode for the batch: a character is a byte
        data, lens = joined.encode("ascii"), [len(t) for t in texts]
    else:
        parts = [_utf8(t if t.isascii() else t.translate(_TO_SPACE), f"text {i}") for i, t in enumerate(texts)]
        data, lens = b"".join(parts), [len(p) for p in parts]
    offsets = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return np.frombuffer(data, dtype=np.uint8), offsets


class TextCounter:
    """``CountVectorizer.transform`` on ``device`` against ``vocabulary``: the words in id
    order, or a ``str -> id`` mapping whose ids are exactly 0 .. V-1.  The table is built once,
    on the host, and uploaded."""

    def __init__(self, vocabulary, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"TextCounter counts on a ROCm GPU (got device {self.device}); there is no host fallback — "
                               "CountVectorizer.transform is the host path")
        table, self.V, self._slots, self._max_word, self._blob_bytes = build_table(vocabulary_words(vocabulary))
        self._table = torch.from_numpy(table).to(self.device)
        self.device = self._table.device

    @classmethod
    def from_sklearn(cls, vectorizer, device="cuda"):
        """From a fitted ``CountVectorizer`` (its ``vocabulary_``).  RuntimeError naming the setting
        for any configuration but the reference's."""
        missing = object()
        for name, want in SUPPORTED:
            got = getattr(vectorizer, name, missing)
            if name == "ngram_range" and isinstance(got, (tuple, list)):
                got = tuple(got)
            if got is missing or type(got) is not type(want) or got != want:
                shown = "missing" if got is missing else repr(got)
                raise RuntimeError(f"TextCounter.from_sklearn: {name}={shown} is not restated; only {name}={want!r} is "
                                   f"(CountVectorizer(token_pattern=r'\\S+', lowercase=False))")
        if not hasattr(vectorizer, "vocabulary_"):
            raise RuntimeError("TextCounter.from_sklearn: the vectorizer is not fitted (no vocabulary_)")
        return cls(vectorizer.vocabulary_, device)

    def pack(self, texts):
        """The host half: ``texts`` (a sequence of str) -> (bytes uint8 [N], offsets int64 [B+1])
        on the device, both views of ONE uploaded buffer.  RuntimeError on a text that is no str
        or cannot be encoded (a lone surrogate)."""
        data, offsets = pack_host(texts)
        head = offsets.nbytes
        buf = np.empty(head + data.size, dtype=np.uint8)
        buf[:head] = offsets.view(np.uint8)
        buf[head:] = data
        dev = torch.from_numpy(buf).to(self.device)
        return dev[head:], dev[:head].view(torch.int64)

    def count(self, bytes, offsets):
        """The device half: ``bytes`` uint8 [N] and ``offsets`` int64 [B+1] (ascending, from 0 to
        at most N) on the counter's device -> (indptr int32 [B+1], indices int32 [nnz], counts
        float64 [nnz]).  One host read (nnz)."""
        for what, t, dt in (("bytes", bytes, torch.uint8), ("offsets", offsets, torch.int64)):
            require_device(t, what)
            if t.device != self.device:
                raise RuntimeError(f"{what} is on {t.device}, the vocabulary on {self.device}")
            if t.dim() != 1 or t.dtype != dt:
                raise RuntimeError(f"{what} must be one-dimensional {dt}, got {t.dtype} {tuple(t.shape)}")
        if offsets.numel() < 1:
            raise RuntimeError("offsets holds B + 1 entries: at least one")
        bytes, offsets = bytes.contiguous(), offsets.contiguous()
        N, B, dev, lib = bytes.numel(), offsets.numel() - 1, self.device, _lib.load()
        wsb = int(lib.gcnk_text_workspace_bytes(N, B, self.V))
        if wsb < 0:
            _lib.check(wsb, "gcnk_text_workspace_bytes")
        indptr = torch.empty(B + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gcnk_text_count(
                bytes.data_ptr() if N else None, N, offsets.data_ptr(), B, self._table.data_ptr(), self._table.numel(),
                self.V, self._slots, self._max_word, self._blob_bytes, indptr.data_ptr(), ws.data_ptr(), wsb,
                _lib.stream(dev)), "gcnk_text_count")
            nnz = int(indptr[B])   # the one synchronisation
            indices = torch.empty(nnz, dtype=torch.int32, device=dev)
            counts = torch.empty(nnz, dtype=torch.float64, device=dev)
            if nnz:
                _lib.check(lib.gcnk_text_emit(N, B, self.V, nnz, indices.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                              wsb, _lib.stream(dev)), "gcnk_text_emit")
        return indptr, indices, counts

    def __call__(self, texts):
        return self.count(*self.pack(texts))
