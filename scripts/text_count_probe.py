"""Counting words on the device (text_count.TextCounter: gcnk_text_count, the host read of nnz, gcnk_text_emit)
timed on R8-shaped synthetic text, beside the path it replaces, doc_term(CountVectorizer.transform(texts)), on the
same box in the same call where sklearn is installed.  Nothing is read from the reference.

  input     lda_estep_probe.synthetic()'s 7,674 documents over 7,463 words written out as text: every word of a
            document as often as its count, shuffled, with out-of-vocabulary tokens mixed in up to 504 k tokens in
            all, single spaces between; the words are distinct lower-case strings of 2 .. 11 letters, 5.6 on
            average, which gives R8's 3.35 MB.
  count     counter.count(bytes, offsets), the device half: HIP events around the call (memset, tokens, radix
            sort, run heads, scan, run starts, rows; the host read of nnz; emit).
  call      counter(texts) end to end, pack included: host wall clock, the device drained.
  pack      counter.pack(texts) alone (join, encode, one upload), and its host part without the upload.
  parent    doc_term(vectorizer.transform(texts), device): host wall clock, the device drained; and sklearn's
            transform alone beside it.

Warm, the legs alternated inside every run; median and spread (max - min) of --runs runs (sklearn: --sklearn-runs).
One JSON line:

  python scripts/text_count_probe.py [--runs 9] [--sklearn-runs 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
TOKENS, SEED = 504345, 20241


def words_and_texts(np, indptr, indices, counts, V):
    """(V vocabulary words, B texts, tokens in all, tokens outside the vocabulary)."""
    rng = np.random.default_rng(SEED)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))

    def fresh(n, seen):
        out = []
        while len(out) < n:
            length = int(np.clip(np.rint(rng.normal(5.6, 2.0)), 2, 11))
            w = "".join(rng.choice(letters, length))
            if w not in seen:
                seen.add(w)
                out.append(w)
        return out
    seen = set()
    words = fresh(V, seen)
    outside = fresh(2000, seen)
    B = len(indptr) - 1
    inside = int(counts.sum())
    extra = rng.multinomial(max(TOKENS - inside, 0), np.full(B, 1.0 / B))
    texts = []
    for d in range(B):
        ids = np.repeat(indices[indptr[d]:indptr[d + 1]], counts[indptr[d]:indptr[d + 1]])
        toks = [words[i] for i in ids] + [outside[i] for i in rng.integers(0, len(outside), extra[d])]
        rng.shuffle(toks)
        texts.append(" ".join(toks))
    return words, texts, inside + int(extra.sum()), int(extra.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--sklearn-runs", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import TextCounter, _lib, doc_term, text_count
    from lda_estep_probe import B, V, synthetic

    assert torch.cuda.is_available(), "this probe times the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    indptr, indices, counts, _, n = synthetic(np)
    words, texts, tokens, outside = words_and_texts(np, indptr, indices, counts, V)
    counter = TextCounter(words, dev)
    data, offsets = counter.pack(texts)
    per_doc = np.diff(indptr)
    res = {"case": f"word counts, B={B} V={V}: {tokens} tokens ({outside} outside the vocabulary) in {data.numel()} bytes, "
                   f"at most {int(max(len(t.split()) for t in texts))} tokens and {int(per_doc.max())} distinct words a "
                   f"document, nnz={int(indptr[-1])}; warm, {args.runs} runs alternating the legs",
           "lib": os.path.basename(_lib.LIB_PATH), "table_bytes": counter._table.numel(),
           "workspace_bytes": int(_lib.load().gcnk_text_workspace_bytes(data.numel(), B, V))}

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    def wall_us(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    legs = {"count": (event_us, lambda: counter.count(data, offsets)),
            "call": (wall_us, lambda: counter(texts)),
            "pack": (wall_us, lambda: counter.pack(texts)),
            "pack_host": (wall_us, lambda: text_count.pack_host(texts))}
    for _ in range(2):   # warm: allocator, kernels' code objects
        for _, fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.runs):
        for k, (timer, fn) in legs.items():
            times[k].append(timer(fn)[0])
    for k, v in times.items():
        res[f"{k}_us"] = round(statistics.median(v), 1)
        res[f"{k}_spread_us"] = round(max(v) - min(v), 1)
    got = counter(texts)
    want = (indptr, indices, counts.astype(np.float64))
    res["equal_to_the_generating_counts"] = all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))

    try:
        from sklearn.feature_extraction.text import CountVectorizer
    except ImportError:
        res["sklearn"] = "not installed here: no comparator on this box"
    else:
        vec = CountVectorizer(vocabulary=words, token_pattern=r"\S+", lowercase=False)
        parent, alone = [], []
        for _ in range(args.sklearn_runs):
            us, host = wall_us(lambda: doc_term(vec.transform(texts), dev))
            parent.append(us)
            t0 = time.perf_counter()
            vec.transform(texts)
            alone.append((time.perf_counter() - t0) * 1e6)
        res["parent_doc_term_of_transform_us"] = round(statistics.median(parent), 1)
        res["parent_spread_us"] = round(max(parent) - min(parent), 1)
        res["sklearn_transform_us"] = round(statistics.median(alone), 1)
        res["sklearn_transform_spread_us"] = round(max(alone) - min(alone), 1)
        res["parent_over_call"] = round(res["parent_doc_term_of_transform_us"] / res["call_us"], 1)
        res["parent_over_count"] = round(res["parent_doc_term_of_transform_us"] / res["count_us"], 1)
        res["equal_to_the_parent_path"] = all(torch.equal(g, h) and g.dtype == h.dtype for g, h in zip(got, host))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
