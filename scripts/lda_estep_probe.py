"""The LDA E-step on the device (gcnk_lda_estep_f64, topic_infer.TopicInferencer) timed on an R8-shaped
synthetic input, beside sklearn's LatentDirichletAllocation.transform of the same input on this box's CPU
where sklearn is installed.  Nothing is read from the reference.

  input    7,674 documents over a vocabulary of 7,463 words, 50 topics, seeded: distinct words per document
           drawn log-normally to R8's statistics (median 30, 99th percentile 208, at most 291), counts
           1 + geometric; the model lambda = eta + a Dirichlet(0.05) draw per topic scaled to the corpus,
           documents drawn from mixtures of one to three topics.
  theta    inf(indptr, indices, counts): one launch; also the documents of at most one tile (64 words) and
           the longer ones as launches of their own, and the longest document alone (a launch lasts as long
           as its slowest wave).
  operands inf.scorer_operands(...): the same launch with the (x, a) epilogue instead of theta.
  labels   scorer_operands -> DocumentScorer.predict, against inf(...) -> from_theta -> predict, on a
           synthetic doc-topic graph of the same size (datasets.doc_topic_graph) and a seeded GCN.

Warm, HIP events around each call, the legs alternated inside every run; median and spread (max - min) of
--runs runs.  sklearn: host wall clock of transform(), median of --sklearn-runs.  One JSON line:

  python scripts/lda_estep_probe.py [--runs 15] [--sklearn-runs 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, V, K = 7674, 7463, 50
THRESHOLD = 0.02


def synthetic(np):
    rng = np.random.default_rng(20240)
    n = np.clip(np.rint(np.exp(rng.normal(np.log(30.0), 0.832, B))), 1, 291).astype(np.int64)
    topics = rng.dirichlet(np.full(V, 0.05), K)
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    indices = np.empty(indptr[-1], np.int32)
    for d in range(B):
        mix = rng.dirichlet(np.full(int(rng.integers(1, 4)), 1.0))
        p = mix @ topics[rng.choice(K, mix.size, replace=False)] + 1e-9
        indices[indptr[d]:indptr[d + 1]] = np.sort(rng.choice(V, n[d], replace=False, p=p / p.sum()))
    counts = rng.geometric(0.7, indptr[-1]).astype(np.int64)
    lam = 1.0 / K + topics * (counts.sum() / K)
    return indptr, indices, counts, lam, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--sklearn-runs", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import (GCN, DocumentScorer, TopicInferencer, _lib,
                                                                           datasets, from_theta)

    assert torch.cuda.is_available(), "this probe times the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    indptr, indices, counts, lam, n = synthetic(np)
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    docs = (up(indptr), up(indices), up(counts))
    alpha = 1.0 / K
    inf = TopicInferencer.from_components(up(lam), alpha)
    res = {"case": f"LDA E-step, B={B} V={V} K={K} nnz={int(indptr[-1])}, tol 1e-3, cap 100; warm, HIP events around "
                   f"each call, {args.runs} runs alternating the legs; sklearn: host wall clock",
           "lib": os.path.basename(_lib.LIB_PATH),
           "words_per_document": {"median": float(np.median(n)), "p99": float(np.percentile(n, 99)), "max": int(n.max())}}

    g = datasets.doc_topic_graph(ndoc=B, ntopic=K, nclass=8, seed=0)
    torch.manual_seed(5)
    model = GCN(nfeat=g["nfeat"], nhid=200, nclass=8, dropout=0.5).to(dev).eval()
    scorer = DocumentScorer(model, g["features"].to(dev), g["adj"].to(dev))

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    def subset(keep):   # the documents `keep` as a batch of their own
        sel = np.concatenate([np.arange(indptr[d], indptr[d + 1]) for d in keep])
        ip = np.concatenate([[0], np.cumsum(n[keep])]).astype(np.int32)
        return up(ip), up(indices[sel]), up(counts[sel])

    short, long_ = subset(np.flatnonzero(n <= 64)), subset(np.flatnonzero(n > 64))
    longest = subset(np.array([int(n.argmax())]))
    res["documents"] = {"one_tile": int((n <= 64).sum()), "chunked": int((n > 64).sum())}
    legs = {"theta": lambda: inf(*docs),
            "theta_one_tile_documents": lambda: inf(*short),
            "theta_chunked_documents": lambda: inf(*long_),
            "theta_longest_document_alone": lambda: inf(*longest),
            "operands": lambda: inf.scorer_operands(*docs, THRESHOLD),
            "labels_fused": lambda: scorer.predict(*inf.scorer_operands(*docs, THRESHOLD)),
            "labels_from_theta": lambda: scorer.predict(*from_theta(inf(*docs), THRESHOLD))}
    for fn in legs.values():   # warm: allocator, kernels' code objects, the held table
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times, outs = {k: [] for k in legs}, {}
    for _ in range(args.runs):
        for k, fn in legs.items():
            t, outs[k] = event_us(fn)
            times[k].append(t)
    for k, v in times.items():
        res[f"{k}_us"] = round(statistics.median(v), 1)
        res[f"{k}_spread_us"] = round(max(v) - min(v), 1)
    res["labels_equal"] = bool(torch.equal(outs["labels_fused"], outs["labels_from_theta"]))
    theta, iters = inf(*docs, return_iterations=True)
    it = iters.cpu().numpy()
    res["iterations"] = {"min": int(it.min()), "median": float(np.median(it)), "p99": float(np.percentile(it, 99)),
                         "max": int(it.max()), "mean": round(float(it.mean()), 2), "at_cap": int((it == 100).sum())}
    res["longest_document"] = {"words": int(n.max()), "iterations": int(it[int(n.argmax())])}
    slow = int((it * np.ceil(n / 64)).argmax())
    res["most_chunk_iterations"] = {"words": int(n[slow]), "iterations": int(it[slow])}
    res["theta_us_per_document_iteration"] = round(res["theta_us"] / float(it.sum()), 6)

    try:
        from sklearn.decomposition import LatentDirichletAllocation
        import scipy.sparse as sp
    except ImportError:
        res["sklearn"] = "not installed here: no comparator on this box"
    else:
        lda = LatentDirichletAllocation(n_components=K, doc_topic_prior=alpha)
        lda.components_ = lam
        lda.exp_dirichlet_component_ = inf.exp_topic_word.cpu().numpy().copy()
        lda.doc_topic_prior_ = alpha
        lda.n_features_in_ = V
        X = sp.csr_matrix((counts, indices, indptr), shape=(B, V))
        wall = []
        for _ in range(args.sklearn_runs):
            t0 = time.perf_counter()
            want = lda.transform(X)
            wall.append(time.perf_counter() - t0)
        res["sklearn_transform_s"] = round(statistics.median(wall), 3)
        res["sklearn_transform_spread_s"] = round(max(wall) - min(wall), 3)
        res["sklearn_over_device"] = round(res["sklearn_transform_s"] * 1e6 / res["theta_us"], 1)
        err = np.abs(theta.cpu().numpy() - want).max(1)
        res["max_abs_theta_minus_sklearn"] = float(err.max())
        res["documents_off_sklearn_by_more_than_1e-12"] = int((err > 1e-12).sum())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
