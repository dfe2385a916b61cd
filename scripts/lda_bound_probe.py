"""The topic model's bound, score and perplexity on the device (topic_bound.TopicBound: the gamma E-step, then
gcnk_lda_bound_{docs,topics,finish}_f64) timed on lda_estep_probe.py's R8-shaped synthetic corpus, beside sklearn's
LatentDirichletAllocation.score of the same matrix on this box's CPU where sklearn is installed, and what
fit_topics(evaluate_every=1) adds to an EM iteration of the batch fit.  Nothing is read from the reference.

  input     lda_estep_probe.synthetic(): 7,674 documents over 7,463 words, K = 50; the model is fit_topics' batch
            fit of it, max_iter = 20, tol 1e-3, cap 100.
  score     TopicBound.score of all documents: HIP events around the whole call (4 launches: the E-step from
            gamma = 1, the documents' terms, the sum; the topic term is held, derived.py's cache).
  kinds     the same evaluation driven from here with an event pair around every launch, the topic term included
            (the events add a little to each launch; the figures say where the time goes, `score` what it costs).
  fit       fit_topics(max_iter=20) as it was, with compute_bound=True, and with evaluate_every=1 and perp_tol=0
            (20 evaluations, 20 host reads, no early stop): the difference over 20 is the cost an EM iteration.

Warm, the legs alternated inside every run; median and spread (max - min) of --runs runs.  sklearn: host wall
clock, the median of 3 scores.  One JSON line:

  python scripts/lda_bound_probe.py [--runs 7] [--no-sklearn]
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
MAX_ITER, SEED = 20, 42


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import _lib, fit_topics, topic_bound
    from graph_convolutional_networks_for_text_classification_amd.topic_infer import run_estep
    from lda_estep_probe import B, K, V, synthetic

    assert torch.cuda.is_available(), "this probe times the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    indptr, indices, counts, _, n = synthetic(np)
    nnz = int(indptr[-1])
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    docs = (up(indptr), up(indices), up(counts.astype(np.float64)))
    alpha = eta = 1.0 / K
    res = {"case": f"LDA bound, B={B} V={V} K={K} nnz={nnz}, the model a batch fit of max_iter {MAX_ITER}, tol 1e-3, "
                   f"cap 100; warm, HIP events, {args.runs} runs alternating the legs; sklearn: wall clock",
           "lib": os.path.basename(_lib.LIB_PATH)}

    rs = np.random.RandomState(SEED)
    lam0 = up(rs.gamma(100.0, 0.01, (K, V)))
    g0s = up(rs.gamma(100.0, 0.01, (MAX_ITER, B, K)))
    kw = dict(num_topics=K, max_iter=MAX_ITER, init=(lam0, g0s))
    model = fit_topics(*docs, V, **kw)
    tb = model.scorer()
    table = tb.inferencer._table().t

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    def by_kind():
        pairs, held = [], {}

        def timed(kind, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            held[kind] = fn()
            e1.record()
            pairs.append((kind, e0, e1))
        timed("estep_gamma", lambda: run_estep(table, K, V, *docs, B, alpha, 1e-3, 100, gamma=True)["gamma"])
        timed("bound_docs", lambda: topic_bound.doc_terms(table, K, V, *docs, B, held["estep_gamma"], alpha))
        timed("bound_topics", lambda: topic_bound.topic_terms(tb.components, eta))
        timed("bound_finish", lambda: topic_bound.finish(held["bound_docs"], held["bound_topics"], docs[0], docs[2], 1.0))
        torch.cuda.synchronize()
        return {kind: e0.elapsed_time(e1) * 1e3 for kind, e0, e1 in pairs}, held["bound_finish"]

    legs = {"score": lambda: tb.score(*docs),
            "fit": lambda: fit_topics(*docs, V, **kw),
            "fit_compute_bound": lambda: fit_topics(*docs, V, compute_bound=True, **kw),
            "fit_evaluate_every_1": lambda: fit_topics(*docs, V, evaluate_every=1, perp_tol=0.0, **kw)}
    for _ in range(2):   # warm: allocator, kernels' code objects
        for fn in legs.values():
            fn()
        by_kind()
    torch.cuda.synchronize()
    times, kinds = {k: [] for k in legs}, {}
    for _ in range(args.runs):
        for k, fn in legs.items():
            times[k].append(event_us(fn)[0])
        for k, v in by_kind()[0].items():
            kinds.setdefault(k, []).append(v)
    for k, v in times.items():
        res[f"{k}_us"] = round(statistics.median(v), 1)
        res[f"{k}_spread_us"] = round(max(v) - min(v), 1)
    for k, v in kinds.items():
        res[f"{k}_launch_us"] = round(statistics.median(v), 1)
        res[f"{k}_launch_spread_us"] = round(max(v) - min(v), 1)
    res["evaluate_every_1_extra_us_per_em_iteration"] = round(
        (res["fit_evaluate_every_1_us"] - res["fit_compute_bound_us"]) / MAX_ITER, 1)
    res["compute_bound_extra_us"] = round(res["fit_compute_bound_us"] - res["fit_us"], 1)

    out = by_kind()[1].cpu().numpy()
    res["score"], res["word_count"], res["perplexity"] = float(out[0]), float(out[1]), float(out[2])
    res["score_bitwise_equal_to_the_call"] = bool(float(tb.score(*docs)) == float(out[0]))
    ee = fit_topics(*docs, V, evaluate_every=1, perp_tol=0.0, **kw)
    res["training_perplexity_per_em_iteration"] = [round(p, 3) for p in ee.perplexities]
    res["fit_bound"] = float(ee.bound)

    if args.no_sklearn:
        res["sklearn"] = "not run"
    else:
        try:
            from sklearn.decomposition import LatentDirichletAllocation
            import scipy.sparse as sp
        except ImportError:
            res["sklearn"] = "not installed here: no comparator on this box"
        else:
            X = sp.csr_matrix((counts, indices, indptr), shape=(B, V))
            lda = LatentDirichletAllocation(n_components=K, random_state=SEED, max_iter=1).fit(X[:64])
            lda.components_ = tb.components.cpu().numpy()         # the device's model, evaluated by sklearn
            lda.exp_dirichlet_component_ = model.exp_topic_word.cpu().numpy().copy()
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                sk = float(lda.score(X))
                walls.append(time.perf_counter() - t0)
            res["sklearn_score_s"] = round(statistics.median(walls), 3)
            res["sklearn_score_spread_s"] = round(max(walls) - min(walls), 3)
            res["sklearn_over_device_score"] = round(res["sklearn_score_s"] * 1e6 / res["score_us"], 1)
            res["sklearn_score"] = sk
            res["rel_score_minus_sklearn"] = abs(res["score"] - sk) / abs(sk)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
