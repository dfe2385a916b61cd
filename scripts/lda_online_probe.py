"""The ONLINE LDA fit on the device (topic_fit.fit_topics(learning_method="online"): per minibatch fit E-step ->
online M-step -> exp_dirichlet) timed on lda_estep_probe.py's R8-shaped synthetic corpus, beside the device's
batch fit from the same run and sklearn's online LatentDirichletAllocation.fit of the same matrix on this box's
CPU where sklearn is installed.  Nothing is read from the reference.

  input     lda_estep_probe.synthetic(): 7,674 documents over 7,463 words, K = 50; max_iter = 20, batch_size 128
            (60 minibatches an EM iteration, 1,200 in all), tol 1e-3, cap 100.
  online    fit_topics(..., learning_method="online", init=(lambda0, gamma0s)) with the draws already on the
            device: HIP events around the whole call (index build, 3,601 launches, the normalisation).
  batch     fit_topics(..., init=...) of the same call, the batch method (61 launches).
  kinds     the online loop driven from here with an event pair around every launch, summed per kind of kernel
            (the events add a little to each launch; the sums say where the time goes, `online` what it costs).
  partial   OnlineTopics.partial_fit of the first 128 and of the first 1,024 documents (index build included),
            gamma0 already on the device.

Warm, the legs alternated inside every run; median and spread (max - min) of --runs runs.  sklearn: host wall
clock of one online fit.  One JSON line:

  python scripts/lda_online_probe.py [--runs 7] [--no-sklearn]
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
MAX_ITER, SEED, BATCH, DECAY, OFFSET = 20, 42, 128, 0.7, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import OnlineTopics, _lib, fit_topics, topic_fit
    from lda_estep_probe import B, K, V, synthetic

    assert torch.cuda.is_available(), "this probe times the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    indptr, indices, counts, _, n = synthetic(np)
    nnz = int(indptr[-1])
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    docs = (up(indptr), up(indices), up(counts.astype(np.float64)))
    alpha = eta = 1.0 / K
    slices = [(b0, min(b0 + BATCH, B)) for b0 in range(0, B, BATCH)]
    res = {"case": f"LDA online fit, B={B} V={V} K={K} nnz={nnz}, max_iter {MAX_ITER}, batch_size {BATCH} "
                   f"({len(slices) * MAX_ITER} minibatches), tol 1e-3, cap 100; warm, HIP events, {args.runs} runs "
                   f"alternating the legs; sklearn: wall clock",
           "lib": os.path.basename(_lib.LIB_PATH)}

    rs = np.random.RandomState(SEED)
    lam0 = up(rs.gamma(100.0, 0.01, (K, V)))
    g0s = up(rs.gamma(100.0, 0.01, (MAX_ITER, B, K)))

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    # the online loop of fit_topics driven from here, an event pair around every launch
    lib = _lib.load()
    ix = topic_fit.word_index(docs[0], docs[1], V)
    table = torch.zeros((V, (K + 1) // 2 * 2), dtype=torch.float64, device=dev)
    lam = torch.empty((K, V), dtype=torch.float64, device=dev)
    etheta = torch.empty((B, K), dtype=torch.float64, device=dev)
    ratio = torch.empty(nnz, dtype=torch.float64, device=dev)
    stream = _lib.stream(dev)
    ldt = table.stride(0)

    def exp_dirichlet():
        _lib.check(lib.gcnk_lda_exp_dirichlet_f64(lam.data_ptr(), V, K, V, table.data_ptr(), ldt, stream), "exp")

    def estep(it, b0, b1):
        _lib.check(lib.gcnk_lda_estep_fit_f64(docs[0][b0:].data_ptr(), docs[1].data_ptr(), docs[2].data_ptr(), 0, b1 - b0,
                                              V, K, table.data_ptr(), ldt, alpha, 1e-3, 100, g0s[it, b0:].data_ptr(), K,
                                              nnz, ratio.data_ptr(), etheta[b0:].data_ptr(), K, None, 0, None, stream),
                   "estep")

    def mstep(b0, b1, step):
        _lib.check(lib.gcnk_lda_mstep_online_f64(ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), nnz, b0, b1,
                                                 ratio.data_ptr(), etheta.data_ptr(), K, B, V, K, table.data_ptr(), ldt,
                                                 eta, float(np.power(OFFSET + step, -DECAY)), float(B) / (b1 - b0),
                                                 lam.data_ptr(), V, stream), "mstep_online")

    def by_kind():
        pairs = []

        def timed(kind, fn, *a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(*a)
            e1.record()
            pairs.append((kind, e0, e1))
        lam.copy_(lam0)
        timed("exp_dirichlet", exp_dirichlet)
        step = 1
        for it in range(MAX_ITER):
            for b0, b1 in slices:
                timed("estep_fit", estep, it, b0, b1)
                timed("mstep_online", mstep, b0, b1, step)
                timed("exp_dirichlet", exp_dirichlet)
                step += 1
        torch.cuda.synchronize()
        out = {}
        for kind, e0, e1 in pairs:
            out[kind] = out.get(kind, 0.0) + e0.elapsed_time(e1) * 1e3
        return out

    kw = dict(num_topics=K, max_iter=MAX_ITER, init=(lam0, g0s))
    online = lambda: fit_topics(*docs, V, learning_method="online", batch_size=BATCH, learning_decay=DECAY,   # noqa: E731
                                learning_offset=OFFSET, **kw)
    batch = lambda: fit_topics(*docs, V, **kw)   # noqa: E731

    def first(m):
        hi = int(indptr[m])
        return docs[0][:m + 1].contiguous(), docs[1][:hi].contiguous(), docs[2][:hi].contiguous()

    model = OnlineTopics(V, num_topics=K, total_samples=B, batch_size=BATCH, init_components=lam0)
    parts = {m: (first(m), g0s[0, :m].contiguous()) for m in (128, 1024)}
    partial = lambda m: model.partial_fit(*parts[m][0], gamma0=parts[m][1])   # noqa: E731

    for _ in range(2):   # warm: allocator, kernels' code objects
        online()
        batch()
        by_kind()
        partial(128)
        partial(1024)
    torch.cuda.synchronize()
    times = {"online_fit": [], "batch_fit": [], "partial_fit_128": [], "partial_fit_1024": []}
    kinds = {}
    for _ in range(args.runs):
        times["online_fit"].append(event_us(online)[0])
        times["batch_fit"].append(event_us(batch)[0])
        for k, v in by_kind().items():
            kinds.setdefault(k, []).append(v)
        times["partial_fit_128"].append(event_us(lambda: partial(128))[0])
        times["partial_fit_1024"].append(event_us(lambda: partial(1024))[0])
    for k, v in times.items():
        res[f"{k}_us"] = round(statistics.median(v), 1)
        res[f"{k}_spread_us"] = round(max(v) - min(v), 1)
    for k, v in kinds.items():
        res[f"{k}_launches_summed_us"] = round(statistics.median(v), 1)
        res[f"{k}_launches_summed_spread_us"] = round(max(v) - min(v), 1)
    launches = {"estep_fit": len(slices) * MAX_ITER, "mstep_online": len(slices) * MAX_ITER,
                "exp_dirichlet": len(slices) * MAX_ITER + 1}
    res["us_per_launch"] = {k: round(res[f"{k}_launches_summed_us"] / m, 1) for k, m in launches.items()}
    res["online_over_batch_fit"] = round(res["online_fit_us"] / res["batch_fit_us"], 2)

    fit = fit_topics(*docs, V, learning_method="online", batch_size=BATCH, return_iterations=True, **kw)
    its = fit.iterations.cpu().numpy()
    res["updates_per_em_iteration"] = [int(x) for x in its.sum(1)]
    res["documents_at_cap_per_em_iteration"] = [int(x) for x in (its == 100).sum(1)]
    lam_dev = fit.components.cpu().numpy()
    res["lambda_finite"] = bool(np.isfinite(lam_dev).all())
    res["n_batch_iter"] = fit.n_batch_iter

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
            t0 = time.perf_counter()
            lda = LatentDirichletAllocation(n_components=K, random_state=SEED, max_iter=MAX_ITER, learning_method="online",
                                            batch_size=BATCH, learning_decay=DECAY, learning_offset=OFFSET).fit(X)
            res["sklearn_online_fit_s"] = round(time.perf_counter() - t0, 2)
            res["sklearn_over_device_online_fit"] = round(res["sklearn_online_fit_s"] * 1e6 / res["online_fit_us"], 1)
            rel = np.abs(lam_dev - lda.components_) / lda.components_
            res["max_rel_lambda_minus_sklearn"] = float(rel.max())
            res["median_rel_lambda_minus_sklearn"] = float(np.median(rel))
            res["sklearn_n_batch_iter_"] = int(lda.n_batch_iter_)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
