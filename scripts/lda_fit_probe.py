"""The LDA fit on the device (topic_fit.fit_topics: exp_dirichlet -> fit E-step -> M-step, max_iter times) timed
on lda_estep_probe.py's R8-shaped synthetic corpus, beside sklearn's LatentDirichletAllocation.fit of the same
matrix on this box's CPU where sklearn is installed.  Nothing is read from the reference.

  input    lda_estep_probe.synthetic(): 7,674 documents over 7,463 words, K = 50; max_iter = 20, tol 1e-3, cap 100.
  fit      fit_topics(..., init=(lambda0, gamma0s)) with the draws already on the device: HIP events around the
           whole call (index build, 61 launches, the normalisation).
  kinds    the same loop driven from here with an event pair around every launch, summed per kind of kernel
           (the events add a little to each launch; the sums say where the time goes, `fit` what it costs).
  longest  the M-step of the whole vocabulary, of the most frequent word alone, and of one word that 0.95 B
           documents hold (the longest chain max_df = 0.95 allows; a launch lasts as long as its longest chain).
  host     numpy's RandomState draw of lambda0 and the (max_iter, B, K) gamma0s, and their upload: wall clock.

Warm, the legs alternated inside every run; median and spread (max - min) of --runs runs.  sklearn: host wall
clock of one fit (it takes tens of seconds).  One JSON line:

  python scripts/lda_fit_probe.py [--runs 15] [--no-sklearn]
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
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import _lib, fit_topics, topic_fit
    from lda_estep_probe import B, K, V, synthetic

    assert torch.cuda.is_available(), "this probe times the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    indptr, indices, counts, _, n = synthetic(np)
    nnz = int(indptr[-1])
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    docs = (up(indptr), up(indices), up(counts.astype(np.float64)))
    alpha = eta = 1.0 / K
    df = np.bincount(indices, minlength=V)
    res = {"case": f"LDA batch fit, B={B} V={V} K={K} nnz={nnz}, max_iter {MAX_ITER}, tol 1e-3, cap 100; warm, HIP events, "
                   f"{args.runs} runs alternating the legs; host draw and sklearn: wall clock",
           "lib": os.path.basename(_lib.LIB_PATH),
           "document_frequency": {"median": float(np.median(df)), "p99": float(np.percentile(df, 99)), "max": int(df.max()),
                                  "unheld_words": int((df == 0).sum())}}

    host = {"draw_s": [], "upload_s": []}
    for _ in range(3):
        t0 = time.perf_counter()
        rs = np.random.RandomState(SEED)
        lam0_h = rs.gamma(100.0, 0.01, (K, V))
        g0_h = rs.gamma(100.0, 0.01, (MAX_ITER, B, K))
        t1 = time.perf_counter()
        lam0, g0s = up(lam0_h), up(g0_h)
        torch.cuda.synchronize()
        host["draw_s"].append(t1 - t0)
        host["upload_s"].append(time.perf_counter() - t1)
    res["host_draw_s"] = round(statistics.median(host["draw_s"]), 4)
    res["host_upload_s"] = round(statistics.median(host["upload_s"]), 4)

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    # the loop of fit_topics driven from here, an event pair around every launch
    lib = _lib.load()
    ix = topic_fit.word_index(docs[0], docs[1], V)
    table = torch.zeros((V, (K + 1) // 2 * 2), dtype=torch.float64, device=dev)
    lam = torch.empty((K, V), dtype=torch.float64, device=dev)
    etheta = torch.empty((B, K), dtype=torch.float64, device=dev)
    ratio = torch.empty(nnz, dtype=torch.float64, device=dev)
    stream = _lib.stream(dev)
    ldt = table.stride(0)

    def exp_dirichlet(src):
        _lib.check(lib.gcnk_lda_exp_dirichlet_f64(src.data_ptr(), src.stride(0), K, V, table.data_ptr(), ldt, stream), "exp")

    def estep(it):
        g0 = g0s[it]
        _lib.check(lib.gcnk_lda_estep_fit_f64(docs[0].data_ptr(), docs[1].data_ptr(), docs[2].data_ptr(), 0, B, V, K,
                                              table.data_ptr(), ldt, alpha, 1e-3, 100, g0.data_ptr(), K, nnz,
                                              ratio.data_ptr(), etheta.data_ptr(), K, None, 0, None, stream), "estep")

    def mstep():
        _lib.check(lib.gcnk_lda_mstep_f64(ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), nnz, ratio.data_ptr(),
                                          etheta.data_ptr(), K, B, V, K, table.data_ptr(), ldt, eta, lam.data_ptr(), V,
                                          stream), "mstep")

    def by_kind():
        pairs = []

        def timed(kind, fn, *a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(*a)
            e1.record()
            pairs.append((kind, e0, e1))
        for it in range(MAX_ITER):
            timed("exp_dirichlet", exp_dirichlet, lam0 if it == 0 else lam)
            timed("estep_fit", estep, it)
            timed("mstep", mstep)
        timed("exp_dirichlet", exp_dirichlet, lam)
        torch.cuda.synchronize()
        out = {}
        for kind, e0, e1 in pairs:
            out[kind] = out.get(kind, 0.0) + e0.elapsed_time(e1) * 1e3
        return out

    # one word as a vocabulary of its own, a single chain: the corpus's most frequent word, and a word that
    # 0.95 B documents hold (CountVectorizer's max_df = 0.95 allows it; this corpus has none)
    one_lam = torch.empty((K, 1), dtype=torch.float64, device=dev)

    def one_word(holds):
        ip = up(np.concatenate([[0], np.cumsum(holds)]).astype(np.int32))
        m = int(holds.sum())
        ix1 = topic_fit.word_index(ip, torch.zeros(m, dtype=torch.int32, device=dev), 1)
        return lambda: _lib.check(lib.gcnk_lda_mstep_f64(   # noqa: E731
            ix1.wptr.data_ptr(), ix1.pos.data_ptr(), ix1.doc.data_ptr(), m, ratio.data_ptr(), etheta.data_ptr(), K, B, 1,
            K, table.data_ptr(), ldt, eta, one_lam.data_ptr(), 1, stream), "mstep")

    holds = np.zeros(B, np.int64)
    holds[np.unique(np.repeat(np.arange(B), np.diff(indptr))[indices == int(df.argmax())])] = 1
    mstep_longest = one_word(holds)
    chain = int(0.95 * B)
    mstep_chain = one_word((np.arange(B) < chain).astype(np.int64))

    whole = lambda: fit_topics(*docs, V, num_topics=K, max_iter=MAX_ITER, init=(lam0, g0s))   # noqa: E731
    for _ in range(2):   # warm: allocator, kernels' code objects
        whole()
        by_kind()
        mstep_longest()
        mstep_chain()
    torch.cuda.synchronize()
    times = {"fit": [], "mstep_all_words": [], "mstep_longest_word_alone": [], "mstep_chain_of_095B_alone": []}
    kinds = {}
    for _ in range(args.runs):
        t, fit = event_us(whole)
        times["fit"].append(t)
        for k, v in by_kind().items():
            kinds.setdefault(k, []).append(v)
        times["mstep_all_words"].append(event_us(mstep)[0])
        times["mstep_longest_word_alone"].append(event_us(mstep_longest)[0])
        times["mstep_chain_of_095B_alone"].append(event_us(mstep_chain)[0])
    for k, v in times.items():
        res[f"{k}_us"] = round(statistics.median(v), 1)
        res[f"{k}_spread_us"] = round(max(v) - min(v), 1)
    for k, v in kinds.items():
        res[f"{k}_launches_summed_us"] = round(statistics.median(v), 1)
        res[f"{k}_launches_summed_spread_us"] = round(max(v) - min(v), 1)
    res["longest_word"] = {"documents": int(df.max()), "of_B": round(float(df.max()) / B, 3)}
    res["chain_of_095B"] = {"documents": chain, "ns_per_entry": round(res["mstep_chain_of_095B_alone_us"] * 1e3 / chain, 1)}

    fit = fit_topics(*docs, V, num_topics=K, max_iter=MAX_ITER, init=(lam0, g0s), return_iterations=True)
    its = fit.iterations.cpu().numpy()
    res["updates_per_em_iteration"] = [int(x) for x in its.sum(1)]
    res["documents_at_cap_per_em_iteration"] = [int(x) for x in (its == 100).sum(1)]
    lam_dev = fit.components.cpu().numpy()
    res["lambda_finite"] = bool(np.isfinite(lam_dev).all())

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
            lda = LatentDirichletAllocation(n_components=K, random_state=SEED, max_iter=MAX_ITER,
                                            learning_method="batch").fit(X)
            res["sklearn_fit_s"] = round(time.perf_counter() - t0, 2)
            res["sklearn_over_device_fit"] = round(res["sklearn_fit_s"] * 1e6 / res["fit_us"], 1)
            res["sklearn_over_device_fit_with_host_draw"] = round(
                res["sklearn_fit_s"] / (res["fit_us"] * 1e-6 + res["host_draw_s"] + res["host_upload_s"]), 1)
            rel = np.abs(lam_dev - lda.components_) / lda.components_
            res["max_rel_lambda_minus_sklearn"] = float(rel.max())
            res["median_rel_lambda_minus_sklearn"] = float(np.median(rel))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
