"""The doc-topic graph built on the device (gcnk_topic_graph_build,
topic_graph.build_topic_graph) beside the two ways to the same A-hat that existed before it,
from the same theta and topic similarities, at thresholds 0.02 / 0.3:

  build        build_topic_graph(theta, topic_sim): device theta -> the CSR of A-hat, its one
               host synchronisation included;
  composition  torch nonzero / cat / stack -> a symmetric COO -> sparse.preprocess_adj
               (gcnk_coo_to_csr, its sortedness and symmetry check with a transpose,
               gcnk_sym_normalize), from the same device tensors;
  edgelist     the reference's hand-over: datasets.load_edgelist of a "u v weight" text file
               (written here, outside the timing) + sparse.preprocess_adj, host wall clock.

Two inputs: R8 (D = 7674, K = 50: the fixture's kept theta and topic block) and the 20ng shape
of datasets.doc_topic_graph (D = 18846, K = 70: seeded Dirichlet(1/K) theta, U(0, 1) sim).
build and composition: warm, HIP events around the whole call (the host blocks inside it, so
the interval is the caller's latency), alternated inside every run; median and spread
(max - min) of --runs runs.  One JSON line:

  python scripts/topic_graph_probe.py [--runs 15] [--edgelist-runs 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TD, TT = 0.02, 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--edgelist-runs", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import _lib, build_topic_graph, datasets, sparse
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import topic_graph_ref as ref

    assert torch.cuda.is_available(), "this probe times the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    r8_theta, r8_sim, _, _ = ref.r8_inputs()
    inputs = {"r8": (r8_theta, r8_sim),
              "20ng": (ref.dirichlet_theta(18846, 70, seed=0), ref.uniform_sim(70, seed=0))}
    res = {"case": f"theta -> A-hat at thresholds {TD} / {TT}; warm, HIP events around each call, {args.runs} runs "
                   "alternating build and composition; edgelist: host wall clock",
           "lib": os.path.basename(_lib.LIB_PATH)}

    def composition(theta, sim):
        D, K = theta.shape
        d, k = (theta >= TD).nonzero(as_tuple=True)
        w = theta[d, k].float()
        i, j = ((sim > TT) & torch.ones_like(sim, dtype=torch.bool).triu(1)).nonzero(as_tuple=True)
        ww = sim[i, j].float()
        rows = torch.cat([d, D + k, D + i, D + j])
        cols = torch.cat([D + k, d, D + j, D + i])
        A = torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.cat([w, w, ww, ww]), (D + K, D + K))
        return sparse.preprocess_adj(A)

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    for name, (theta_h, sim_h) in inputs.items():
        theta, sim = torch.from_numpy(theta_h).to(dev), torch.from_numpy(sim_h).to(dev)
        D, K = theta.shape
        legs = {"build": lambda: build_topic_graph(theta, topic_sim=sim, doc_topic_threshold=TD,
                                                   topic_topic_threshold=TT).adj,
                "composition": lambda: composition(theta, sim)}
        for fn in legs.values():   # warm: allocator, kernels' code objects
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times, outs = {k: [] for k in legs}, {}
        for _ in range(args.runs):
            for k, fn in legs.items():
                t, outs[k] = event_us(fn)
                times[k].append(t)
        a, b = outs["build"], outs["composition"]
        same = (torch.equal(a.rowptr, b.rowptr) and torch.equal(a.colind, b.colind)
                and torch.equal(a.val.view(torch.int32), b.val.view(torch.int32)))
        res[f"{name}_shape"] = [D, K, a.nnz]
        res[f"{name}_build_equals_composition_bitwise"] = same
        for k, v in times.items():
            res[f"{name}_{k}_us"] = round(statistics.median(v), 1)
            res[f"{name}_{k}_spread_us"] = round(max(v) - min(v), 1)
        res[f"{name}_composition_over_build"] = round(res[f"{name}_composition_us"] / res[f"{name}_build_us"], 2)

        # the reference's hand-over: a text edge list (each edge once, as nx.write_weighted_edgelist writes it)
        dd, kk = np.nonzero(theta_h >= TD)
        ii, jj = np.nonzero(np.triu(sim_h > TT, 1))
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "graph.txt")
            with open(path, "w") as f:
                # (the format cannot name a node without an edge: neither input has one)
                for u, v, wgt in zip(dd, D + kk, theta_h[dd, kk]):
                    f.write(f"{u} {v} {float(wgt)!r}\n")
                for u, v, wgt in zip(D + ii, D + jj, sim_h[ii, jj]):
                    f.write(f"{u} {v} {float(wgt)!r}\n")
            wall = []
            for _ in range(args.edgelist_runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c = sparse.preprocess_adj(datasets.load_edgelist(path, device=dev))
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
        res[f"{name}_edgelist_ms"] = round(statistics.median(wall), 3)
        res[f"{name}_edgelist_spread_ms"] = round(max(wall) - min(wall), 3)
        res[f"{name}_edgelist_equals_build_bitwise"] = bool(
            c.shape == a.shape and torch.equal(c.rowptr, a.rowptr) and torch.equal(c.colind, a.colind)
            and torch.equal(c.val.view(torch.int32), a.val.view(torch.int32)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
