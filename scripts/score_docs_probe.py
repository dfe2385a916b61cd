"""Held-graph scoring (gcnk_score_docs_f32, inductive.DocumentScorer) on R8-shaped
documents, beside the two other ways to the same logits, for B = 32, 1,024 and
7,674 documents (R8's own, scored "as new"):

  kernel       the one launch, scorer(x, a);
  composition  entry points that existed before it: torch for the coefficients,
               gcnk_dense_gc1_f32 on [c_self x | c] with [W1[k0:k0+Kc]; S_T], torch
               for the closing c_self s2 + c S2_T + b2 (the held state precomputed,
               as the scorer holds it);
  copy floor   gcnk_stream_copy_f32 over the kernel's algorithmic bytes
               4 (B (Kc + H) + (Kc + H) F + F P + H P + B P), half read, half written;
  append       the parent's way: the documents appended to the graph as nodes, the
               adjacency normalised again, every operand-derived state rebuilt and one
               eval forward over all rows -- host wall clock from the arrays to the
               logits on the device, synchronised (its hub degrees include the new
               documents, so its logits are NOT the held-graph ones).

kernel, composition and copy floor: graph replays of --reps calls each (warm),
HIP events, the variants alternated inside every run; median and spread
(max - min) of --runs runs.  One JSON line per process:

  python scripts/score_docs_probe.py [--reps 20] [--runs 9] [--append-runs 3]
  python scripts/score_docs_probe.py --processes 3     # fresh child processes; the median of their medians
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (32, 1024, 7674)


def many(args):
    rows = []
    for _ in range(args.processes):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--runs", str(args.runs),
                            "--append-runs", str(args.append_runs)], check=True, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    out = {"case": f"median over {len(rows)} processes of each process's median; spread = max - min over the processes"}
    for key in rows[0]:
        if key.endswith("_us") or key.endswith("_ms"):
            vals = [r[key] for r in rows]
            out[key] = round(statistics.median(vals), 3)
            if "spread" not in key:
                out[key.rsplit("_", 1)[0] + "_process_spread_" + key.rsplit("_", 1)[1]] = round(max(vals) - min(vals), 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--append-runs", type=int, default=3)
    ap.add_argument("--processes", type=int, default=0)
    args = ap.parse_args()
    if args.processes:
        return many(args)

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import GCN, DocumentScorer, _lib, datasets, ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import score_ref

    assert torch.cuda.is_available(), "this probe times the GPU: no device, no number"
    dev = torch.device("cuda", 0)
    r8 = datasets.load_r8_fixture(os.path.join(ROOT, "tests", "golden", "r8_graph.npz"))
    ndoc, N, H = r8["ndoc"], r8["nodes"], r8["ntopic"]
    torch.manual_seed(0)
    model = GCN(nfeat=r8["nfeat"], nhid=200, nclass=r8["nclass"], dropout=0.5).to(dev)
    model.eval()
    X, A = r8["features"].to(dev), r8["adj"].to(dev)
    scorer = DocumentScorer(model, X, A)
    # (the scorer's held state, a private object: fac (.Kc, .k0, .hubs), F, P, W1, W2, b1, b2, S_T, S2_T, dh are read here)
    held = scorer._state()
    fac, F, P = held.fac, held.F, held.P
    Kc, k0 = fac.Kc, fac.k0
    import scipy.sparse as ssp
    a0 = r8["adj"].coalesce()
    Asp = ssp.csr_matrix((a0.values().double().numpy(), a0.indices().numpy()), shape=(N, N))
    a_all, _ = score_ref.recovered_edges(Asp, np.arange(ndoc), fac.hubs.numpy())
    x_all = np.ascontiguousarray(r8["features_dense"][:ndoc, k0:k0 + Kc])
    lib = _lib.load()
    res = {"case": f"R8-shaped documents (Kc={Kc}, H={H}, F={F}, P={P}), {args.reps} calls per graph replay (warm), "
                   f"{args.runs} runs alternating the variants", "lib": os.path.basename(_lib.LIB_PATH)}

    # the composition's fixed operand, held like the scorer's state
    Bcat = torch.cat([held.W1[k0:k0 + Kc], held.S_T], 0).contiguous()
    Kcat = Kc + H
    Kp = (Kcat + 3) // 4 * 4

    def composition(x, a):
        a64 = a.double()
        dd = (1.0 + a64.sum(1)).pow(-0.5)
        c_self = (dd * dd).float()[:, None]
        c = ((dd[:, None] * a64) * held.dh).float()
        U = torch.empty((x.shape[0], Kp), dtype=torch.float32, device=dev)[:, :Kcat]
        U[:, :Kc] = c_self * x
        U[:, Kc:] = c
        # (ops.dense_gc1 reads only .AX and .K of its ops.DenseAX argument: a stand-in with those two fields)
        got = ops.dense_gc1(types.SimpleNamespace(AX=U, K=Kcat), Bcat, held.b1, held.W2, store_h1=False)
        assert got is not None, "gcnk_dense_gc1_f32 refused the composition's operands"
        out = c_self * got[1] + c @ held.S2_T
        return out + held.b2 if held.b2 is not None else out

    def graph_of(fn):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.reps):
                keep = fn()
        g.replay()
        torch.cuda.synchronize()
        return g, keep

    def replay_us(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps * 1e3

    for B in SIZES:
        x = torch.zeros((B, (Kc + 3) // 4 * 4), device=dev)[:, :Kc]
        a = torch.zeros((B, (H + 3) // 4 * 4), device=dev)[:, :H]
        x.copy_(torch.from_numpy(x_all[:B]))
        a.copy_(torch.from_numpy(a_all[:B]))
        nbytes = 4 * (B * (Kc + H) + (Kc + H) * F + F * P + H * P + B * P)
        n_copy = nbytes // 8
        src, dst = torch.randn(n_copy, device=dev), torch.empty(n_copy, device=dev)

        def copy():
            _lib.check(lib.gcnk_stream_copy_f32(src.data_ptr(), dst.data_ptr(), n_copy, _lib.stream(dev)),
                       "gcnk_stream_copy_f32")

        legs = {"kernel": graph_of(lambda: scorer(x, a)), "composition": graph_of(lambda: composition(x, a)),
                "copy_floor": graph_of(copy)}
        diff = float((legs["kernel"][1] - legs["composition"][1]).abs().max())
        times = {k: [] for k in legs}
        for _ in range(args.runs):
            for k, (g, _) in legs.items():
                times[k].append(replay_us(g))
        for k, v in times.items():
            res[f"B{B}_{k}_us"] = round(statistics.median(v), 3)
            res[f"B{B}_{k}_spread_us"] = round(max(v) - min(v), 3)
        res[f"B{B}_algorithmic_bytes"] = nbytes
        res[f"B{B}_floor_over_kernel"] = round(res[f"B{B}_copy_floor_us"] / res[f"B{B}_kernel_us"], 3)
        res[f"B{B}_kernel_vs_composition_max_abs_diff"] = diff
        del legs

        # the parent's way: B more nodes, everything rebuilt, one forward over all rows
        theta_rows = np.repeat(np.arange(B), H)
        hub_cols = np.tile(fac.hubs.numpy(), B)
        w = a_all[:B].reshape(-1)
        nz = w > 0
        app = []
        for _ in range(args.append_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nr, nc = N + theta_rows[nz], hub_cols[nz]
            rows = np.concatenate([r8["a_rows"], nr, nc])
            cols = np.concatenate([r8["a_cols"], nc, nr])
            vals = np.concatenate([r8["a_vals"], w[nz], w[nz]])
            rr, cc, vv = datasets.sym_normalize(rows, cols, vals, N + B)
            A2 = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rr, cc])), torch.from_numpy(vv),
                                         (N + B, N + B)).to(dev)
            xi = r8["features"].coalesce()
            dr, dc = np.nonzero(x_all[:B])
            idx = torch.cat([xi.indices(), torch.from_numpy(np.stack([N + dr, k0 + dc]))], 1)
            val = torch.cat([xi.values(), torch.from_numpy(x_all[:B][dr, dc])])
            X2 = torch.sparse_coo_tensor(idx, val, (N + B, r8["nfeat"])).to(dev)
            with torch.no_grad():
                out2 = model(X2, A2)[N:]
            torch.cuda.synchronize()
            app.append((time.perf_counter() - t0) * 1e3)
            del A2, X2
        res[f"B{B}_append_and_forward_ms"] = round(statistics.median(app), 3)
        res[f"B{B}_append_and_forward_spread_ms"] = round(max(app) - min(app), 3)
        res[f"B{B}_append_vs_held_max_abs_diff"] = float((out2 - scorer(x, a)).abs().max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
