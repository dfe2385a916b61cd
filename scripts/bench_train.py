"""R8 training-step timing: one step of trainer.py:354-361
(model.train(), zero_grad, forward, cross-entropy on the training nodes,
backward, Adam step) through the HIP drop-in, next to the oracle's torch-CPU
step (the reference's own ATen calls) on this host's cores.

Prints one JSON line per case.  Eager launches (the training loop is eager in
the reference too); GPU times are HIP events around `--steps` steps.  The step
on the device's own masks is also measured with the native loss and optimiser
(train.IndexedCrossEntropy, train.Adam) beside torch's, each eager and
replayed from a hipGraph (median and spread of `--runs` runs), and the Adam
launch alone beside a stream copy of its bytes.

usage: python scripts/bench_train.py [--steps 50] [--cpu-steps 5] [--runs 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--cpu-steps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5, help="timed runs of --steps replays per replayed leg")
    args = ap.parse_args()

    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import GCN, _lib, datasets, train
    from oracle import gcn_ref

    dev = torch.device("cuda", 0)
    r8 = datasets.load_r8_fixture(os.path.join(ROOT, "tests", "golden", "r8_graph.npz"))
    nfeat, nclass = r8["nfeat"], r8["nclass"]
    target = torch.as_tensor(r8["target"]).long()
    tr = torch.as_tensor(r8["train_lst"]).long()

    def run(model, x, adj, tgt, idx, steps, sync):
        opt = torch.optim.Adam(model.parameters(), lr=0.02)
        crit = torch.nn.CrossEntropyLoss()

        def step():
            model.train()
            opt.zero_grad()
            logits = model(x, adj)
            loss = crit(logits[idx], tgt[idx])
            loss.backward()
            opt.step()
            return loss

        for _ in range(3):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        return (time.perf_counter() - t0) / steps * 1e3

    x, adj = r8["features"].to(dev), r8["adj"].to(dev)
    for rng in ("cpu", "device"):
        torch.manual_seed(0)
        model = GCN(nfeat=nfeat, nhid=200, nclass=nclass, dropout=0.5, dropout_rng=rng).to(dev)
        ms = run(model, x, adj, target.to(dev), tr.to(dev), args.steps, torch.cuda.synchronize)
        print(json.dumps({"case": "R8 train step (fwd + bwd + Adam)", "impl": f"HIP, dropout_rng={rng}",
                          "ms_per_step": round(ms, 4), "steps": args.steps}), flush=True)

    # the same step (dropout_rng="device") captured once in a hipGraph and replayed:
    # launch-overhead-free kernel time of a training step.  The hash offset lives
    # on the device and the captured forward advances it, so every replay trains
    # on a fresh mask (checked below: the stream position moves one step per replay).
    # Two legs in this one process: torch's CrossEntropyLoss on logits[idx] and
    # torch.optim.Adam (trainer.py:307-308 as written), and the native loss and
    # optimiser (train.IndexedCrossEntropy, train.Adam); each eager and replayed, the replayed step as the median of
    # --runs timed runs with their spread (max - min).
    tgt, idx = target.to(dev), tr.to(dev)

    def leg(native):
        torch.manual_seed(0)
        model = GCN(nfeat=nfeat, nhid=200, nclass=nclass, dropout=0.5, dropout_rng="device").to(dev)
        model.train()
        if native:
            opt = train.Adam(model.parameters(), lr=0.02)
            crit = train.IndexedCrossEntropy()

            def step():
                opt.zero_grad()   # to None, as the reference's call does: no fills, and autograd stores, not adds
                loss = crit(model(x, adj), tgt, idx)
                loss.backward()
                opt.step()
                return loss
        else:
            opt = torch.optim.Adam(model.parameters(), lr=0.02, capturable=True)
            crit = torch.nn.CrossEntropyLoss()

            def step():
                opt.zero_grad(set_to_none=False)
                loss = crit(model(x, adj)[idx], tgt[idx])
                loss.backward()
                opt.step()
                return loss

        name = "native loss + Adam" if native else "torch loss + Adam"
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            s.synchronize()
            eager_ms = (time.perf_counter() - t0) / args.steps * 1e3
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        print(json.dumps({"case": "R8 train step (fwd + bwd + Adam)", "impl": f"HIP, dropout_rng=device, {name}, eager",
                          "ms_per_step": round(eager_ms, 4), "steps": args.steps}), flush=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        g.replay()
        torch.cuda.synchronize()
        base0 = int(model._rng_base.item())
        runs = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                g.replay()
            e1.record()
            e1.synchronize()
            runs.append(e0.elapsed_time(e1) / args.steps)
        advanced = (int(model._rng_base.item()) - base0) // (r8["nodes"] * 200)
        res = {"case": "R8 train step (fwd + bwd + Adam)", "impl": f"HIP, dropout_rng=device, {name}, hipGraph replay",
               "ms_per_step": round(statistics.median(runs), 4), "runs_ms": [round(r, 4) for r in runs],
               "spread_ms": round(max(runs) - min(runs), 4), "steps": args.steps,
               "fresh_masks": advanced == args.steps * args.runs}
        if native:
            res["optimizer_steps"] = opt.steps
        print(json.dumps(res), flush=True)
        return res

    torch_leg, native_leg = leg(False), leg(True)
    gain = torch_leg["ms_per_step"] - native_leg["ms_per_step"]
    print(json.dumps({"case": "R8 replayed train step, native loss + Adam against torch's",
                      "torch_ms": torch_leg["ms_per_step"], "native_ms": native_leg["ms_per_step"],
                      "torch_spread_ms": torch_leg["spread_ms"], "native_spread_ms": native_leg["spread_ms"],
                      "gain_ms": round(gain, 4), "faster_beyond_torch_spread": gain > torch_leg["spread_ms"]}),
          flush=True)

    # the Adam launch alone on R8's 1.49 M parameters (28 B per element) beside the streaming
    # floor for the same bytes: gcnk_stream_copy_f32 of 3.5 floats per element (14 B read, 14 B written)
    params = [p for p in GCN(nfeat=nfeat, nhid=200, nclass=nclass, dropout=0.5).to(dev).parameters()]
    for p in params:
        p.grad = torch.randn_like(p)
    opt = train.Adam(params, lr=0.02)
    numel = sum(p.numel() for p in params)
    n_copy = (7 * numel // 2) // 4 * 4
    src, dst = torch.randn(n_copy, device=dev), torch.empty(n_copy, device=dev)
    lib = _lib.load()

    def timed(fn, reps=20):   # `reps` launches per replay of a graph: kernel time, no host time between them
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        g.replay()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / reps * 1e3)
        return round(statistics.median(out), 3)

    def copy():
        lib.gcnk_stream_copy_f32(src.data_ptr(), dst.data_ptr(), n_copy,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    adam_us = timed(opt.step)
    copy_us = timed(copy)
    print(json.dumps({"case": "Adam step alone, R8 parameters, 20 launches per graph replay (warm caches)",
                      "numel": numel, "bytes": 28 * numel, "adam_us": adam_us,
                      "stream_copy_same_bytes_us": copy_us,
                      "adam_GBps": round(28 * numel / adam_us / 1e3, 1),
                      "copy_GBps": round(8 * n_copy / copy_us / 1e3, 1)}), flush=True)

    if args.cpu_steps > 0:
        torch.manual_seed(0)
        ref = gcn_ref.RefGCN(nfeat=nfeat, nhid=200, nclass=nclass, dropout=0.5)
        ms = run(ref, r8["features"], r8["adj"], target, tr, args.cpu_steps, lambda: None)
        print(json.dumps({"case": "R8 train step (fwd + bwd + Adam)", "impl": "oracle torch-CPU (reference ATen calls)",
                          "threads": torch.get_num_threads(), "ms_per_step": round(ms, 2),
                          "steps": args.cpu_steps}), flush=True)


if __name__ == "__main__":
    main()
