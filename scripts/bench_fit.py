"""R8 training loop timing: what an epoch costs when the loop itself is on the
device (train.fit) against the loop written by hand.

One process, the R8 fixture, the device's own dropout masks, every leg the same
number of epochs (patience is set out of reach, so no leg stops early):

  (a) the hand-written loop of tests/test_native_train_step.py: train.Adam,
      train.IndexedCrossEntropy, metrics.evaluate_with_loss and a Python
      EarlyStopping, two host syncs per epoch (needs nothing newer than those:
      this leg runs on an older tree too);
  (b) train.fit eager, poll_every=1;
  (c) train.fit from a hipGraph, poll_every=16;
  (d) (c) with restore_best=True: a gcnk_keep_best_f32 launch behind every
      epoch tail and the restore at the end.  After (c) on its own, (c) and (d)
      are run alternately, run by run, so that drift of the box falls on both;
      (d) also reports how many of its epochs copied and which epoch it restored.

Per-epoch time = wall time of the whole run / epochs (for fit: the call, its
eager first epoch and its capture included), median and spread (max - min) of
--runs runs.  Then, as graph replays of --reps launches each (kernel time, no
host time between launches): the fused epoch tail alone beside the four nodes
it replaces (memset, class stats, loss forward, loss reduce), and the Adam
launch with no gate beside the gated one with its gate open.  (The keep
launch alone is scripts/keep_probe.py.)

Prints one JSON line per case.

usage: python scripts/bench_fit.py [--epochs 97] [--runs 5] [--reps 20] [--replay-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=97, help="epochs per run (1 eager + 6 x 16 replays in leg c)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="launches per graph replay in the kernel-alone legs")
    ap.add_argument("--replay-only", action="store_true",
                    help="only the captured epoch alone, without and with the keeper, twice each")
    args = ap.parse_args()

    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import GCN, datasets, metrics, train
    from oracle import gcn_ref

    dev = torch.device("cuda", 0)
    r8 = datasets.load_r8_fixture(os.path.join(ROOT, "tests", "golden", "r8_graph.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "r8_meta.json")) as f:
        run = json.load(f)["train_runs"]["50494"]
    nfeat, nclass = r8["nfeat"], r8["nclass"]
    x, adj = r8["features"].to(dev), r8["adj"].to(dev)
    tgt = torch.as_tensor(r8["target"]).long().to(dev)
    tr = torch.as_tensor(run["train_idx"]).long().to(dev)
    va = torch.as_tensor(run["val_idx"]).long().to(dev)
    E, far = args.epochs, 10 ** 6   # a patience no run reaches
    have_fit = hasattr(train, "fit")
    have_keep = hasattr(train, "BestKeeper")

    def model_():
        torch.manual_seed(50494)
        np.random.seed(50494)
        return GCN(nfeat=nfeat, nhid=200, nclass=nclass, dropout=0.5, dropout_rng="device").to(dev)

    def hand_loop():
        model = model_()
        opt = train.Adam(model.parameters(), lr=0.02)
        crit = train.IndexedCrossEntropy()
        stopper = gcn_ref.EarlyStopping(far)
        history = []
        for epoch in range(E):
            model.train()
            opt.zero_grad()
            loss = crit(model(x, adj), tgt, tr)
            loss.backward()
            opt.step()
            model.eval()
            with torch.no_grad():
                acc, f1, p, r, vl = metrics.evaluate_with_loss(model(x, adj), tgt, va, nclass)
            history.append(dict(epoch=epoch, train_loss=loss.item(), val_loss=vl, acc=acc, macro_f1=f1, precision=p,
                                recall=r))
            if stopper(vl):
                break
        return history

    # the captured epoch alone: HIP events around 96 replays of train.run_epoch's graph, nothing read back
    def captured(with_keeper):
        model = model_()
        log = train.EpochLog(10 ** 4, nclass, dev, patience=far)
        opt = train.Adam(model.parameters(), lr=0.02, gate=log.stop_word)
        ep = (model, x, adj, tgt, tr, va, opt, log)
        kw = {"keeper": train.BestKeeper(list(model.parameters()), log)} if with_keeper else {}
        train.run_epoch(*ep, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            train.run_epoch(*ep, **kw)
        g.replay()
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(96):
                g.replay()
            e1.record()
            e1.synchronize()
            runs.append(e0.elapsed_time(e1) / 96)
        res = {"case": "R8 epoch (train step + eval forward + epoch tail" + (" + keep" if with_keeper else "") +
                       "), hipGraph replay alone",
               "ms_per_epoch": round(statistics.median(runs), 4), "runs_ms": [round(r, 4) for r in runs],
               "spread_ms": round(max(runs) - min(runs), 4), "epochs_recorded": log.poll()[0],
               "optimizer_steps": opt.steps}
        if with_keeper:
            res["copying_epochs"] = log.keeper.state().copies
        print(json.dumps(res), flush=True)
        del g

    if args.replay_only:
        for _ in range(2):
            captured(False)
            if have_keep:
                captured(True)
        return

    kept = {}

    def fit_(graph, poll, **kw):
        res = train.fit(model_(), x, adj, tgt, tr, va, lr=0.02, max_epoch=E, patience=far, graph=graph,
                        poll_every=poll, **kw)
        assert res.epochs == E and res.stop_reason == 2
        if kw:
            st = res.log.keeper.state()
            kept.update(copying_epochs=st.copies, best_epoch=res.log.best_epoch,
                        val_loss_is_the_minimum=res.history[st.best - 1]["val_loss"] == min(
                            h["val_loss"] for h in res.history))
        return res.history

    def legs(*named):
        """The legs alternately: run 1 of each, run 2 of each, ..."""
        for _, fn in named:
            fn()   # warm: plans, launch records, code objects
        torch.cuda.synchronize()
        runs, trace = {n: [] for n, _ in named}, {}
        for _ in range(args.runs):
            for name, fn in named:
                t0 = time.perf_counter()
                hist = fn()
                torch.cuda.synchronize()
                runs[name].append((time.perf_counter() - t0) / E * 1e3)
                trace[name] = hist
        out = []
        for name, _ in named:
            r = runs[name]
            res = {"case": f"R8 training loop, {E} epochs, dropout_rng=device", "impl": name,
                   "ms_per_epoch": round(statistics.median(r), 4), "runs_ms": [round(v, 4) for v in r],
                   "spread_ms": round(max(r) - min(r), 4), "epochs": len(trace[name]),
                   "last_epoch": {k: (round(v, 6) if isinstance(v, float) else v)
                                  for k, v in trace[name][-1].items()}}
            print(json.dumps(res), flush=True)
            out.append(res)
        return out

    a, = legs(("(a) hand-written loop: evaluate_with_loss + Python EarlyStopping, two syncs per epoch", hand_loop))
    if have_fit:
        b, = legs(("(b) train.fit eager, poll_every=1", lambda: fit_(False, 1)))
        c, = legs(("(c) train.fit hipGraph, poll_every=16", lambda: fit_(True, 16)))
        if have_keep:
            c2, d = legs(("(c) again, alternating with (d)", lambda: fit_(True, 16)),
                         ("(d) train.fit hipGraph, poll_every=16, restore_best=True",
                          lambda: fit_(True, 16, restore_best=True)))
            pairs = [round(y - x, 4) for x, y in zip(c2["runs_ms"], d["runs_ms"])]
            print(json.dumps({"case": "R8 epoch, what restore_best=True costs: (d) - (c), run by run (alternating)",
                              "c_ms": c2["ms_per_epoch"], "d_ms": d["ms_per_epoch"],
                              "cost_ms": round(d["ms_per_epoch"] - c2["ms_per_epoch"], 4),
                              "paired_cost_ms": pairs, "paired_cost_median_ms": round(statistics.median(pairs), 4),
                              "c_spread_ms": c2["spread_ms"], "d_spread_ms": d["spread_ms"], **kept,
                              "same_history": c2["last_epoch"] == d["last_epoch"]}), flush=True)
        gain = a["ms_per_epoch"] - c["ms_per_epoch"]
        print(json.dumps({"case": "R8 epoch, fit from a hipGraph (c) against the hand-written loop (a)",
                          "a_ms": a["ms_per_epoch"], "b_ms": b["ms_per_epoch"], "c_ms": c["ms_per_epoch"],
                          "a_spread_ms": a["spread_ms"], "c_spread_ms": c["spread_ms"], "gain_ms": round(gain, 4),
                          "c_beats_a_beyond_a_spread": gain > a["spread_ms"],
                          "same_last_epoch": a["last_epoch"] == c["last_epoch"] == b["last_epoch"]}), flush=True)

        captured(False)
        if have_keep:
            captured(True)

    # ---- single launches, as graph replays of `reps` launches (bench_train.py's `timed`)
    def timed(fn, reps=args.reps):
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
        return round(statistics.median(out), 3), round(max(out) - min(out), 3)

    model = model_().eval()
    with torch.no_grad():
        logits = model(x, adj)
        _, _, rc = train._prepare(logits, tgt, va)
        buf = torch.empty(3 * nclass + 2, dtype=torch.int32, device=dev)

        def four_nodes():   # evaluate_with_loss's launches without its copy
            metrics.class_stats(logits, tgt, va, out=buf)
            train._forward(logits, tgt, rc, False, loss=buf[3 * nclass + 1:].view(torch.float32))

        four_us, four_spread = timed(four_nodes)
        res = {"case": f"R8 validation tail ({va.numel()} of {logits.shape[0]} rows, {nclass} classes), "
                       f"{args.reps} per graph replay (warm caches)",
               "memset_stats_loss_reduce_us": four_us, "memset_stats_loss_reduce_spread_us": four_spread}
        if have_fit:
            log = train.EpochLog(args.reps * (args.runs + 4), nclass, dev, patience=far)
            tl = torch.ones(1, device=dev)
            tail_us, tail_spread = timed(lambda: log.record(logits, tgt, va, tl))
            assert log.poll() == (args.reps * (args.runs + 1) + 1, 0)
            res.update({"fused_tail_us": tail_us, "fused_tail_spread_us": tail_spread,
                        "tail_shorter_than_the_nodes_it_replaces": tail_us < four_us})
        print(json.dumps(res), flush=True)

    params = [p for p in GCN(nfeat=nfeat, nhid=200, nclass=nclass, dropout=0.5).to(dev).parameters()]
    for p in params:
        p.grad = torch.randn_like(p)
    numel = sum(p.numel() for p in params)
    opt = train.Adam(params, lr=0.02)
    adam_us, adam_spread = timed(opt.step)
    res = {"case": f"Adam step alone, R8 parameters, {args.reps} launches per graph replay (warm caches)",
           "numel": numel, "adam_gate_null_us": adam_us, "adam_gate_null_spread_us": adam_spread}
    if have_fit:
        opt.gate = torch.zeros(1, dtype=torch.int32, device=dev)
        res["adam_gate_open_us"], res["adam_gate_open_spread_us"] = timed(opt.step)
        opt.gate.fill_(1)
        res["adam_gate_closed_us"], res["adam_gate_closed_spread_us"] = timed(opt.step)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
