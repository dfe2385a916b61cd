"""The keep launch alone (gcnk_keep_best_f32, csrc/keep.hip) on R8's parameter
shapes -- 1,494,408 floats in four tensors: 5.98 MB read and 5.98 MB written
when it copies -- beside gcnk_stream_copy_f32 over the same bytes, the way the
Adam launch is judged against its floor.

Every keep launch here carries GCNK_KEEP_HOLD_STATE, so it decides from the
epoch state alone and leaves the keeper state as it is: with (epoch 1,
counter 0) every launch copies, with (epoch 1, counter 1) none does.  A last
leg runs the launch that does not copy WITHOUT the flag, as the fit loop
issues it: every workgroup then also arrives at the state's counter.

  python scripts/keep_probe.py [--reps 20] [--runs 7]
      graph replays of --reps launches each, HIP events, median and spread of
      --runs replays: one JSON line.  Under GCNK_LIB=<a `make variant` build> the
      same for that build (how the store policy, the place of the loads, the
      chunk and the workgroup size were A/B'd, with temporary -D switches in
      csrc/keep.hip that are no longer in the source: profiles/r17_keep_ab.log).
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/keep_probe.py --trace
  python scripts/keep_probe.py --report DIR
      kernel durations from the trace: N copying launches, N stream copies, N
      launches that do not copy, in that order, each after 3 warm ones.
"""
import argparse
import ctypes
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_TRACE, N_WARM = 30, 3


def report(d):
    import csv
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def us(name):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]

    keep, copy = us("keep_kernel"), us("stream_copy_kernel")
    assert len(keep) == 2 * (N_TRACE + N_WARM) and len(copy) == N_TRACE + N_WARM, (len(keep), len(copy))
    parts = {"keep_copies_us": keep[N_WARM:N_WARM + N_TRACE], "stream_copy_us": copy[N_WARM:],
             "keep_does_not_copy_us": keep[N_TRACE + 2 * N_WARM:]}
    out = {"case": f"kernel trace, {N_TRACE} launches each, eager"}
    for k, v in parts.items():
        out[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--report")
    args = ap.parse_args()
    if args.report:
        return report(args.report)

    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import GCN, _lib, datasets

    dev = torch.device("cuda", 0)
    r8 = datasets.load_r8_fixture(os.path.join(ROOT, "tests", "golden", "r8_graph.npz"))
    torch.manual_seed(0)
    params = [p.detach() for p in GCN(nfeat=r8["nfeat"], nhid=200, nclass=r8["nclass"], dropout=0.5).to(dev).parameters()]
    best = [torch.zeros_like(p) for p in params]
    numel = sum(p.numel() for p in params)
    flat_src, flat_dst = torch.randn(numel, device=dev), torch.zeros(numel, device=dev)
    lib = _lib.load()
    tab = (_lib.KeepTensor * len(params))()
    for k, (p, b) in enumerate(zip(params, best)):
        tab[k].src, tab[k].dst, tab[k].numel = p.data_ptr(), b.data_ptr(), p.numel()
    st = torch.zeros(4, dtype=torch.int32, device=dev)

    def epoch_state(counter):
        s = _lib.EpochState()
        s.epoch, s.counter = 1, counter
        return torch.frombuffer(bytearray(bytes(s)), dtype=torch.int32).to(dev)

    improved, worse = epoch_state(0), epoch_state(1)

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def keep(es):
        _lib.check(lib.gcnk_keep_best_f32(tab, len(params), es.data_ptr(), st.data_ptr(), _lib.KEEP_HOLD_STATE,
                                          stream()), "gcnk_keep_best_f32")

    def copy():
        _lib.check(lib.gcnk_stream_copy_f32(flat_src.data_ptr(), flat_dst.data_ptr(), numel, stream()),
                   "gcnk_stream_copy_f32")

    st2 = torch.zeros(4, dtype=torch.int32, device=dev)

    def keep_counting_in():   # without HOLD_STATE: every workgroup arrives at the state's counter; never fresh after the first
        _lib.check(lib.gcnk_keep_best_f32(tab, len(params), worse.data_ptr(), st2.data_ptr(), 0, stream()),
                   "gcnk_keep_best_f32")

    legs = [("keep_copies", lambda: keep(improved)), ("stream_copy", copy), ("keep_does_not_copy", lambda: keep(worse))]
    if args.trace:
        for _, fn in legs:
            for _ in range(N_WARM + N_TRACE):
                fn()
                torch.cuda.synchronize()
        assert all(torch.equal(p, b) for p, b in zip(params, best)) and not st.any()
        return

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.reps):
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
            out.append(e0.elapsed_time(e1) / args.reps * 1e3)
        return round(statistics.median(out), 3), round(max(out) - min(out), 3)

    res = {"case": f"keep launch alone, R8 parameters ({numel} floats), {args.reps} launches per graph replay (warm)",
           "lib": os.path.basename(_lib.LIB_PATH)}
    for name, fn in legs + [("keep_does_not_copy_updates_state", keep_counting_in)]:
        res[name + "_us"], res[name + "_spread_us"] = timed(fn)
    assert tuple(st2.cpu().tolist()) == (1, 0, 0, 0)
    assert all(torch.equal(p, b) for p, b in zip(params, best)) and not st.any()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
