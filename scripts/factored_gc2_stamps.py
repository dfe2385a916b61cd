"""In-kernel timeline of gc2's aggregation from the hub factor
(csrc/factor_gc2.hip, factored_spmm_row_kernel) on R8 (needs the stamps build:
make -C <pkg>/csrc variant NAME=stamps DEFS=-DGCNK_STAMPS, then
GCNK_LIB=_variants/libgcnk_stamps.so).  Per workgroup s_memrealtime (100 MHz):
0 entry, 1 operands landed (hub rows: the last pass's items issued), 2 sums
done, 3 exit; percentiles in us from the first entry, cold (a fresh S2 per
call), the hub-row and the document workgroups reported apart."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import _lib, datasets, factor, ops
    from graph_convolutional_networks_for_text_classification_amd.sparse import as_csr
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    if os.environ.get("GCNK_STAMP_GRAPH") == "20ng":     # BASELINE config 3's shape: 70 hubs, 20 classes
        g = datasets.doc_topic_graph(18846, 70, 20, seed=0)
    else:
        g = datasets.load_r8_fixture(os.path.join(ROOT, "tests", "golden", "r8_graph.npz"))
    A, X = g["adj"].to(dev), g["features"].to(dev)
    f = factor.get(as_csr(A), ops.Operand(X))
    P = g["nclass"]
    print(json.dumps({"M": f.M, "H": f.H, "P": P, "rec_words": f.rec_words, "nblk": f.nblk}), flush=True)
    S2s = [torch.randn(f.M, P, device=dev) for _ in range(6)]
    b2 = torch.randn(P, device=dev) * 0.1
    for S2 in S2s:
        assert ops.hubfactor_gc2(f, S2, b2) is not None
    torch.cuda.synchronize()
    buf = torch.zeros(4 * 8192, dtype=torch.int64, device=dev)
    q = lambda x: [round(float(np.percentile(x, p)), 2) for p in (0, 10, 50, 90, 100)]  # noqa: E731
    for rep in range(4):
        S2 = torch.randn(f.M, P, device=dev)
        torch.cuda.synchronize()
        buf.zero_()
        assert lib.gcnk_debug_set_stamps(buf.data_ptr()) == 0
        ops.hubfactor_gc2(f, S2, b2)
        torch.cuda.synchronize()
        lib.gcnk_debug_set_stamps(None)
        s = buf.view(-1, 4).cpu().numpy().astype(np.float64)[:f.H + f.nblk]
        t0 = s[:, 0].min()
        rel = (s - t0) / 100.0
        for kind, part in (("hub rows", rel[:f.H]), ("documents", rel[f.H:])):
            worst = int(np.argmax(part[:, 3]))
            print(json.dumps({"rep": rep, "workgroups": kind, "n": len(part), "entry": q(part[:, 0]),
                              "operands_landed": q(part[:, 1] - part[:, 0]), "sums": q(part[:, 2] - part[:, 1]),
                              "to_exit": q(part[:, 3] - part[:, 2]), "exit": q(part[:, 3]),
                              "slowest": part[worst].round(2).tolist()}), flush=True)


if __name__ == "__main__":
    main()
