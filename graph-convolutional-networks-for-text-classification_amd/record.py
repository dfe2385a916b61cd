"""Whole-forward and whole-backward launch records (gcnk_gcn_forward_f32,
gcnk_gcn_backward_f32, include/gcnk.h).

The reference's trainer calls ``model.forward(features, adj)`` eagerly every
epoch (trainer.py:357 train, trainer.py:382 eval).  Issued op by op, the
forward's 4-5 launches each paid Python + ctypes marshalling, plan and
workspace lookups and device guards: 76-92 us per forward for ~26 us of
kernels (profiles/r03_eager_forward_host_profile.log).  A ForwardRecord holds,
per (adjacency, features, widths, stream), every pointer that does not change
between calls -- plans and their host headers, workspaces, counter regions,
the factored operands and the intermediates S1 / S2 -- in a C struct, and one
ctypes call issues the whole forward.

Which schedule a forward runs (dense-AX, hub-factored, SpMM + projection or
SpMM + GEMM), on which operands and plans, is decided in one place,
ops.choose_forward: a ForwardRecord is filled from the ForwardPath it returns
and ops.GCNFn's per-op path dispatches on the same value, so the launches,
their arguments and their order agree and results are bitwise the same.
"""
import ctypes
from collections import namedtuple

import torch

from . import _lib, derived, factor, ops
from .sparse import CSR

_c = ctypes


# gcnk_plan_ref, gcnk_gcn_fwd, gcnk_gcn_bwd as _lib reads them from include/gcnk.h
PlanRef, GcnFwd, GcnBwd = (_lib.STRUCTS[name] for name in ("gcnk_plan_ref", "gcnk_gcn_fwd", "gcnk_gcn_bwd"))
FACTORED, SPMM_PROJ, SPMM_GEMM, DENSE_AX = ops.FWD_FACTORED, ops.FWD_SPMM_PROJ, ops.FWD_SPMM_GEMM, ops.FWD_DENSE_AX
KIND_NAMES = {FACTORED: "factored", SPMM_PROJ: "spmm+proj", SPMM_GEMM: "spmm+gemm", DENSE_AX: "dense-ax"}
BWD_AX_DIRECT = _lib.BWD_AX_DIRECT


def layout_ok():
    """The structs read from the header match the library's own layout (gcnk_gcn_fwd_layout)."""
    buf = (_c.c_int64 * 16)()
    n = _lib.load().gcnk_gcn_fwd_layout(buf, 16)
    want = [_c.sizeof(PlanRef), _c.sizeof(GcnFwd), GcnFwd.x.offset, GcnFwd.U.offset, GcnFwd.aF.offset,
            GcnFwd.aP.offset, GcnFwd.ld_h1_tmp.offset, PlanRef.lanes_hint.offset, _c.sizeof(GcnBwd),
            GcnBwd.xT.offset, GcnBwd.bwd2_ws_bytes.offset, GcnFwd.gc2_diag.offset]
    return n == len(want) and list(buf)[:n] == want


def _scratch(nbytes, device, keep):
    """(pointer, bytes) of a workspace of `nbytes`, (None, 0) for none.  (A
    record's launches take raw pointers: what they point into goes on `keep`.)"""
    ws = ops.workspace(nbytes, device)
    if ws is None:
        return None, 0
    keep.append(ws)
    return ws.data_ptr(), nbytes


def _matrix(rows, cols, device, keep):
    """(pointer, leading dimension) of an fp32 [rows x cols] intermediate."""
    t = torch.empty((rows, cols), dtype=torch.float32, device=device)
    keep.append(t)
    return t.data_ptr(), cols


def _gemm_operand(s, x, M, N, K, trans, device, keep):
    """Dense `x` as left operand of the record's [M x N x K] GEMM (ops.gemm's K-slabs)."""
    s.x_dense, s.ldx = x.data_ptr(), x.stride(0)
    s.x_split_k = ops.default_split_k(M, N, K, trans=trans)
    keep.append(x)
    s.gemm_ws, s.gemm_ws_bytes = _scratch(int(_lib.load().gcnk_gemm_workspace_bytes(M, N, K, s.x_split_k)),
                                          device, keep)


def _fill_plan(ref, plan, F, lanes, device, keep):
    """PlanRef for `plan` at width F: its header, a workspace and the counter
    region torch's current stream uses (Plan.counters)."""
    ref.plan = plan.buf.data_ptr()
    for i in range(16):
        ref.hdr[i] = plan.hdr[i]
    ref.workspace, ref.workspace_bytes = _scratch(plan.workspace_bytes(F), device, keep)
    cnt = plan.counters(device)
    if cnt is not None:
        keep.append(cnt)
        ref.counters, ref.counter_bytes = cnt.data_ptr(), 4 * cnt.numel()
    ref.lanes_hint = int(lanes)
    keep.append(plan)


class ForwardRecord:
    """One gcnk_gcn_fwd filled from ops.choose_forward's ForwardPath, plus the
    tensors and plans it points into."""

    __slots__ = ("s", "keep", "kind", "dax", "M", "F", "P", "pinned", "__weakref__")

    def __init__(self, adj, xop, F, P, device, train=False):
        p = ops.choose_forward(adj, xop, F, P, train)
        M = adj.shape[0]
        s = GcnFwd()
        keep = []
        s.kind, s.M, s.F, s.P = p.kind, M, F, P
        if p.kind == DENSE_AX:
            # gc1 from the cached A-hat X: no first product, no F-wide plan
            s.Kc, s.U, s.ldu = p.dax.K, p.dax.AX.data_ptr(), p.dax.AX.stride(0)
            keep.append(p.dax.AX)
        elif p.kind == FACTORED:
            fac = p.fac
            s.Kc, s.nhub, s.k0, s.rec_words = fac.Kc, fac.H, fac.k0, fac.rec_words
            s.U, s.ldu, s.rec = fac.U.data_ptr(), fac.U.stride(0), fac.rec.data_ptr()
            keep += [fac.U, fac.rec]
            if ops.FACTOR_GC2 and fac.diag is not None:   # gc2's aggregation from the factor too (hub ids / row pointers: host arrays)
                s.gc2_diag, s.gc2_pre = fac.diag.data_ptr(), fac.pre.data_ptr()
                s.gc2_hub_ids, s.gc2_hub_rp = fac.hub_ids_h.ctypes.data, fac.a_hub_rp_h.ctypes.data
                s.gc2_hub_ci, s.gc2_hub_val = fac.a_hub_ci.data_ptr(), fac.a_hub_val.data_ptr()
                keep += [fac.diag, fac.pre, fac.hub_ids_h, fac.a_hub_rp_h, fac.a_hub_ci, fac.a_hub_val]
        else:
            # H1 scratch for an eval forward: the unfused path's intermediate, and
            # the fused path's fallback where the library refuses the fusion (an
            # operand it cannot take as float4, gcnk_gcn_forward_f32)
            s.h1_tmp, s.ld_h1_tmp = _matrix(M, F, device, keep)
            _fill_plan(s.aF, p.plan_f, F, p.lanes, device, keep)
        if p.kind != DENSE_AX:
            # the first product S1 = X W1 (factored: S_T = X_hubs W1); H1 W2 runs unsplit
            rows, cols = s.x_rows, s.x_cols = p.x.shape
            if isinstance(p.x, CSR):
                _fill_plan(s.x, ops.plan_for(p.x, F), F, 0, device, keep)
            else:
                _gemm_operand(s, p.x, rows, F, cols, False, device, keep)
            s.s1, s.lds1 = _matrix(rows, F, device, keep)
        s.s2, s.lds2 = _matrix(M, P, device, keep)
        _fill_plan(s.aP, p.plan_p, P, 0, device, keep)   # gc2's aggregation A S2 + b2 (ops.spmm, lanes 0)
        self.s, self.keep, self.kind, self.dax, self.M, self.F, self.P = s, keep, p.kind, p.dax, M, F, P
        self.pinned = False   # (set once a hipGraph is captured through this record: derived.py)

    def run(self, W1, b1, W2, b2, epi, store_h1, stream):
        """(out, H1, self.dax) of one forward with ops.Epilogue `epi`; H1 is None unless store_h1."""
        dev = W1.device
        out = torch.empty((self.M, self.P), dtype=torch.float32, device=dev)
        H1 = torch.empty((self.M, self.F), dtype=torch.float32, device=dev) if store_h1 else None
        rc = _lib.load().gcnk_gcn_forward_f32(
            _c.byref(self.s), W1.data_ptr(), b1.data_ptr() if b1 is not None else None, W2.data_ptr(),
            b2.data_ptr() if b2 is not None else None, out.data_ptr(), self.P,
            H1.data_ptr() if H1 is not None else None, self.F, *epi.c_args(), stream)
        _lib.check(rc, "gcnk_gcn_forward_f32")
        return out, H1, self.dax


class BackwardRecord:
    """One filled gcnk_gcn_bwd: ops.GCNFn.backward's launches (A-hat^T G, the
    fused gcn_bwd2, A-hat^T gZ1, X^T gS1) with their plans, workspaces and
    scratch, issued by one ctypes call (bitwise the per-op backward).  `dax`:
    the forward's DenseAX (GCNFn's ctx.dax): gW1 = (A-hat X)^T gZ1 directly."""

    __slots__ = ("s", "keep", "M", "F", "P", "x_cols", "pinned", "__weakref__")

    def __init__(self, adj, xop, F, P, device, dax=None):
        M = adj.shape[0]
        s = GcnBwd()
        keep = []
        s.M, s.F, s.P = M, F, P
        adjT = adj.t()
        keep.append(adjT)
        for ref, width in ((s.aTP, P), (s.aTF, F)) if dax is None else ((s.aTP, P),):
            _fill_plan(ref, ops.plan_for(adjT, width), width, 0, device, keep)
        rows, cols = s.x_rows, s.x_cols = xop.shape
        if dax is not None:
            s.flags = BWD_AX_DIRECT
            s.x_rows, s.x_cols = M, dax.K
            _gemm_operand(s, dax.AX, dax.K, F, M, True, device, keep)
        elif xop.csr is not None:    # X^T gS1 = spmm(X^T, gS1)  (ops.Operand.t_times)
            xT = xop.csr.t()
            keep.append(xT)
            _fill_plan(s.xT, ops.plan_for(xT, F), F, 0, device, keep)
        else:                        # gemm(X, gS1, transA=True)
            _gemm_operand(s, xop.dense, cols, F, rows, True, device, keep)
        s.gS2, s.gZ1 = _matrix(M, P, device, keep)[0], _matrix(M, F, device, keep)[0]
        if dax is None:
            s.gS1 = _matrix(rows, F, device, keep)[0]
        s.bwd2_ws, s.bwd2_ws_bytes = _scratch(int(_lib.load().gcnk_gcn_bwd2_workspace_bytes(M, F, P)), device, keep)
        self.s, self.keep, self.M, self.F, self.P, self.x_cols = s, keep, M, F, P, cols
        self.pinned = False

    def run(self, G, H1, W2, scale, want_gw1, want_gb1, want_gw2, want_gb2, stream):
        """(gW1, gb1, gW2, gb2), each None unless wanted."""
        dev = G.device
        gW1 = torch.empty((self.x_cols, self.F), dtype=torch.float32, device=dev) if want_gw1 else None
        gb1 = torch.empty(self.F, dtype=torch.float32, device=dev) if want_gb1 else None
        gW2 = torch.empty((self.F, self.P), dtype=torch.float32, device=dev) if want_gw2 else None
        gb2 = torch.empty(self.P, dtype=torch.float32, device=dev) if want_gb2 else None
        rc = _lib.load().gcnk_gcn_backward_f32(
            _c.byref(self.s), G.data_ptr(), H1.data_ptr(), H1.stride(0), W2.data_ptr(), scale,
            gW1.data_ptr() if gW1 is not None else None, gb1.data_ptr() if gb1 is not None else None,
            gW2.data_ptr() if gW2 is not None else None, gb2.data_ptr() if gb2 is not None else None, stream)
        _lib.check(rc, "gcnk_gcn_backward_f32")
        return gW1, gb1, gW2, gb2


# adj._records (a derived.Cache of 8) maps what a record was built for (tag "fwd" /
# "bwd", X's id, widths, stream) and the knobs it was built under (ops.FACTOR_GC1,
# ops.FUSE_PROJECTION, ops.DENSE_AX, factor.XHUB_DENSE; variant: fwd, the pair (a
# training forward where X[hubs] may take its training form, ops.FACTOR_GC2); bwd,
# gW1 from the forward's A-hat X) to the record built from (adj, X); values() and items() show an entry as
# Cached (the sources (adj, X), their stamp, the record).
RecordKey = namedtuple("RecordKey", "tag src_id F P stream factor_gc1 fuse_projection dense_ax xhub_dense variant")
Cached = namedtuple("Cached", "srcs stamp rec")

# records (and plans) displaced from their cache while a captured graph still
# points into them, and the call that drops them once those graphs are gone
_PINNED, release_pinned = derived.PINNED, derived.release_pinned


def get_backward(adj, xop, F, P, device, dax=None):
    """(record, stream): the BackwardRecord of (adj, X, F, P) for torch's
    current stream, built on first use, and that stream.  ``dax``: the DenseAX
    the forward ran on, if it did (GCNFn's ctx.dax)."""
    return _get(adj, xop, F, P, device, BackwardRecord, "bwd", dax is not None, dax)


def get(adj, xop, F, P, device, train=False):
    """(record, stream): the ForwardRecord of (adj, X, F, P) for torch's current
    stream, built on first use, and that stream.  ``train``: a forward whose H1
    the backward keeps (its X_hubs W1 may take another form, factor.hub_operand)."""
    return _get(adj, xop, F, P, device, _forward_record, "fwd",
                (bool(train) and factor.XHUB_TRAIN_TILE, ops.FACTOR_GC2), train)


def _forward_record(adj, xop, F, P, device, train):
    """The training forward's record is the eval forward's wherever the mode
    does not change the path (all but a factored gc1 whose X[hubs] has both
    forms): one set of S1 / S2 / H1 scratch, filed under both keys."""
    if train and factor.XHUB_TRAIN_TILE:
        p = ops.choose_forward(adj, xop, F, P, True)
        if p.kind != FACTORED or p.fac.hub_operand(True) == p.fac.hub_operand(False):
            return get(adj, xop, F, P, device)[0]
    return ForwardRecord(adj, xop, F, P, device, train)


def _get(adj, xop, F, P, device, build, tag, variant, arg):
    """A record's launches bake in raw pointers to its scratch buffers, so a
    record is rebuilt when either operand's values change in place (the
    factored operands and plans are derived from them) and a record that was
    used while a hipGraph was being captured is pinned (derived.py): the graph keeps
    replaying into its buffers.  A record's scratch (S1, S2, H1) is shared by
    every launch on its stream; a graph captured on that stream replays into it, so two
    graphs of the same record must not replay concurrently.  ``arg``: build's last argument."""
    stream = torch.cuda.current_stream(device).cuda_stream
    src = xop.csr if xop.csr is not None else xop.dense
    # RecordKey's fields as a plain tuple: it finds the stored RecordKey (equal,
    # same hash) without building one on every call
    key = (tag, id(src), F, P, stream, ops.FACTOR_GC1, ops.FUSE_PROJECTION, ops.DENSE_AX, factor.XHUB_DENSE, variant)
    recs = adj.__dict__.get("_records")
    if recs is None:
        recs = derived.cache_of(adj, "_records", 8, RecordKey, Cached)
    rec = recs.get(key, (adj, src), build, adj, xop, F, P, device, arg)
    if torch.cuda.is_current_stream_capturing():
        rec.pinned = True
    return rec, stream
