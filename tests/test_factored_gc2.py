"""gcnk_hubfactor_gc2_f32 (csrc/factor_gc2.hip): gc2's aggregation A-hat S2 + b2
from the hub factor, on hand-built operands the analyzer would never produce,
and the factor build's new operands on the R8 fixture.

Operands are made by hand (block records packed by tests/hub_records.py; diag and
the precede counts per position of the block order; the hub rows as a CSR), so
the expected values are float64 sums of the same arrays and no row is left out.
The bound is the one tests/test_gpu_parity.py applies to its F = 8 SpMM
comparison against csr_ref (_close's defaults): |err| <= 1e-5 + 1e-5 |ref|.
Values are A-hat-like (a row's values sum to at most 1), S2 is N(0, 1).

The kernel runs 256 threads: a hub row is dealt over G = 256 / (P / 4) lane
groups, 16 items each per pass, so one pass covers 16 G items -- G = 256, 128,
85, 32 and passes of 4096, 2048, 1360, 512 items at P = 4, 8, 12, 32.  The hub
rows of the large case have every length on and across those boundaries (one
item per group: G - 1, G, G + 1; one pass: 16 G - 1, 16 G, 16 G + 1) beside 0,
1, 255, 256, 257, 2048, 2049 and 5000.

Document rows: diagonal only, no diagonal, 1 and 17 hub items, the diagonal's
column between two hub columns (a precede count that is neither 0 nor all), an
empty row after a long one.  A document row is one fma chain from +0 in CSR
column order, then the bias -- the order of spmm_row_kernel for a row of one
unit (at most default_ipc nonzeros) -- so those rows must be bit for bit
ops.spmm's on the same CSR (dense tile blocks off).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, _lib, factor, ops
from graph_convolutional_networks_for_text_classification_amd.sparse import as_csr, from_arrays

from hub_records import REC_HEAD, ROWS, pack, rec_words_for

DEV = "cuda"
GUARD = 8
NAN_BITS = np.int32(0x7FC00000)
LOGIT_TOL = 1e-4            # tests/test_gpu_parity.py
TRAINED_LOGIT_TOL = 3e-4    # tests/test_gpu_parity.py (trained-model logits up to |190|)

BOUNDARY = [g + d for P4 in (1, 2, 3, 8) for g in (256 // P4, 16 * (256 // P4)) for d in (-1, 0, 1)]
LARGE_LENGTHS = sorted(set([0, 1, 255, 256, 257, 2048, 2049, 5000] + BOUNDARY))
CASES = {
    # name: (M, hub row ids, hub row lengths)
    "m70_h3": (70, [5, 40, 66], [70, 9, 33]),          # a partial last block; hub 0's row is full (hub columns + diagonal)
    "m96_h1": (96, [50], [60]),
    "m5100": (5100, None, LARGE_LENGTHS),              # hubs spread over the rows
}
# document row patterns by position in the block order: (diagonal, hub items, which)
PATTERNS = [(True, 0, "any"), (False, 1, "any"), (True, 1, "any"), (True, 17, "any"), (False, 0, "any"),
            (True, 6, "around"), (True, 2, "any"), (False, 3, "any"), (True, 13, "any")]


@functools.lru_cache(maxsize=None)
def _structure(name):
    """Rows (sorted columns, values) of an A-hat-like matrix with the case's hub
    rows, a random block order, and the kernel's operands built from them."""
    M, hubs, lengths = CASES[name]
    rng = np.random.default_rng(len(name) * 1000 + M)
    H = len(lengths)
    if hubs is None:
        hubs = np.unique(np.linspace(3, M - 4, H).astype(np.int64))
    hubs = np.asarray(hubs, np.int64)
    assert len(hubs) == H and np.all(np.diff(hubs) > 0)
    hub_index = np.full(M, -1, np.int64)
    hub_index[hubs] = np.arange(H)
    perm = rng.permutation(M)
    pos_of = np.empty(M, np.int64)
    pos_of[perm] = np.arange(M)
    cols, vals = [None] * M, [None] * M
    full = int(np.argmax(np.asarray(lengths) >= min(M, H + 1)))   # this hub row holds every hub column and its diagonal
    for j, (r, L) in enumerate(zip(hubs, lengths)):
        c = rng.choice(M, size=L, replace=False)
        if j == full and L >= H + 1:
            rest = np.setdiff1d(np.arange(M), hubs)
            c = np.concatenate([hubs, rng.choice(rest, size=L - H, replace=False)])
            assert r in c
        cols[r] = np.sort(c)
        vals[r] = (rng.uniform(0.5, 1.0, L) / (L + 1)).astype(np.float32)
    for r in range(M):
        if hub_index[r] >= 0:
            continue
        dg, n, which = PATTERNS[pos_of[r] % len(PATTERNS)]
        if which == "around" and H >= 2:    # hub columns on both sides of r where the hubs allow it
            below, above = hubs[hubs < r], hubs[hubs > r]
            hc = np.concatenate([below[-3:], above[:3]])
        else:
            # (fewer than n distinct hubs: repeated hub columns -- items are items to the kernel)
            hc = rng.choice(hubs, size=n, replace=n > H)
        c = np.sort(np.concatenate([hc, [r]] if dg else [hc]).astype(np.int64), kind="stable")
        cols[r] = c
        vals[r] = (rng.uniform(0.5, 1.0, len(c)) / (len(c) + 1)).astype(np.float32)
    # the kernel's operands
    nblk = (M + ROWS - 1) // ROWS
    npos = nblk * ROWS
    diag, pre = np.zeros(npos, np.float32), np.zeros(npos, np.int32)
    items = [[] for _ in range(npos)]
    for p in range(M):
        r = perm[p]
        isd = cols[r] == r
        hubcol = hub_index[cols[r]] >= 0
        items[p] = [(hub_index[c], v) for c, v in zip(cols[r][hubcol & ~isd], vals[r][hubcol & ~isd])]
        if hub_index[r] >= 0:
            pre[p] = -1        # (its items stay in the record, as the factored gc1 reads them: skipped here)
            if isd.any():      # a hub row's own diagonal is a hub column: gc1's record holds it as an item
                items[p] = [(hub_index[c], v) for c, v in zip(cols[r][hubcol], vals[r][hubcol])]
        else:
            assert isd.sum() <= 1
            diag[p] = vals[r][isd][0] if isd.any() else 0.0
            pre[p] = int(np.sum(hubcol & (cols[r] < r)))
    counts = np.array([len(it) for it in items])
    rec_words = rec_words_for(counts, tail=4)    # every record keeps a tail
    rec = pack(items, perm, M, rec_words, NAN_BITS)
    hub_rp = np.concatenate([[0], np.cumsum([len(cols[r]) for r in hubs])]).astype(np.int32)
    hub_ci = np.concatenate([cols[r] for r in hubs] + [np.zeros(1, np.int64)]).astype(np.int32)   # (never empty)
    hub_val = np.concatenate([vals[r] for r in hubs] + [np.zeros(1, np.float32)]).astype(np.float32)
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    colind = np.concatenate(cols).astype(np.int32)
    val = np.concatenate(vals).astype(np.float32)
    if H >= 2:   # (one hub: a row's items all lie on one side of its diagonal)
        assert any(0 < pre[p] < counts[p] for p in range(M)), "a precede count that is neither 0 nor all"
    assert (pre[:M] > 0).any() and (diag[:M][pre[:M] >= 0] == 0).any()
    return dict(M=M, H=H, hubs=hubs.astype(np.int32), hub_index=hub_index, perm=perm, rec=rec, rec_words=rec_words,
                diag=diag, pre=pre, hub_rp=hub_rp, hub_ci=hub_ci, hub_val=hub_val, rowptr=rowptr, colind=colind,
                val=val, nnz_row=np.diff(rowptr))


@functools.lru_cache(maxsize=None)
def _device(name):
    s = _structure(name)
    d = {k: torch.from_numpy(s[k]).to(DEV) for k in ("rec", "diag", "pre", "hub_ci", "hub_val")}
    d["csr"] = from_arrays(s["rowptr"], s["colind"], s["val"], (s["M"], s["M"]), DEV)
    return d


@functools.lru_cache(maxsize=None)
def _dense(name, P):
    """(S2, b2, float64 A S2) for the case at width P, computed once."""
    s = _structure(name)
    rng = np.random.default_rng(P)
    S2 = rng.standard_normal((s["M"], P)).astype(np.float32)
    b2 = rng.standard_normal(P).astype(np.float32)
    want = np.zeros((s["M"], P))
    rows = np.repeat(np.arange(s["M"]), s["nnz_row"])
    np.add.at(want, rows, s["val"].astype(np.float64)[:, None] * S2[s["colind"]].astype(np.float64))
    return S2, b2, want


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _call(name, S2, b2, out, M=None, H=None, P=None, rec=None, stream=None):
    """The C entry on the case's operands; S2 / out are [M x P] views whose row stride is the ld."""
    s, d = _structure(name), _device(name)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    return _lib.load().gcnk_hubfactor_gc2_f32(
        s["M"] if M is None else M, s["H"] if H is None else H, S2.shape[1] if P is None else P,
        _p(d["rec"] if rec is None else rec), s["rec_words"], _p(d["diag"]), _p(d["pre"]), s["hubs"].ctypes.data,
        s["hub_rp"].ctypes.data, _p(d["hub_ci"]), _p(d["hub_val"]), _p(S2), S2.stride(0), _p(b2), _p(out),
        out.stride(0), stream)


def _guarded(M, P, ld, fill=None):
    """(buffer, [M x P] view at row stride ld) with GUARD rows before and after and ld - P guard columns, all NaN."""
    buf = torch.full((M + 2 * GUARD, ld), float("nan"), device=DEV)
    view = buf[GUARD:GUARD + M, :P]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _guards_intact(buf, M, P):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + M:]).all()) and \
        bool(torch.isnan(buf[:, P:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("P", [4, 8, 12, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_gc2_matches_float64_and_the_row_kernel(name, P):
    """Every row against float64 within the F = 8 SpMM bound, with and without
    b2, at ld = P and at ld > P with NaN guard rows and columns that stay NaN;
    every launch twice with equal bits; document rows of one unit bit for bit
    ops.spmm's."""
    s, d = _structure(name), _device(name)
    M = s["M"]
    S2h, b2h, want0 = _dense(name, P)
    S2t, b2t = torch.from_numpy(S2h).to(DEV), torch.from_numpy(b2h).to(DEV)
    is_doc = s["hub_index"] < 0
    one_unit = torch.from_numpy(is_doc & (s["nnz_row"] <= ops.default_ipc(d["csr"], P))).to(DEV)
    assert int(one_unit.sum()) > 0.5 * M
    worst = 0.0
    for bias in (b2t, None):
        want = want0 + (b2h.astype(np.float64) if bias is not None else 0.0)
        ref = ops.spmm(d["csr"], S2t, bias=bias, epilogue=_lib.EPI_BIAS if bias is not None else _lib.EPI_NONE,
                       dense=2.0)
        for ld_s, ld_o in ((P, P), (P + 4, P + 8)):
            sbuf, S2v = _guarded(M, P, ld_s, S2t)
            outs = []
            for _ in range(2):
                obuf, out = _guarded(M, P, ld_o)
                _lib.check(_call(name, S2v, bias, out), "gcnk_hubfactor_gc2_f32")
                torch.cuda.synchronize()
                assert _guards_intact(obuf, M, P), (name, P, ld_o)
                outs.append(out.clone())
            assert torch.equal(outs[0], outs[1]), "two launches, different bits"
            got = outs[0].double().cpu().numpy()
            assert np.isfinite(got).all()
            ratio = np.abs(got - want) / (1e-5 + 1e-5 * np.abs(want))
            worst = max(worst, float(ratio.max()))
            print(f"{name} P={P} bias={bias is not None} ld=({ld_s},{ld_o}): max err / bound = {ratio.max():.3f} "
                  f"(hub rows {ratio[~is_doc].max():.3f})")
            assert ratio.max() <= 1.0, (name, P, float(ratio.max()))
            assert torch.equal(outs[0][one_unit], ref[one_unit]), "document rows differ from the row kernel's bits"
    print(f"{name} P={P}: largest ratio to the bound {worst:.3f}")


@pytest.mark.gpu
def test_gc2_ignores_record_tails_and_hub_positions():
    """The records' unused tails are NaN bits and the hub rows' positions hold
    items: poisoning those items' values too changes nothing."""
    name, P = "m70_h3", 8
    s, d = _structure(name), _device(name)
    S2h, b2h, _ = _dense(name, P)
    S2t, b2t = torch.from_numpy(S2h).to(DEV), torch.from_numpy(b2h).to(DEV)
    out = torch.empty((s["M"], P), device=DEV)
    _lib.check(_call(name, S2t, b2t, out), "gcnk_hubfactor_gc2_f32")
    rec = s["rec"].copy()
    for p in np.flatnonzero(s["pre"][:s["M"]] < 0):
        b, i = divmod(int(p), ROWS)
        lo, hi = rec[b, i], rec[b, i + 1]
        rec[b, REC_HEAD + 2 * lo:REC_HEAD + 2 * hi] = NAN_BITS
    assert not np.array_equal(rec, s["rec"])
    out2 = torch.empty((s["M"], P), device=DEV)
    _lib.check(_call(name, S2t, b2t, out2, rec=torch.from_numpy(rec).to(DEV)), "gcnk_hubfactor_gc2_f32")
    assert torch.equal(out, out2) and bool(torch.isfinite(out).all())


@pytest.mark.gpu
def test_gc2_replays_from_a_captured_graph():
    name, P = "m5100", 8
    s = _structure(name)
    S2h, b2h, _ = _dense(name, P)
    S2t, b2t = torch.from_numpy(S2h).to(DEV), torch.from_numpy(b2h).to(DEV)
    eager = torch.empty((s["M"], P), device=DEV)
    _lib.check(_call(name, S2t, b2t, eager), "gcnk_hubfactor_gc2_f32")
    out = torch.zeros((s["M"], P), device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(_call(name, S2t, b2t, out), "gcnk_hubfactor_gc2_f32")
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.gpu
def test_gc2_refusals_write_nothing():
    """P = 6, H = 129 and a misaligned out: GCNK_EUNSUP before any launch."""
    name = "m70_h3"
    s = _structure(name)
    M = s["M"]
    many = np.zeros(131, np.int32)

    def refused(P, out, **kw):
        S2 = torch.randn((M, P), device=DEV)
        before = out.clone()
        rc = _call(name, S2, None, out, **kw)
        torch.cuda.synchronize()
        return rc == _lib.EUNSUP and torch.equal(out, before)

    assert refused(6, torch.full((M, 6), 7.0, device=DEV))
    lib = _lib.load()
    d = _device(name)
    S2 = torch.randn((M, 8), device=DEV)
    out = torch.full((M, 8), 7.0, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.gcnk_hubfactor_gc2_f32(M, 129, 8, _p(d["rec"]), s["rec_words"], _p(d["diag"]), _p(d["pre"]),
                                    many.ctypes.data, many.ctypes.data, _p(d["hub_ci"]), _p(d["hub_val"]), _p(S2), 8,
                                    None, _p(out), 8, st)
    torch.cuda.synchronize()
    assert rc == _lib.EUNSUP and bool((out == 7.0).all())
    wide = torch.full((M, 12), 7.0, device=DEV)
    assert refused(8, wide[:, 1:9])               # out's rows start 4 bytes off a 16-B boundary
    assert bool((wide == 7.0).all())


def test_gc2_null_operands_are_bad_arguments():
    """No GPU needed: null operands are refused before anything is read."""
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    host = np.zeros(8, np.int32)
    hp = host.ctypes.data
    good = [70, 3, 8, p, 72, p, p, hp, hp, p, p, p, 8, None, p, 8, None]
    for i in (3, 5, 6, 7, 8, 9, 10, 11, 14):
        args = list(good)
        args[i] = None
        assert lib.gcnk_hubfactor_gc2_f32(*args) == _lib.EARG, i
    assert b"gcnk_hubfactor_gc2_f32" in lib.gcnk_last_error()
    for i, bad in ((0, 0), (1, 0), (2, 0), (4, 64), (4, 70), (12, 4), (15, 4)):   # sizes, record stride, lds
        args = list(good)
        args[i] = bad
        assert lib.gcnk_hubfactor_gc2_f32(*args) == _lib.EARG, i
    assert lib.gcnk_factor_diag_f32(None, p, p, 70, p, p, p, p, None) == _lib.EARG


@pytest.mark.gpu
def test_factor_build_gc2_operands_on_r8(r8):
    """diag (bit for bit), the precede counts and A-hat's hub rows as a CSR
    against a numpy restatement from r8["adj"]."""
    adj = r8["adj"].coalesce()
    M = adj.shape[0]
    rows, cols = adj.indices().numpy()
    vals = adj.values().numpy().astype(np.float32)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M))])
    f = factor.get(as_csr(r8["adj"].to(DEV)), ops.Operand(r8["features"].to(DEV)))
    assert f is not None and f.H == 50
    hubs, perm = f.hubs.numpy(), f.perm.numpy()
    is_hub = np.zeros(M, bool)
    is_hub[hubs] = True
    npos = f.nblk * ROWS
    diag, pre = np.zeros(npos, np.float32), np.zeros(npos, np.int32)
    for p in range(M):
        r = perm[p]
        c, v = cols[rp[r]:rp[r + 1]], vals[rp[r]:rp[r + 1]]
        if is_hub[r]:
            pre[p] = -1
            continue
        if (c == r).any():
            diag[p] = v[c == r][0]
        pre[p] = int(np.sum(is_hub[c] & (c < r)))
    assert np.array_equal(f.diag.cpu().numpy().view(np.int32), diag.view(np.int32))
    assert np.array_equal(f.pre.cpu().numpy(), pre)
    assert int((pre[:M] >= 0).sum()) == M - 50 and not pre[pre >= 0].any()   # R8: the documents precede the topics
    hrp = np.concatenate([[0], np.cumsum(rp[hubs + 1] - rp[hubs])])
    assert np.array_equal(f.a_hub_rp.cpu().numpy(), hrp) and np.array_equal(f.a_hub_rp_h, hrp)
    assert np.array_equal(f.hub_ids_h, hubs)
    hci = np.concatenate([cols[rp[r]:rp[r + 1]] for r in hubs])
    hv = np.concatenate([vals[rp[r]:rp[r + 1]] for r in hubs])
    assert np.array_equal(f.a_hub_ci.cpu().numpy()[:hrp[-1]], hci)
    assert np.array_equal(f.a_hub_val.cpu().numpy()[:hrp[-1]].view(np.int32), hv.view(np.int32))


@pytest.mark.gpu
def test_r8_forward_with_and_without_factored_gc2(r8, golden_logits, trained_golden, monkeypatch):
    """R8's eval forward with FACTOR_GC2 on and off: logits within LOGIT_TOL of
    the golden logits and the same labels; the reference's trained model (min
    top-2 gap 5.1e-3): the reference's label on every row, either way."""
    x, adj = r8["features"].to(DEV), r8["adj"].to(DEV)
    got, trained = {}, {}
    for on in (True, False):
        monkeypatch.setattr(ops, "FACTOR_GC2", on)
        torch.manual_seed(0)
        m = GCN(nfeat=r8["nfeat"], nhid=200, nclass=r8["nclass"], dropout=0.5).to(DEV).eval()
        with torch.no_grad():
            got[on] = m(x, adj).cpu().numpy()
            m.load_state_dict(trained_golden["state_dict"])
            trained[on] = m(x, adj).cpu().numpy()
        err = float(np.abs(got[on] - golden_logits["eval_0"]).max())
        print(f"FACTOR_GC2={on}: max |logit - golden| = {err:.3e}")
        assert err <= LOGIT_TOL
        assert np.abs(trained[on] - trained_golden["logits"]).max() <= TRAINED_LOGIT_TOL
        assert np.array_equal(trained[on].argmax(1), trained_golden["logits"].argmax(1))
    kinds = {k.variant for k, _ in as_csr(adj)._records.items() if k.tag == "fwd"}
    assert (False, True) in kinds and (False, False) in kinds, kinds    # one record per setting
    assert np.array_equal(got[True].argmax(1), got[False].argmax(1))
    diff = got[True] != got[False]
    print(f"on vs off: {int(diff.sum())} of {diff.size} logits differ, largest {np.abs(got[True] - got[False]).max():.3e}")
