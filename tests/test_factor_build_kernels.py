"""The hub factorisation's build kernels (csrc/factor_build.hip) at their own
entry points: gcnk_factor_u_f32, gcnk_aggregate_f32, gcnk_factor_analyze,
gcnk_factor_xl_f32, gcnk_factor_records, gcnk_factor_diag_f32,
gcnk_csr_gather_rows and gcnk_dense_gather_rows_f32.

factor.build reaches them only on well-formed doc-topic graphs, where whole
branches never run (a structure violation, more hubs than the list holds,
explicit zeros in X, a record that does not fit, padded and strided outputs).
Here each entry point is called through ctypes on hand-made int32 CSR arrays of
a few dozen rows.  Every expected value comes from plain numpy in this file;
the float64 sums run sequentially in item order and are rounded to fp32 once,
as the kernels' do, so every comparison is bitwise.  Every output buffer is
larger than the documented extent and pre-filled with a sentinel: a write
outside the extent fails the test.  Operands the kernels must not read (X's hub
rows for U, the columns past Kc or K) hold NaN.

The bad-argument checks at the end need no GPU.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

from hub_records import REC_HEAD, ROWS, pack

DEV = "cuda"
gpu = pytest.mark.gpu
SENT_F = np.float32(-12345.0)
SENT_I = np.int32(-777)
GUARD = 16                    # sentinel words before and after every output
INT_MAX = 2**31 - 1


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _csr(rows):
    """rowptr, colind, val (int32, int32, fp32) of a list of rows, each a list of (col, value), in the order given."""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    v = np.array([x for r in rows for _, x in r], np.float32)
    return rp, ci, v


class Out:
    """A device buffer [GUARD | n words | GUARD] full of a sentinel; .ptr is the address of word 0 of the body
    (off floats further on request), .get() the host copy after checking both guards."""

    def __init__(self, n, sentinel):
        self.n, self.sentinel = n, sentinel
        dtype = torch.float32 if isinstance(sentinel, np.float32) else torch.int32
        self.t = torch.full((n + 2 * GUARD,), sentinel.item(), dtype=dtype, device=DEV)
        assert self.t.data_ptr() % 16 == 0 and GUARD % 4 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def get(self):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == self.sentinel).all(), "written before the buffer"
        assert (h[GUARD + self.n:] == self.sentinel).all(), "written past the buffer"
        return h[GUARD:GUARD + self.n]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------ gcnk_factor_u_f32 / gcnk_aggregate_f32

N_SRC = 80                    # source rows (columns of the CSR, rows of Xl)
LONG = 70


@functools.lru_cache(maxsize=None)
def _u_graph(M):
    """M rows of 0 .. 9 items (i % 10) and one of 70 over N_SRC source rows, the sources with d % 5 == 2 hubs;
    a non-identity row order."""
    rng = np.random.default_rng(100 + M)
    lens = [i % 10 for i in range(M)]
    lens[M // 2] = LONG
    rows = []
    for n in lens:
        cols = np.sort(rng.choice(N_SRC, size=n, replace=False))
        rows.append([(int(c), np.float32(rng.standard_normal())) for c in cols])
    hub_index = np.full(N_SRC, -1, np.int32)
    hubs = np.flatnonzero(np.arange(N_SRC) % 5 == 2)
    hub_index[hubs] = np.arange(len(hubs))
    perm = rng.permutation(M).astype(np.int32)
    if M > 1 and np.array_equal(perm, np.arange(M)):
        perm = perm[::-1].copy()
    return rows, hub_index, perm


def test_u_graph_has_hub_items_in_the_unrolled_body_and_in_its_tail():
    """The precondition, on the arrays alone (no GPU)."""
    rows, hub_index, perm = _u_graph(37)
    body = tail = False
    for r in rows:
        cut = len(r) // 4 * 4
        body |= any(hub_index[c] >= 0 for c, _ in r[:cut])
        tail |= any(hub_index[c] >= 0 for c, _ in r[cut:])
    assert body and tail and not np.array_equal(perm, np.arange(37))
    assert sorted(len(r) for r in rows)[-1] == LONG and {len(r) for r in rows} >= set(range(10))


def _u_reference(rows, order, skip, X, Kc, Kcp):
    """fp32(sum in item order, in float64, of val * X[col, :Kc]) per output position; +0 in the pad columns."""
    out = np.zeros((len(order), Kcp), np.float32)
    for p, r in enumerate(order):
        acc = np.zeros(Kc, np.float64)
        for c, v in rows[r]:
            if skip is not None and skip[c] >= 0:
                continue
            acc = acc + np.float64(v) * X[c, :Kc].astype(np.float64)
        out[p, :Kc] = acc.astype(np.float32)
    return out


def _x_sources(Kc, ldxl, hub_index, seed):
    """[1 float | N_SRC x ldxl] on the device: the rows start 4 bytes off a 16-byte boundary; NaN in the columns
    past Kc and, with a hub index, in the hub rows."""
    rng = np.random.default_rng(seed)
    X = np.full((N_SRC, ldxl), np.nan, np.float32)
    X[:, :Kc] = rng.standard_normal((N_SRC, Kc)).astype(np.float32)
    if hub_index is not None:
        X[hub_index >= 0] = np.nan
    flat = np.concatenate([np.full(4 + 1, np.nan, np.float32), X.reshape(-1)])
    t = _dev(flat)
    assert t.data_ptr() % 16 == 0
    return X, t, t.data_ptr() + 4 * (4 + 1)


@gpu
@pytest.mark.parametrize("padded", [False, True], ids=["Kcp=Kc", "Kcp=Kc^4"])
@pytest.mark.parametrize("Kc", [1, 63, 64, 65, 127, 128])
@pytest.mark.parametrize("M", [1, 4, 5, 37])
def test_factor_u_is_bitwise_the_sequential_float64_sum(M, Kc, padded):
    """U[p, :Kc] of row perm[p] over its light items only, pad columns +0.0,
    ldu > Kcp and ldxl > Kc with everything around untouched, Xl's base 4 bytes
    off a 16-byte boundary, four rows per workgroup (M = 1, 4, 5, 37)."""
    rows, hub_index, perm = _u_graph(M)
    Kcp = (Kc + 3) // 4 * 4 if padded else Kc
    ldxl, ldu = Kc + 3, Kcp + 5
    X, xt, xptr = _x_sources(Kc, ldxl, hub_index, 7 * M + Kc)
    assert xptr % 16 == 4
    rp, ci, v = (_dev(a) for a in _csr(rows))
    hi, pm = _dev(hub_index), _dev(perm)
    U = Out(M * ldu, SENT_F)
    _lib.check(_lib.load().gcnk_factor_u_f32(rp.data_ptr(), ci.data_ptr(), v.data_ptr(), M, hi.data_ptr(),
                                             pm.data_ptr(), xptr, ldxl, Kc, U.ptr, ldu, Kcp, _stream()),
               "gcnk_factor_u_f32")
    torch.cuda.synchronize()
    got = U.get().reshape(M, ldu)
    want = _u_reference(rows, perm, hub_index, X, Kc, Kcp)
    assert np.array_equal(_bits(got[:, :Kcp]), _bits(want))
    assert (got[:, Kcp:] == SENT_F).all()


@gpu
@pytest.mark.parametrize("padded", [False, True], ids=["Kp=K", "Kp=K^4"])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 127, 128])
@pytest.mark.parametrize("M", [1, 4, 5, 37])
def test_aggregate_is_bitwise_the_sequential_float64_sum(M, K, padded):
    """gcnk_aggregate_f32: the same kernel with no hub index and no row order
    -- every item of every row, rows in order."""
    rows, _, _ = _u_graph(M)
    Kp = (K + 3) // 4 * 4 if padded else K
    ldx, ldo = K + 3, Kp + 5
    X, xt, xptr = _x_sources(K, ldx, None, 11 * M + K)
    rp, ci, v = (_dev(a) for a in _csr(rows))
    out = Out(M * ldo, SENT_F)
    _lib.check(_lib.load().gcnk_aggregate_f32(rp.data_ptr(), ci.data_ptr(), v.data_ptr(), M, xptr, ldx, K, out.ptr,
                                              ldo, Kp, _stream()), "gcnk_aggregate_f32")
    torch.cuda.synchronize()
    got = out.get().reshape(M, ldo)
    want = _u_reference(rows, np.arange(M), None, X, K, Kp)
    assert np.array_equal(_bits(got[:, :Kp]), _bits(want))
    assert (got[:, Kp:] == SENT_F).all()


# ------------------------------------------------------------------------------ gcnk_factor_analyze

HMIN = 3


def _pattern(rows):
    """rowptr, colind of a list of column lists."""
    rp, ci, _ = _csr([[(c, 1.0) for c in r] for r in rows])
    return rp, ci


def _doc_topic_rows(long_hub=False):
    """Documents [diagonal, one topic] (HMIN - 1 nonzeros: light), document 7 its diagonal alone; topics 8 and
    9 with four documents each, the other topic and themselves, topic 10 with exactly HMIN nonzeros.
    long_hub: 70 documents and one topic whose row has 71 items instead."""
    if long_hub:
        return [[d, 70] for d in range(70)] + [list(range(71))]
    rows = [[d, 8 + d % 2] for d in range(7)] + [[7]]
    rows += [[0, 2, 4, 6, 8, 9], [1, 3, 5, 8, 9], [0, 1, 10]]
    return rows


def _analyze_reference(rows, hmin, x_rows, K):
    """(hubs, bad, k0, k1, xtot, cnt) by the rules of include/gcnk.h.  x_rows: per row a list of (col, value),
    explicit zeros included; xtot counts stored entries of the hub rows."""
    M = len(rows)
    hubs = [r for r in range(M) if len(rows[r]) >= hmin]
    is_hub = np.zeros(M, bool)
    is_hub[hubs] = True
    bad = int(any(not is_hub[r] and not is_hub[c] and c != r for r in range(M) for c in rows[r]))
    cnt = np.array([sum(bool(is_hub[c]) for c in rows[r]) for r in range(M)], np.int32)
    cols = [c for r in range(M) if not is_hub[r] for c, v in x_rows[r] if v != 0]
    k0, k1 = (min(cols), max(cols)) if cols else (None, -1)
    xtot = sum(len(x_rows[r]) for r in hubs)
    return hubs, bad, k0, k1, xtot, cnt


def _analyze(rows, hmin, max_hubs, x_rows=None, K=0, dense_ldx=0):
    """One call; (info[8], the listed hubs, cnt[M]) with every host and device buffer's guards checked."""
    lib = _lib.load()
    M = len(rows)
    rp, ci = (_dev(a) for a in _pattern(rows))
    keep = [rp, ci]
    if dense_ldx:
        Xd = np.full((M, dense_ldx), np.nan, np.float32)
        Xd[:, :K] = 0.0
        for r, items in enumerate(x_rows):
            for c, v in items:
                Xd[r, c] = v
        xd = _dev(Xd)
        keep.append(xd)
        xa = (None, None, None, xd.data_ptr(), dense_ldx, K)
    else:
        xrp, xci, xv = (_dev(a) for a in _csr(x_rows))
        keep += [xrp, xci, xv]
        xa = (xrp.data_ptr(), xci.data_ptr(), xv.data_ptr(), None, 0, K)
    wsb = int(lib.gcnk_factor_analyze_workspace_bytes(M, max_hubs))
    assert wsb == 4 * (2 * M + 8 + max_hubs)
    ws = Out(wsb // 4, SENT_I)
    info = np.full(8 + 4, SENT_I, np.int32)
    hubs = np.full(max_hubs + 4, SENT_I, np.int32)
    cnt = np.full(M + 4, SENT_I, np.int32)
    _lib.check(lib.gcnk_factor_analyze(rp.data_ptr(), ci.data_ptr(), M, hmin, *xa, max_hubs, info.ctypes.data,
                                       hubs.ctypes.data, cnt.ctypes.data, ws.ptr, wsb, _stream()),
               "gcnk_factor_analyze")
    ws.get()
    assert (info[8:] == SENT_I).all() and (hubs[max_hubs:] == SENT_I).all() and (cnt[M:] == SENT_I).all()
    assert (info[5:8] == 0).all()
    return info[:8], hubs[:max_hubs], cnt[:M]


def _x_for(rows, hmin, K, lo, hi, zeros=False, empty_light=False):
    """X rows: light rows with entries in [lo, hi] (row 0 has lo, row 1 has hi), hub rows with all K columns;
    zeros: light rows also store 0.0 at columns 0 and K - 1."""
    rng = np.random.default_rng(K + lo)
    x = []
    for r, cols in enumerate(rows):
        if len(cols) >= hmin:
            x.append([(c, np.float32(rng.standard_normal())) for c in range(K)])
        elif empty_light:
            x.append([(0, np.float32(0.0))] if zeros and r % 2 else [])
        else:
            pick = {lo} if r == 0 else {hi} if r == 1 else set(rng.choice(np.arange(lo, hi + 1), 2).tolist())
            items = [(c, np.float32(rng.uniform(0.5, 1.5))) for c in sorted(pick)]
            if zeros:
                items = [(0, np.float32(0.0))] + items + [(K - 1, np.float32(0.0))]
            x.append(items)
    return x


def _check_analyze(rows, x_rows, K, got, max_hubs):
    info, listed, cnt = got
    hubs, bad, k0, k1, xtot, want_cnt = _analyze_reference(rows, HMIN, x_rows, K)
    assert info[0] == len(hubs) and info[1] == bad
    shown = listed[:min(len(hubs), max_hubs)].tolist()
    assert len(set(shown)) == len(shown) and set(shown) <= set(hubs)
    if len(hubs) <= max_hubs:
        assert sorted(shown) == hubs
    assert info[3] == k1
    if k1 >= 0:
        assert info[2] == k0
    assert np.array_equal(cnt, want_cnt)
    return hubs, k0, k1, xtot


@gpu
@pytest.mark.parametrize("x", ["csr", "csr_zeros", "dense"])
@pytest.mark.parametrize("graph", ["doc_topic", "long_hub"])
def test_analyze_clean_structure(graph, x):
    """Hub rows = rows of at least hmin nonzeros (exactly hmin is a hub,
    hmin - 1 is not; a hub row of 71 items); a light row with its diagonal
    alone is no violation; cnt[] for every row, hub rows included; X's
    light-row range from a CSR (explicit zeros and the hub rows' columns
    outside it do not move it; info[4] = stored length of X's hub rows) and
    from a dense X with ldx > K (NaN in the padding)."""
    rows = _doc_topic_rows(graph == "long_hub")
    K, lo, hi = 12, 4, 9
    x_rows = _x_for(rows, HMIN, K, lo, hi, zeros=x == "csr_zeros")
    got = _analyze(rows, HMIN, 8, x_rows, K, dense_ldx=K + 3 if x == "dense" else 0)
    hubs, k0, k1, xtot = _check_analyze(rows, x_rows, K, got, 8)
    assert hubs == ([70] if graph == "long_hub" else [8, 9, 10]) and (k0, k1) == (lo, hi) and got[0][1] == 0
    assert got[0][4] == (0 if x == "dense" else xtot) and xtot == K * len(hubs)


@gpu
def test_analyze_reports_a_light_row_that_touches_a_light_row():
    rows = _doc_topic_rows()
    rows[3] = [2, 3]            # document 3: its diagonal and document 2
    x_rows = _x_for(rows, HMIN, 12, 4, 9)
    got = _analyze(rows, HMIN, 8, x_rows, 12)
    _check_analyze(rows, x_rows, 12, got, 8)
    assert got[0][1] == 1


@gpu
@pytest.mark.parametrize("max_hubs", [3, 2])
def test_analyze_hub_list_full_and_one_too_short(max_hubs):
    """H = max_hubs: all listed; H = max_hubs + 1: info[0] is the true count
    and every listed entry is a distinct real hub (nothing past the list)."""
    rows = _doc_topic_rows()
    x_rows = _x_for(rows, HMIN, 12, 4, 9)
    got = _analyze(rows, HMIN, max_hubs, x_rows, 12)
    _check_analyze(rows, x_rows, 12, got, max_hubs)
    assert got[0][0] == 3


@gpu
@pytest.mark.parametrize("x", ["csr", "csr_zeros", "dense"])
def test_analyze_light_rows_without_features(x):
    """No nonzero entry in any light row (none stored, only explicit zeros, or
    a dense X of zeros there): k1 = -1."""
    rows = _doc_topic_rows()
    x_rows = _x_for(rows, HMIN, 12, 4, 9, zeros=x == "csr_zeros", empty_light=True)
    got = _analyze(rows, HMIN, 8, x_rows, 12, dense_ldx=16 if x == "dense" else 0)
    _check_analyze(rows, x_rows, 12, got, 8)
    assert got[0][3] == -1


# ------------------------------------------------------------------------------ gcnk_factor_xl_f32

@gpu
@pytest.mark.parametrize("k0,Kc,Kcp", [(0, 4, 4), (5, 4, 4), (5, 3, 4), (0, 6, 8), (5, 7, 8)])
def test_factor_xl(k0, Kc, Kcp):
    """Xl[r, c] = X[r, k0 + c] for light rows and c < Kc: entries below k0 and
    at or past k0 + Kc dropped, hub rows and pad columns zero, ldxl > Kcp with
    the floats between the rows untouched; M = 11 (three workgroups, the last
    ragged)."""
    rows = _doc_topic_rows()
    M, K = len(rows), 12
    x_rows = _x_for(rows, HMIN, K, 2, 10, zeros=True)
    hub_index = np.full(M, -1, np.int32)
    hub_index[[8, 9, 10]] = [0, 1, 2]
    ldxl = Kcp + 3
    xrp, xci, xv = (_dev(a) for a in _csr(x_rows))
    hi = _dev(hub_index)
    Xl = Out(M * ldxl, SENT_F)
    _lib.check(_lib.load().gcnk_factor_xl_f32(xrp.data_ptr(), xci.data_ptr(), xv.data_ptr(), M, hi.data_ptr(), k0, Kc,
                                              Xl.ptr, ldxl, Kcp, _stream()), "gcnk_factor_xl_f32")
    torch.cuda.synchronize()
    got = Xl.get().reshape(M, ldxl)
    want = np.zeros((M, Kcp), np.float32)
    dropped = kept = 0
    for r in range(M):
        for c, v in x_rows[r]:
            if hub_index[r] < 0 and k0 <= c < k0 + Kc:
                want[r, c - k0] = v
                kept += 1
            elif hub_index[r] < 0:
                dropped += 1
    assert kept and dropped
    assert np.array_equal(_bits(got[:, :Kcp]), _bits(want))
    assert (got[:, Kcp:] == SENT_F).all()


# ------------------------------------------------------------------------------ gcnk_factor_records

BLOCK = ROWS
REC_SRC = 200                 # sources (columns); hubs: d % 3 == 0 and the sources around the long row's 64th
BOUNDARY_HUBS = (72, 73, 74, 75, 136, 137, 138, 139)       # and 128th items (items 62 .. 65 and 126 .. 129)


@functools.lru_cache(maxsize=None)
def _records_problem(M, odd):
    """Rows by position of the block order.  M >= 33: position 33 (32 at M = 33) holds a row of 150 items
    (sources 10 .. 159) with hub items on both sides of its 64th and 128th items.  M = 70: the last block (positions 64 .. 69) has
    no hub item.  The fullest block holds an odd / even number of hub items, as asked."""
    rng = np.random.default_rng(M)
    hub_index = np.full(REC_SRC, -1, np.int32)
    hubs = sorted(set(np.flatnonzero(np.arange(REC_SRC) % 3 == 0).tolist()) | set(BOUNDARY_HUBS))
    hub_index[hubs] = np.arange(len(hubs))
    nblk = (M + BLOCK - 1) // BLOCK
    by_pos = []
    for p in range(M):
        if M >= 33 and p == min(33, M - 1):
            cols = np.arange(10, 160)
        elif M == 70 and p >= 64:
            cols = np.array([c for c in np.sort(rng.choice(190, size=6, replace=False)) if hub_index[c] < 0])
        else:
            cols = np.sort(rng.choice(190, size=(p + 2) % 9, replace=False))     # (position 7: no item)
        by_pos.append([(int(c), np.float32(rng.standard_normal())) for c in cols])
    count = lambda b: sum(hub_index[c] >= 0 for r in by_pos[b * BLOCK:(b + 1) * BLOCK] for c, _ in r)  # noqa: E731
    per_block = [count(b) for b in range(nblk)]
    full = int(np.argmax(per_block))
    if per_block[full] % 2 != int(odd):
        by_pos[full * BLOCK].append((198, np.float32(0.5)))     # source 198 is a hub, past every other column
        per_block[full] += 1
    # two items fewer still hold every other block's
    assert all(n <= per_block[full] - 2 for b, n in enumerate(per_block) if b != full)
    perm = rng.permutation(M).astype(np.int32)
    rows = [None] * M
    for p in range(M):
        rows[perm[p]] = by_pos[p]
    return rows, by_pos, hub_index, perm, per_block, full


def _records_reference(by_pos, hub_index, perm, M, rec_words):
    """The records (unused tail zero) and, per block, whether its items all fit in rec_words."""
    items = [[(hub_index[c], v) for c, v in row if hub_index[c] >= 0] for row in by_pos]
    rec = pack(items, perm, M, rec_words, 0)
    return rec, [2 * int(rec[b, BLOCK]) <= rec_words - REC_HEAD for b in range(len(rec))]


def test_records_problems_hold_what_the_tests_are_about():
    """The preconditions, on the arrays alone (no GPU)."""
    for M in (1, 32, 33, 70):
        for odd in (False, True):
            rows, by_pos, hub_index, perm, per_block, full = _records_problem(M, odd)
            assert len(rows) == M and per_block[full] % 2 == int(odd)
            assert all(c < REC_SRC for r in rows for c, _ in r)
            assert all([c for c, _ in r] == sorted({c for c, _ in r}) for r in rows)
            if M >= 33:
                long_row = by_pos[min(33, M - 1)]
                assert len(long_row) >= 150
                hub_at = {i for i, (c, _) in enumerate(long_row) if hub_index[c] >= 0}
                assert {62, 63, 64, 65, 126, 127, 128, 129} <= hub_at and len(hub_at) < len(long_row)
            if M == 70:
                assert per_block[2] == 0 and any(by_pos[p] for p in range(64, 70))
            if M > 1:
                assert not np.array_equal(perm, np.arange(M))


def _records(M, odd, short_words):
    rows, by_pos, hub_index, perm, per_block, full = _records_problem(M, odd)
    rec_words = (REC_HEAD + 2 * per_block[full] + 3) // 4 * 4 - short_words
    nblk = (M + BLOCK - 1) // BLOCK
    rp, ci, v = (_dev(a) for a in _csr(rows))
    hi, pm = _dev(hub_index), _dev(perm)
    rec = Out(nblk * rec_words, SENT_I)
    over = Out(1, SENT_I)
    _lib.check(_lib.load().gcnk_factor_records(rp.data_ptr(), ci.data_ptr(), v.data_ptr(), M, hi.data_ptr(),
                                               pm.data_ptr(), rec.ptr, rec_words, over.ptr, _stream()),
               "gcnk_factor_records")
    torch.cuda.synchronize()
    want, fits = _records_reference(by_pos, hub_index, perm, M, rec_words)
    return rec.get().reshape(nblk, rec_words), int(over.get()[0]), want, fits, per_block, full, rec_words


@gpu
@pytest.mark.parametrize("M", [1, 32, 33, 70])
def test_factor_records_exactly_sufficient(M):
    """Offsets, row ids (-1 past M), every row's hub items in CSR order (a row
    of 150 items with hub items on both sides of its 64th and 128th, a block
    with no hub item), the unused tail zero; rec_words = 68 + 2 x the fullest
    block's items leaves no spare word there: *overflow == 0."""
    got, over, want, fits, per_block, full, rec_words = _records(M, False, 0)
    assert rec_words == REC_HEAD + 2 * per_block[full] and all(fits)
    if M == 70:
        assert per_block[2] == 0 and per_block[1] > 64
    assert np.array_equal(got, want)
    assert over == 0


@gpu
@pytest.mark.parametrize("M,short", [(33, 1), (70, 1), (70, 2), (1, 1)])
def test_factor_records_items_short_in_one_block(M, short):
    """rec_words one item (and two items) short for the fullest block alone:
    *overflow == 1 -- it counts blocks, not items --, that block holds its
    first items and nothing at or past its rec_words, the neighbouring records
    are whole."""
    # (rec_words is a multiple of 4: one item short of an odd count, two of an even one)
    got, over, want, fits, per_block, full, rec_words = _records(M, short == 1, 4)
    assert rec_words == REC_HEAD + 2 * (per_block[full] - short) and rec_words >= REC_HEAD
    assert [not f for f in fits] == [b == full for b in range(len(fits))]
    assert np.array_equal(got, want)
    assert over == 1


# ------------------------------------------------------------------------------ gcnk_factor_diag_f32

@gpu
@pytest.mark.parametrize("M", [1, 32, 37])
def test_factor_diag(M):
    """diag[p], pre[p] of row perm[p]: a missing diagonal gives 0, a hub row
    (0, -1), positions past M (0, 0); hub columns below and above the diagonal
    (only those below count)."""
    rng = np.random.default_rng(40 + M)
    hub_index = np.full(M, -1, np.int32)
    hubs = np.flatnonzero(np.arange(M) % 6 == 1) if M > 1 else np.array([], np.int64)
    hub_index[hubs] = np.arange(len(hubs))
    rows = []
    for r in range(M):
        cols = set(rng.choice(hubs, size=min(len(hubs), r % 5), replace=False).tolist()) if len(hubs) else set()
        if r % 4 != 3:
            cols.add(r)                                          # (every fourth row has no diagonal)
        rows.append([(int(c), np.float32(rng.standard_normal())) for c in sorted(cols)])
    perm = rng.permutation(M).astype(np.int32)
    npos = (M + BLOCK - 1) // BLOCK * BLOCK
    rp, ci, v = (_dev(a) for a in _csr(rows))
    hi, pm = _dev(hub_index), _dev(perm)
    diag, pre = Out(npos, SENT_F), Out(npos, SENT_I)
    _lib.check(_lib.load().gcnk_factor_diag_f32(rp.data_ptr(), ci.data_ptr(), v.data_ptr(), M, hi.data_ptr(),
                                                pm.data_ptr(), diag.ptr, pre.ptr, _stream()), "gcnk_factor_diag_f32")
    torch.cuda.synchronize()
    wd, wp = np.zeros(npos, np.float32), np.zeros(npos, np.int32)
    for p in range(M):
        r = perm[p]
        if hub_index[r] >= 0:
            wp[p] = -1
            continue
        for c, val in rows[r]:
            if c == r:
                wd[p] = val
            elif c < r and hub_index[c] >= 0:
                wp[p] += 1
    if M == 37:
        light = [r for r in range(M) if hub_index[r] < 0]
        assert any(any(c < r for c, _ in rows[r]) and any(c > r for c, _ in rows[r]) for r in light)
        assert any(all(c != r for c, _ in rows[r]) for r in light) and (wp == -1).any()
    assert np.array_equal(_bits(diag.get()), _bits(wd))
    assert np.array_equal(pre.get(), wp)


# ------------------------------------------------------------------------------ the row gathers

def _gather_source():
    """Six rows: 3 items, none, 300, 1, none, 7."""
    rng = np.random.default_rng(9)
    rows = []
    for n in (3, 0, 300, 1, 0, 7):
        cols = np.sort(rng.choice(400, size=n, replace=False))
        rows.append([(int(c), np.float32(rng.standard_normal())) for c in cols])
    return rows


@gpu
@pytest.mark.parametrize("sel", [[2], [1], [5, 1, 2, 4, 0], [4, 1]], ids=["long", "empty", "out_of_order", "all_empty"])
def test_csr_gather_rows(sel):
    """Selected rows in the order given (one row; empty rows; a row of 300
    entries, more than a workgroup's 256 threads), out_rowptr[nrows] included,
    nothing written past the gathered entries."""
    rows = _gather_source()
    rp, ci, v = (_dev(a) for a in _csr(rows))
    total = sum(len(rows[r]) for r in sel)
    rs = _dev(np.array(sel, np.int32))
    orp, oci, ov = Out(len(sel) + 1, SENT_I), Out(total + 8, SENT_I), Out(total + 8, SENT_F)
    _lib.check(_lib.load().gcnk_csr_gather_rows(rp.data_ptr(), ci.data_ptr(), v.data_ptr(), rs.data_ptr(), len(sel),
                                                orp.ptr, oci.ptr, ov.ptr, _stream()), "gcnk_csr_gather_rows")
    torch.cuda.synchronize()
    wrp, wci, wv = _csr([rows[r] for r in sel])
    assert np.array_equal(orp.get(), wrp)
    gci, gv = oci.get(), ov.get()
    assert np.array_equal(gci[:total], wci) and np.array_equal(_bits(gv[:total]), _bits(wv))
    assert (gci[total:] == SENT_I).all() and (gv[total:] == SENT_F).all()


@gpu
@pytest.mark.parametrize("K,ldo", [(5, 5), (5, 12), (300, 300), (300, 308)])
@pytest.mark.parametrize("sel", [[3], [4, 0, 2]], ids=["one", "out_of_order"])
def test_dense_gather_rows(sel, K, ldo):
    """Rows of a dense X with ldx > K (NaN in its padding) in the order given,
    columns K .. ldo - 1 zero; K past a workgroup's 256 threads."""
    rng = np.random.default_rng(K)
    ldx = K + 3
    X = np.full((6, ldx), np.nan, np.float32)
    X[:, :K] = rng.standard_normal((6, K)).astype(np.float32)
    xd, rs = _dev(X), _dev(np.array(sel, np.int32))
    out = Out(len(sel) * ldo, SENT_F)
    _lib.check(_lib.load().gcnk_dense_gather_rows_f32(xd.data_ptr(), ldx, K, rs.data_ptr(), len(sel), out.ptr, ldo,
                                                      _stream()), "gcnk_dense_gather_rows_f32")
    torch.cuda.synchronize()
    want = np.zeros((len(sel), ldo), np.float32)
    want[:, :K] = X[sel, :K]
    assert np.array_equal(_bits(out.get().reshape(len(sel), ldo)), _bits(want))


# ------------------------------------------------------------------------------ bad arguments (no GPU)

P_ = ctypes.c_void_p(16)


def _refused(fn, good, nulls, bads):
    lib = _lib.load()
    f = getattr(lib, fn)
    for i in nulls:
        args = list(good)
        assert args[i] is P_ or isinstance(args[i], int) and args[i] > 4096, (fn, i)
        args[i] = None
        assert f(*args) == _lib.EARG, (fn, i)
        assert fn.encode() in lib.gcnk_last_error()
    for i, bad in bads:
        args = list(good)
        args[i] = bad
        assert f(*args) == _lib.EARG, (fn, i, bad)


def test_build_entries_refuse_bad_arguments():
    """No GPU needed: a null for each pointer, Kcp > 128, Kcp < Kc, leading
    dimensions below the width, rec_words below 68 or no multiple of 4 and an
    analyze workspace one byte short are refused before anything is read."""
    p = P_
    host = np.zeros(64, np.int32)
    hp = int(host.ctypes.data)
    # rowptr, colind, val, M, hub_index, perm, Xl, ldxl, Kc, U, ldu, Kcp, stream
    _refused("gcnk_factor_u_f32", [p, p, p, 10, p, p, p, 8, 6, p, 8, 8, None], (0, 1, 2, 4, 5, 6, 9),
             ((3, 0), (8, 0), (11, 5), (11, 132), (10, 7), (7, 5)))
    assert _lib.load().gcnk_factor_u_f32(p, p, p, 10, p, p, p, 200, 128, p, 200, 129, None) == _lib.EARG
    # rowptr, colind, val, M, X, ldx, K, out, ldo, Kp, stream
    _refused("gcnk_aggregate_f32", [p, p, p, 10, p, 8, 6, p, 8, 8, None], (0, 1, 2, 4, 7),
             ((3, 0), (6, 0), (9, 5), (9, 132), (8, 7), (5, 5)))
    # rowptr, colind, val, M, hub_index, perm, rec, rec_words, overflow, stream
    _refused("gcnk_factor_records", [p, p, p, 10, p, p, p, 72, p, None], (0, 1, 2, 4, 5, 6, 8),
             ((3, 0), (7, 64), (7, 67), (7, 70), (7, 0)))
    # rowptr, colind, M, hmin, x_rowptr, x_colind, x_val, x_dense, ldx, K, max_hubs, info, hubs, cnt, ws, bytes, stream
    need = int(_lib.load().gcnk_factor_analyze_workspace_bytes(10, 4))
    assert need == 4 * (2 * 10 + 8 + 4)
    csr_x = [p, p, 10, 3, p, p, p, None, 0, 12, 4, hp, hp, hp, p, need, None]
    _refused("gcnk_factor_analyze", csr_x, (0, 1, 4, 5, 6, 11, 12, 13, 14), ((2, 0), (3, 0), (10, 0), (15, need - 1)))
    dense_x = [p, p, 10, 3, None, None, None, p, 12, 12, 4, hp, hp, hp, p, need, None]
    _refused("gcnk_factor_analyze", dense_x, (7,), ((8, 11), (9, 0), (15, need - 1)))
    assert _lib.load().gcnk_factor_analyze_workspace_bytes(-1, 4) == _lib.EARG
    # x_rowptr, x_colind, x_val, M, hub_index, k0, Kc, Xl, ldxl, Kcp, stream
    _refused("gcnk_factor_xl_f32", [p, p, p, 10, p, 0, 6, p, 8, 8, None], (0, 1, 2, 4, 7),
             ((3, 0), (5, -1), (6, 0), (9, 5), (8, 7)))
    # rowptr, colind, val, M, hub_index, perm, diag, pre, stream
    _refused("gcnk_factor_diag_f32", [p, p, p, 10, p, p, p, p, None], (0, 1, 2, 4, 5, 6, 7), ((3, 0),))
    # rowptr, colind, val, rows, nrows, out_rowptr, out_colind, out_val, stream
    _refused("gcnk_csr_gather_rows", [p, p, p, p, 2, p, p, p, None], (0, 1, 2, 3, 5, 6, 7), ((4, 0),))
    # X, ldx, K, rows, nrows, out, ldo, stream
    _refused("gcnk_dense_gather_rows_f32", [p, 8, 6, p, 2, p, 8, None], (0, 3, 5), ((4, 0), (2, 0), (1, 5), (6, 5)))
