"""The device dropout mask (dropout_rng="device", GCNK_EPI_BIAS_RELU_HASH)
held to its contract in every kernel that draws it.

The contract (include/gcnk.h): element (r, c) is kept iff
hash(seed, *rng_base + offset + r*ldm + c) < keep_prob.  oracle/hash_ref.py
restates it in numpy (pinned on the CPU by tests/test_hash_ref.py); here every
application site -- the row kernel's light rows and heavy-row combines, the
top-entry launch, the tile epilogue, the slab reduce, the two-part launch, the
fused projection, gcnk_hubfactor_gc1_f32 and gcnk_dense_gc1_f32 -- and the GCN
module's wiring of seed / base / advance are compared with it element by
element, with no tolerance on the mask and no element excluded.

The common device: the pre-activation acc is computed in float64 and the bias
is c + randn(F) with c large enough that acc + bias >= 1 at EVERY element
(c = 1 + ceil(max|acc| + max|randn|)), so relu never clips, "output != 0" is
the kept bit of every element, and the values are (acc + bias) * scale where
kept.  Value tolerances are those of the same kernel's float64 test in
tests/test_gpu_parity.py, times the dropout scale.
"""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, _lib, datasets, from_arrays, ops
from graph_convolutional_networks_for_text_classification_amd.ops import _ptr, _stream
from graph_convolutional_networks_for_text_classification_amd.sparse import DENSE_THRESHOLD, as_csr
from oracle import csr_ref, hash_ref

from test_gpu_parity import _close, _grads_close, _mixed_density_csr, _random_csr

pytestmark = pytest.mark.gpu
DEV = "cuda"
HASH = _lib.EPI_BIAS_RELU_HASH
SCALE = 2.0


# ------------------------------------------------------------------------------ the common device

def _bias_clear_of_relu(acc, rng):
    """bias = c + randn(F) with acc + bias >= 1 everywhere (float32, as the kernels read it)."""
    noise = rng.standard_normal(acc.shape[1])
    c = 1.0 + np.ceil(np.abs(acc).max() + np.abs(noise).max())
    bias = (c + noise).astype(np.float32)
    pre = acc + bias.astype(np.float64)
    assert pre.min() >= 1.0
    return bias, pre


def _arg_sets(M, F):
    """The argument sets S0-S4 (keep_prob 0.5): name, seed, offset, *rng_base
    (None: a null pointer), ldm (0: the kernels' default, F)."""
    half = M * F // 2
    if F >= 4 and (half % F) % 4 == 0:
        half += 2          # 2^32 falls inside an aligned group of 4 columns, not on its edge
    if F >= 4:
        assert (half % F) % 4 != 0 and half < M * F
    return [
        ("S0 plain", 123, 0, None, 0),
        ("S1 across 2^32", 0xDEADBEEF12345678, 2**32 - half, None, 0),
        ("S2 across 2^64", 5, 2**64 - M * F // 3, None, 0),
        ("S3 device base", 123, 17, 3 * M * F + 1, 0),
        ("S4 explicit ldm", 123, 0, None, F + 12),
    ]


def _assert_mask(name, H, want):
    got = H != 0
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} of {want.size} elements kept/dropped against the contract, "
                             f"first (r, c): {[tuple(int(v) for v in b) for b in bad[:6]]}")


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _check_kernel(run, pre, h_atol, W2=None, s2_atol=None, unstored=False, sets=None):
    """Every argument set through ``run(seed, offset, base, ldm, keep, store)``
    -> (H, S2) (torch tensors; S2 None for a kernel without the projection; H
    None when not stored): (a) the mask, (b) the values, (c) the not-stored
    variant.  ``base`` is a one-element int64 device tensor or None.  h_atol /
    s2_atol already hold the factor SCALE."""
    M, F = pre.shape
    W2d = None if W2 is None else np.asarray(W2, np.float64)

    def check(name, seed, offset, base, ldm, keep, mask):
        bt = None if base is None else torch.tensor([base], dtype=torch.int64, device=DEV)
        H, S2 = run(seed, offset, bt, ldm, keep, True)
        Hn = _np(H)
        assert np.isfinite(Hn).all(), name
        _assert_mask(name, Hn, mask)                                            # (a)
        want = np.where(mask, pre * SCALE, 0.0)
        _close(Hn.astype(np.float64), want, rtol=1e-5, atol=h_atol)             # (b)
        if W2d is not None:
            assert bool(torch.isfinite(S2).all()), name
            _close(S2, want @ W2d, rtol=1e-5, atol=s2_atol)
            if unstored:                                                        # (c)
                Hu, S2u = run(seed, offset, bt, ldm, keep, False)
                assert Hu is None and torch.equal(S2u, S2), name
        if bt is not None:
            assert int(bt.item()) == base, "the kernel only reads *rng_base"
        return H, S2

    for name, seed, offset, base, ldm in (_arg_sets(M, F) if sets is None else sets):
        mask = hash_ref.keep_mask(seed, base or 0, offset, M, F, ldm or F, 0.5)
        H, S2 = check(name, seed, offset, base, ldm, 0.5, mask)
        if base is not None:   # the same call with the base folded into offset and a null pointer: same bits
            Hf, S2f = run(seed, (offset + base) % 2**64, None, ldm, 0.5, True)
            assert torch.equal(Hf, H), name
            assert S2 is None or torch.equal(S2f, S2), name
    # S5: keep_prob 1 (all kept), 0 (none kept, nothing non-finite), 0.9 (rate)
    for keep in (1.0, 0.0, 0.9):
        mask = hash_ref.keep_mask(123, 0, 0, M, F, F, keep)
        H, S2 = check(f"S5 keep {keep}", 123, 0, None, 0, keep, mask)
        kept = _np(H) != 0
        if keep == 1.0:
            assert kept.all()
        elif keep == 0.0:
            assert not kept.any() and (S2 is None or not bool(S2.any()))
        else:
            z = (kept.sum() - kept.size * keep) / np.sqrt(kept.size * keep * (1 - keep))
            assert abs(z) <= 4, z


# ------------------------------------------------------------------------------ the SpMM entry points, raw

def _spmm_raw(a, B, bias, seed, offset, base, ldm, keep, ldc=None, ipc=None, lanes=0, dense=None, parts=False,
              W=None, store_main=True):
    """gcnk_spmm_csr_f32 / _part (parts 1 then 2) / gcnk_spmm_proj_f32 (W given)
    with the hash epilogue and every argument explicit, as ops.spmm /
    ops.spmm_proj marshal them.  Returns (rc, the whole C buffer [M x ldc]
    pre-filled with 7 -- None when not stored --, C2, the plan)."""
    lib = _lib.load()
    M, K = a.shape
    F = B.shape[1]
    if W is not None and not lanes:
        lanes = 64
    if ipc is None:
        ipc = ops.default_ipc(a, F, lanes)
    groups = int(lib.gcnk_spmm_groups(F, int(lanes)))
    plan = a.plan(ipc, groups, DENSE_THRESHOLD if dense is None else dense)
    wsb = plan.workspace_bytes(F)
    ws = torch.empty((wsb + 3) // 4, dtype=torch.float32, device=B.device) if wsb > 0 else None
    cnt = plan.counters(B.device)
    ldc = F if ldc is None else ldc
    buf = torch.full((M, ldc), 7.0, device=B.device) if store_main else None
    head = (_ptr(plan.buf), ctypes.cast(plan.hdr, ctypes.c_void_p), _ptr(B), B.stride(0), F, _ptr(buf), ldc,
            _ptr(bias), HASH, None, int(ldm), SCALE, float(keep), int(seed), int(offset), _ptr(base))
    tail = (_ptr(ws), wsb, _ptr(cnt), 4 * cnt.numel() if cnt is not None else 0, int(lanes))
    st = _stream(B.device)
    C2 = None
    if W is not None:
        P = W.shape[1]
        C2 = torch.full((M, P), float("nan"), device=B.device)
        rc = lib.gcnk_spmm_proj_f32(*head, _ptr(W), W.stride(0), P, _ptr(C2), P, *tail, st)
    elif parts:
        rc = lib.gcnk_spmm_csr_f32_part(*head, *tail, 1, st) or lib.gcnk_spmm_csr_f32_part(*head, *tail, 2, st)
    else:
        rc = lib.gcnk_spmm_csr_f32(*head, *tail, st)
    return rc, buf, C2, plan


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def light_heavy():
    """700 x 500, light rows and one heavy row (400 + nonzeros, one combine)."""
    rng = np.random.default_rng(11)
    rp, ci, v = _random_csr(700, 500, 5000, rng, heavy_rows=(1,), heavy_deg=400)
    return rp, ci, v, from_arrays(rp, ci, v, (700, 500), DEV)


@pytest.mark.parametrize("F", [1, 7, 64, 200])
def test_row_kernel_light_and_heavy_rows(light_heavy, F):
    """spmm_row_kernel's finish_row (scalar columns F = 1, 7 -- a column tail --
    and float4 columns 64, 200) on light rows and a heavy row of one combine,
    into a view of a wider buffer (ldc = 2F) whose padding stays untouched; the
    op wrapper gives the same bits."""
    rp, ci, v, a = light_heavy
    M, K = a.shape
    rng = np.random.default_rng(100 + F)
    B = rng.standard_normal((K, F)).astype(np.float32)
    bias, pre = _bias_clear_of_relu(csr_ref.spmm_csr(rp, ci, v, B), rng)
    Bt, bt = _t(B), _t(bias)
    deg = int(np.diff(rp).max())

    def run(seed, offset, base, ldm, keep, store):
        rc, buf, _, plan = _spmm_raw(a, Bt, bt, seed, offset, base, ldm, keep, ldc=2 * F, dense=2.0)
        _lib.check(rc, "gcnk_spmm_csr_f32")
        assert plan.ntile == 0 and plan.nunits > 0 and plan.nhunits > 0, "row kernel only: light units and heavy segments"
        assert bool((buf[:, F:] == 7.0).all()), "columns past F of the output buffer are not the kernel's"
        return buf[:, :F], None
    _check_kernel(run, pre, h_atol=2e-5 * np.sqrt(deg) * SCALE)
    got = ops.spmm(a, Bt, bias=bt, epilogue=HASH, scale=SCALE, keep_prob=0.5, seed=0xDEADBEEF12345678,
                   offset=2**32 - 77, dense=2.0)
    rc, buf, _, _ = _spmm_raw(a, Bt, bt, 0xDEADBEEF12345678, 2**32 - 77, None, 0, 0.5, dense=2.0)
    assert rc == 0 and torch.equal(got, buf)


@pytest.mark.parametrize("F,ipc,lanes", [(64, 4, 64), (8, 4, 0)])
def test_heavy_row_combines_and_top_entry(F, ipc, lanes):
    """The last-arriver combine (spmm_row_kernel) and spmm_heavy_top_kernel:
    rows of 1,023 ... 2,049 and 70,000 nonzeros (more than 64 segments: groups
    under a top entry), an empty row (output = mask ? bias * scale : 0), rows of
    1 and 5."""
    rng = np.random.default_rng(F + ipc)
    K = 80_000
    degs = [1023, 1024, 1025, 2047, 2049, 70_000, 0, 5, 1, 300]
    rows, cols = [], []
    for r, d in enumerate(degs):
        span = K // 8 if r < 5 else K
        c = np.sort(rng.choice(span, d, replace=False)) if d else np.zeros(0, np.int64)
        rows.append(np.full(d, r))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    rp, ci, v = csr_ref.coo_to_csr(rows, cols, rng.standard_normal(rows.size), (len(degs), K))
    a = from_arrays(rp, ci, v, (len(degs), K), DEV)
    B = rng.standard_normal((K, F)).astype(np.float32)
    acc = csr_ref.spmm_csr(rp, ci, v, B)
    assert not acc[6].any()
    bias, pre = _bias_clear_of_relu(acc, rng)
    Bt, bt = _t(B), _t(bias)

    def run(seed, offset, base, ldm, keep, store):
        rc, buf, _, plan = _spmm_raw(a, Bt, bt, seed, offset, base, ldm, keep, ipc=ipc, lanes=lanes)
        _lib.check(rc, "gcnk_spmm_csr_f32")
        assert plan.nheavy >= 6 and plan.has_tops, "multi-segment heavy rows and a top entry expected"
        return buf, None
    _check_kernel(run, pre, h_atol=2e-5 * np.sqrt(70_000) * SCALE)


@pytest.mark.parametrize("F", [7, 64, 200])
@pytest.mark.parametrize("M", [700, 900])
def test_tile_epilogue_slab_reduce_and_two_part_launch(F, M):
    """spmm_tile_kernel's epilogue (single-chunk blocks) and
    spmm_tile_reduce_kernel (multi-chunk blocks) beside the row kernel, on a
    square operand (diagonal kept aside) and a rectangular one; the two-part
    launch (gcnk_spmm_csr_f32_part 1 then 2) gives the one-launch bits."""
    rng = np.random.default_rng(F + 1)
    K = 900
    rp, ci, v = _mixed_density_csr(rng, M, K)
    a = from_arrays(rp, ci, v, (M, K), DEV)
    B = rng.standard_normal((K, F)).astype(np.float32)
    bias, pre = _bias_clear_of_relu(csr_ref.spmm_csr(rp, ci, v, B), rng)
    Bt, bt = _t(B), _t(bias)

    def run(seed, offset, base, ldm, keep, store):
        rc, buf, _, plan = _spmm_raw(a, Bt, bt, seed, offset, base, ldm, keep)
        _lib.check(rc, "gcnk_spmm_csr_f32")
        assert plan.ntile > 0 and plan.nred > 0, "dense blocks (single and multi-chunk) expected on the tile path"
        assert plan.has_diag == (M == K)
        assert plan.nsingle > 0 and plan.ntile > plan.nsingle, "both single- and multi-chunk tile blocks expected"
        rc2, two, _, _ = _spmm_raw(a, Bt, bt, seed, offset, base, ldm, keep, parts=True)
        _lib.check(rc2, "gcnk_spmm_csr_f32_part")
        assert torch.equal(two, buf), "two-part launch"
        return buf, None
    _check_kernel(run, pre, h_atol=2e-5 * np.sqrt(K) * SCALE)


@pytest.mark.parametrize("P", [1, 8, 33])
def test_fused_projection(light_heavy, P):
    """gcnk_spmm_proj_f32 (the row kernel's finish_row with the projection; H
    stored or not) at P = 1, 8; P = 33 is outside it (GCNK_EUNSUP) and
    ops.spmm_proj's unfused fallback draws the same mask.  S2's bound: the
    existing fused-projection test's 2e-4 (H of magnitude ~1 there) times
    max|H_ref| here."""
    rp, ci, v, a = light_heavy
    M, K = a.shape
    F = 200
    rng = np.random.default_rng(300 + P)
    B = rng.standard_normal((K, F)).astype(np.float32)
    W2 = rng.standard_normal((F, P)).astype(np.float32)
    bias, pre = _bias_clear_of_relu(csr_ref.spmm_csr(rp, ci, v, B), rng)
    Bt, bt, Wt = _t(B), _t(bias), _t(W2)
    s2_atol = 2e-4 * max(1.0, SCALE * pre.max())
    if P <= 32:
        def run(seed, offset, base, ldm, keep, store):
            rc, buf, C2, plan = _spmm_raw(a, Bt, bt, seed, offset, base, ldm, keep, W=Wt, store_main=store)
            _lib.check(rc, "gcnk_spmm_proj_f32")       # (GCNK_EUNSUP would mean the fused kernel did not run)
            assert plan.ntile == 0
            return buf, C2
        _check_kernel(run, pre, h_atol=2e-5 * SCALE, W2=W2, s2_atol=s2_atol, unstored=True)
        H, S2 = ops.spmm_proj(a, Bt, Wt, bias=bt, epilogue=HASH, scale=SCALE, keep_prob=0.5, seed=5,
                              offset=2**64 - 1000)
        rc, buf, C2, _ = _spmm_raw(a, Bt, bt, 5, 2**64 - 1000, None, 0, 0.5, W=Wt)
        assert rc == 0 and torch.equal(H, buf) and torch.equal(S2, C2)
        return
    rc, _, _, _ = _spmm_raw(a, Bt, bt, 123, 0, None, 0, 0.5, W=Wt)
    assert rc == _lib.EUNSUP

    def run(seed, offset, base, ldm, keep, store):
        return ops.spmm_proj(a, Bt, Wt, bias=bt, epilogue=HASH, scale=SCALE, keep_prob=keep, seed=seed,
                             offset=offset, rng_base=base, store_main=store)
    # (the wrapper has no ldm argument: S4 is the row kernel's, above)
    _check_kernel(run, pre, h_atol=2e-5 * SCALE, W2=W2, s2_atol=s2_atol, unstored=True,
                  sets=_arg_sets(M, F)[:4])


@pytest.fixture(scope="module")
def doc_topic():
    """doc_topic_graph(2000, 40, 5, seed=4, tt_prob=0.3): its factor (hub rows
    moved by the block order) and the float64 A-hat, X."""
    import scipy.sparse as ssp
    from graph_convolutional_networks_for_text_classification_amd import factor
    g = datasets.doc_topic_graph(2000, 40, 5, seed=4, tt_prob=0.3)
    A, X = g["adj"].to(DEV), g["features"].to(DEV)
    f = factor.get(as_csr(A), ops.Operand(X))
    assert f is not None
    assert not np.array_equal(f.perm.numpy(), np.arange(f.M))   # a site hashing the block position would differ
    a = g["adj"].coalesce()
    Ad = ssp.csr_matrix((a.values().double().numpy(), a.indices().numpy()), shape=tuple(a.shape))
    return g, f, Ad, g["features_dense"].astype(np.float64)


@pytest.mark.parametrize("F,P", [(52, 3), (200, 20)])
def test_hubfactor_gc1(doc_topic, F, P):
    """gcnk_hubfactor_gc1_f32: rows written through the block order's row ids
    (Vec<4>::epi on 4-column groups), H1 stored or not; each launch follows an
    LDS poison launch."""
    g, f, Ad, Xd = doc_topic
    rng = np.random.default_rng(3 + F)
    W1 = rng.standard_normal((g["nfeat"], F)).astype(np.float32)
    W2 = rng.standard_normal((F, P)).astype(np.float32)
    bias, pre = _bias_clear_of_relu(Ad @ (Xd @ W1.astype(np.float64)), rng)
    W1t, W2t, bt = _t(W1), _t(W2), _t(bias)
    S_T = f.hub_times(W1t).contiguous()
    lib = _lib.load()

    def run(seed, offset, base, ldm, keep, store):
        st = _stream(bt.device)
        H1 = torch.full((f.M, F), float("nan"), device=DEV) if store else None
        S2 = torch.full((f.M, P), float("nan"), device=DEV)
        _lib.check(lib.gcnk_debug_poison_lds(0xFFFFFFFF, st), "gcnk_debug_poison_lds")
        _lib.check(lib.gcnk_hubfactor_gc1_f32(
            f.M, F, f.Kc, f.H, P, _ptr(f.U), f.U.stride(0), _ptr(W1t), F, f.k0, _ptr(S_T), F, _ptr(f.rec),
            f.rec_words, _ptr(bt), HASH, None, int(ldm), SCALE, float(keep), int(seed), int(offset), _ptr(base),
            _ptr(W2t), P, _ptr(H1), F, _ptr(S2), P, st), "gcnk_hubfactor_gc1_f32")
        return H1, S2
    tol = 2e-5 * max(1.0, pre.max()) * SCALE
    _check_kernel(run, pre, h_atol=tol, W2=W2, s2_atol=tol * max(1.0, np.abs(W2).sum(0).max()), unstored=True)
    H1, S2 = run(5, 2**64 - 1000, None, 0, 0.5, True)
    Hw, Sw = ops.hubfactor_gc1(f, W1t, bt, W2t, epilogue=HASH, scale=SCALE, keep_prob=0.5, seed=5,
                               offset=2**64 - 1000, S=S_T)
    assert torch.equal(Hw, H1) and torch.equal(Sw, S2)


@pytest.mark.parametrize("K,F,P,M", [(7, 8, 3, 1000), (97, 196, 19, 300), (100, 240, 20, 600), (13, 200, 1, 16)])
def test_dense_gc1(K, F, P, M):
    """gcnk_dense_gc1_f32: the main n-tiles and the rotating tail n-tile (F =
    196, 200), four n-tiles (240), a partial last 16-row tile (M = 1000, 300,
    600; M = 16 is one whole tile); H1 stored or not."""
    rng = np.random.default_rng(K * 1000 + F + P)
    AX = rng.standard_normal((M, (K + 3) // 4 * 4)).astype(np.float32)
    AX[:, K:] = 0.0
    W1 = rng.standard_normal((K, F)).astype(np.float32)
    W2 = rng.standard_normal((F, P)).astype(np.float32)
    bias, pre = _bias_clear_of_relu(csr_ref.gemm(AX[:, :K], W1), rng)
    AXt, W1t, W2t, bt = _t(AX), _t(W1), _t(W2), _t(bias)
    lib = _lib.load()

    def run(seed, offset, base, ldm, keep, store):
        H1 = torch.full((M, F), float("nan"), device=DEV) if store else None
        S2 = torch.full((M, P), float("nan"), device=DEV)
        _lib.check(lib.gcnk_dense_gc1_f32(M, K, F, P, _ptr(AXt), AXt.stride(0), _ptr(W1t), F, _ptr(bt), HASH, None,
                                          int(ldm), SCALE, float(keep), int(seed), int(offset), _ptr(base),
                                          _ptr(W2t), P, _ptr(H1), F, _ptr(S2), P, _stream(bt.device)),
                   "gcnk_dense_gc1_f32")
        return H1, S2
    tol = 2e-5 * max(1.0, pre.max()) * SCALE
    _check_kernel(run, pre, h_atol=tol, W2=W2, s2_atol=tol * max(1.0, np.abs(W2).sum(0).max()), unstored=True)


# ------------------------------------------------------------------------------ the module's wiring

NHID = 200
MODEL_SEED = 2**40 + 3        # seed_hi != 0


@pytest.fixture(scope="module")
def wiring():
    """The doc-topic graph with a sparse X (600 columns, 8 % full: the CSR
    paths) and the gensim-shaped dense X (100 columns: the dense paths), the
    float64 A-hat, a fixed random R for the loss (logits * R).sum(), and a
    cache of the float64 step-independent terms per X."""
    import scipy.sparse as ssp
    gs = datasets.doc_topic_graph(2000, 40, 5, seed=4, tt_prob=0.3, emb_dim=600)
    gd = datasets.doc_topic_graph(2000, 40, 5, seed=4, tt_prob=0.3)
    a = gs["adj"].coalesce()
    assert torch.equal(a.indices(), gd["adj"].coalesce().indices())
    Ad = ssp.csr_matrix((a.values().double().numpy(), a.indices().numpy()), shape=tuple(a.shape))
    R = np.random.default_rng(8).standard_normal((gs["nodes"], gs["nclass"])).astype(np.float32)
    return {"sparse": gs, "dense": gd, "Ad": Ad, "R": R, "A": gs["adj"].to(DEV), "ref": {}}


def _reference(w, kind, params):
    """Step-independent float64 terms of the forward / backward for X of `kind`."""
    hit = w["ref"].get(kind)
    if hit is None:
        Ad, R = w["Ad"], w["R"].astype(np.float64)
        Xd = w[kind]["features_dense"].astype(np.float64)
        W1, b1, W2, b2 = (params[k].astype(np.float64) for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias"))
        AX = Ad @ Xd
        gS2 = Ad.T @ R
        hit = w["ref"][kind] = {"AX": AX, "Z1b": AX @ W1 + b1, "gS2": gS2, "gH1": gS2 @ W2.T, "W2": W2, "b2": b2,
                                "gb2": R.sum(0)}
    return hit


def _step_reference(w, ref, mask, scale):
    """float64 logits and gradients of one train-mode step under keep-mask `mask`."""
    H1 = np.where(mask, ref["Z1b"] * scale, 0.0)
    logits = w["Ad"] @ (H1 @ ref["W2"]) + ref["b2"]
    gZ1 = np.where(mask, scale * ref["gH1"], 0.0)
    grads = {"gc1.weight": ref["AX"].T @ gZ1, "gc1.bias": gZ1.sum(0), "gc2.weight": H1.T @ ref["gS2"],
             "gc2.bias": ref["gb2"]}
    return logits, grads


def _step_close(logits, grads, want_logits, want_grads):
    tol = 1e-5 * max(1.0, float(np.abs(want_logits).max()))
    err = float(np.abs(logits - want_logits).max())
    assert err <= tol, f"logits: max err {err:.3e} > {tol:.3e}"
    for k, g in want_grads.items():
        _grads_close(grads[k].astype(np.float64), g, k, rtol=1e-4, kink_frac=0)


@pytest.mark.parametrize("path", ["factored", "spmm_proj", "spmm_gemm", "dense_factored", "dense_spmm", "dense_ax"])
def test_gcn_wires_seed_base_and_advance(wiring, path, monkeypatch):
    """GCN(dropout_rng="device") on each forward path: step t of a seeded model
    (torch.manual_seed(2^40 + 3): seed_hi != 0) draws keep_mask(seed, t*M*nhid,
    0, M, nhid, nhid, 0.5) in the forward AND masks the backward with it --
    logits and all four gradients against float64 under that mask, and NOT
    under the mask of step t +- 1 (the bounds discriminate); _rng_base advances
    by M*nhid per training forward and an eval forward leaves it alone."""
    from graph_convolutional_networks_for_text_classification_amd import record
    monkeypatch.setattr(ops, "FACTOR_GC1", path in ("factored", "dense_factored"))
    monkeypatch.setattr(ops, "FUSE_PROJECTION", path != "spmm_gemm")
    monkeypatch.setattr(ops, "DENSE_AX", path == "dense_ax")
    kind = "dense" if path.startswith("dense") else "sparse"
    g, A = wiring[kind], wiring["A"]
    X = g["features"].to(DEV)
    assert (ops.Operand(X).dense is not None) == (kind == "dense")
    M, P = g["nodes"], g["nclass"]
    torch.manual_seed(MODEL_SEED)
    m = GCN(nfeat=g["nfeat"], nhid=NHID, nclass=P, dropout=0.5, dropout_rng="device")
    # gc1's bias clear of the ReLU: Z1 + b1 >= 1 everywhere, so no element sits at a kink
    Z1 = wiring["Ad"] @ (g["features_dense"].astype(np.float64) @ m.gc1.weight.detach().double().numpy())
    noise = np.random.default_rng(2).standard_normal(NHID)
    c = 1.0 + np.ceil(np.abs(Z1).max() + np.abs(noise).max())
    with torch.no_grad():
        m.gc1.bias.copy_(torch.from_numpy((c + noise).astype(np.float32)))
    params = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    ref = _reference(wiring, kind, params)
    assert ref["Z1b"].min() >= 1.0
    m = m.to(DEV).train()
    seed = int(torch.initial_seed())
    assert seed == MODEL_SEED
    Rt = torch.from_numpy(wiring["R"]).to(DEV)
    scale = float(torch.ones((), dtype=torch.float32).div_(0.5))
    masks = [hash_ref.keep_mask(seed, t * M * NHID, 0, M, NHID, NHID, 0.5) for t in range(4)]
    for t in range(3):
        m.zero_grad(set_to_none=True)
        lg = m(X, A)
        (lg * Rt).sum().backward()
        assert int(m._rng_base.item()) == (t + 1) * M * NHID
        logits = lg.detach().cpu().numpy().astype(np.float64)
        grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
        _step_close(logits, grads, *_step_reference(wiring, ref, masks[t], scale))
        for other in (t - 1, t + 1):
            if other >= 0:
                with pytest.raises(AssertionError):
                    _step_close(logits, grads, *_step_reference(wiring, ref, masks[other], scale))
        if t == 1:   # an eval forward in between: no draw, no advance, the unmasked forward
            m.eval()
            with torch.no_grad():
                ev = m(X, A).cpu().numpy().astype(np.float64)
            m.train()
            assert int(m._rng_base.item()) == (t + 1) * M * NHID
            want = wiring["Ad"] @ (ref["Z1b"] @ ref["W2"]) + ref["b2"]
            assert np.abs(ev - want).max() <= 1e-5 * max(1.0, float(np.abs(want).max()))
    recs = [c.rec for c in getattr(as_csr(A), "_records", {}).values()]
    kinds = {r.kind for r in recs if isinstance(r, record.ForwardRecord)}
    assert any(isinstance(r, record.BackwardRecord) for r in recs)
    want_kind = {"factored": record.FACTORED, "dense_factored": record.FACTORED, "spmm_proj": record.SPMM_PROJ,
                 "spmm_gemm": record.SPMM_GEMM, "dense_ax": record.DENSE_AX}.get(path)
    if want_kind is not None:
        assert want_kind in kinds, kinds
