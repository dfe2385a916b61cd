"""Float64 numpy restatement of held-graph scoring (include/gcnk.h,
gcnk_score_docs_f32) and the pieces the tests share: the held state of a
graph from the math, the edge weights recovered from A-hat, the label rule."""
import numpy as np


def coefficients(a, dh):
    """(c_self [B], c [B x H]) as fp32 values: float64 throughout, rounded once."""
    a = np.asarray(a, np.float32).astype(np.float64)
    s = np.zeros(a.shape[0])
    for j in range(a.shape[1]):          # j ascending
        s = s + a[:, j]
    dd = np.power(1.0 + s, -0.5)
    c_self = (dd * dd).astype(np.float32)
    c = ((dd[:, None] * a) * np.asarray(dh, np.float64)[None, :]).astype(np.float32)
    return c_self, c


def score(x, a, W1, S_T, W2, S2_T, dh, b1=None, b2=None, k0=0):
    """out [B x P] in float64 from fp32 operands (the coefficients rounded to fp32 as the definition says)."""
    x = np.asarray(x, np.float64)
    Kc = x.shape[1]
    c_self, c = coefficients(a, dh)
    cs, c = c_self.astype(np.float64)[:, None], c.astype(np.float64)
    W1, S_T, W2, S2_T = (np.asarray(t, np.float64) for t in (W1, S_T, W2, S2_T))
    z = cs * (x @ W1[k0:k0 + Kc]) + c @ S_T
    if b1 is not None:
        z = z + np.asarray(b1, np.float64)
    h = np.maximum(z, 0.0)               # (np.maximum keeps a NaN, as th.relu does)
    out = cs * (h @ W2) + c @ S2_T
    if b2 is not None:
        out = out + np.asarray(b2, np.float64)
    return out


def labels(out):
    """First index of the maximum, a NaN maximal (csrc/metrics.hip class_stats)."""
    out = np.asarray(out)
    nan = np.isnan(out)
    lab = np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, out).argmax(1))
    return lab.astype(np.int64)


def top2_gap(out):
    """Per row: the float64 gap between the two largest logits (inf for P = 1 and for NaN rows: decided)."""
    out = np.asarray(out, np.float64)
    if out.shape[1] < 2:
        return np.full(out.shape[0], np.inf)
    s = np.sort(out, axis=1)
    g = s[:, -1] - s[:, -2]
    return np.where(np.isnan(g), np.inf, g)


def recovered_edges(A, docs, hubs):
    """a [len(docs) x H] fp32 from A-hat (scipy CSR, float64 values of its fp32
    entries): a = A-hat[d, hub_j] / (sqrt(A-hat[d, d]) dh_j), and dh [H]."""
    hubs = np.asarray(hubs)
    diag = A.diagonal()
    dh = np.sqrt(diag[hubs])
    sub = np.asarray(A[docs][:, hubs].todense(), np.float64)
    a = sub / (np.sqrt(diag[docs])[:, None] * dh[None, :])
    return a.astype(np.float32), dh


def held_state(A, X, hubs, W1, b1, W2):
    """(S_T [H x F], S2_T [H x P]) in float64 from the eval forward's first layer on the training graph."""
    W1, W2 = np.asarray(W1, np.float64), np.asarray(W2, np.float64)
    S1 = X @ W1
    Z = A @ S1
    if b1 is not None:
        Z = Z + np.asarray(b1, np.float64)
    S2 = np.maximum(Z, 0.0) @ W2
    hubs = np.asarray(hubs)
    return np.asarray(S1[hubs]), np.asarray(S2[hubs])


def reference_init(seed, nfeat, nhid, nclass):
    """(W1, b1, W2, b2) as the reference initialises them after th.manual_seed(seed)
    (layer.py:75-82: gc1.weight, gc1.bias, gc2.weight, gc2.bias, U(-1/sqrt(out), 1/sqrt(out)))."""
    import math
    import torch
    torch.manual_seed(seed)
    out = []
    for fin, fout in ((nfeat, nhid), (nhid, nclass)):
        bound = 1.0 / math.sqrt(fout)
        out.append(torch.empty(fin, fout, dtype=torch.float32).uniform_(-bound, bound).numpy())
        out.append(torch.empty(fout, dtype=torch.float32).uniform_(-bound, bound).numpy())
    return tuple(out)


# ------------------------------------------------------------------ the kernel tests' cases (tests/test_score_docs.py)
# (B, Kc, H, F, P, k0): one document; a partial, a full and a just-over block; several blocks with Kc + H past one
# k-chunk multiple and two n-tiles of P; the largest shape ([W1[Kc]; S_T], 256 KB, staged in three chunks of 96, 96
# and 64 rows); nothing a multiple of anything, k0 > 0; more blocks than one residency round at a block per CU; then
# three shapes whose MFMA k-loop runs up to 3 operand columns past the hub sum's Kc + 16 KHQ (Kc + H rounded up to 4
# reaches past it: H = 63 / 127 / 64 with Kc % 4 != 0) -- the reference's Kc = H = ntopic layout at 63 and 127 topics
SHAPES = [(1, 3, 2, 4, 1, 0), (31, 50, 50, 200, 8, 0), (32, 50, 50, 200, 8, 0), (33, 50, 50, 200, 8, 0),
          (97, 70, 70, 200, 20, 0), (40, 128, 128, 256, 32, 0), (65, 37, 41, 36, 3, 5), (2100, 50, 50, 200, 8, 0),
          (40, 63, 63, 200, 8, 0), (33, 127, 127, 256, 8, 0), (45, 50, 64, 200, 8, 0)]
# per shape, a seed for which the float64 reference alone leaves at most 1 % of the rows within 2 atol of a tie
# (checked on the CPU: tests/test_score_docs_abi.py)
SEEDS = {s: 1 for s in SHAPES}


def atol_of(ref):
    """test_factored_gc1_kernel_against_float64's tolerance for this chain."""
    return 2e-5 * max(1.0, float(np.abs(ref).max()))


def make_case(shape, seed=None):
    """fp32 operands of one shape: documents with LDA-like sparse edge weights and
    L2-normalised features; row 0 without an edge, row 1 with all H edges, row 2
    with x = 0 (where B has them)."""
    B, Kc, H, F, P, k0 = shape
    rng = np.random.default_rng(SEEDS[shape] if seed is None else seed)
    f32 = lambda v: np.ascontiguousarray(v, np.float32)
    theta = rng.dirichlet(np.full(H, 2.0 / H), size=B)
    a = np.where(theta >= 0.02, theta, 0.0)
    a[0] = 0.0
    if B > 1:
        a[1] = theta[1] + 0.02
    x = rng.random((B, Kc)) * (rng.random((B, Kc)) < 0.4)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    if B > 2:
        x[2] = 0.0
    return {
        "shape": shape, "x": f32(x), "a": f32(a),
        "W1": f32(rng.standard_normal((k0 + Kc + 2, F))), "S_T": f32(rng.standard_normal((H, F))),
        "W2": f32(rng.standard_normal((F, P)) / np.sqrt(F)), "S2_T": f32(rng.standard_normal((H, P))),
        "dh": rng.uniform(0.03, 0.6, H), "b1": f32(rng.standard_normal(F)), "b2": f32(rng.standard_normal(P)),
    }


def case_ref(c, b1=True, b2=True):
    return score(c["x"], c["a"], c["W1"], c["S_T"], c["W2"], c["S2_T"], c["dh"], c["b1"] if b1 else None,
                 c["b2"] if b2 else None, k0=c["shape"][5])
