"""Float64 restatements (numpy) of the two contracts in include/gcnk.h that
train.py sits on: the mean cross-entropy over a node set (gcnk_ce_*) and the
Adam step (gcnk_adam_f32).  tests/test_train_ref.py holds them to torch in
float64; the GPU tests hold the kernels to them."""
import numpy as np


def counts_of(idx, M):
    """Row multiplicities of an index set over M rows (gcnk_ce_row_counts): int64 [M + 1],
    the last entry counting the entries outside [0, M)."""
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < M)
    c = np.zeros(M + 1, dtype=np.int64)
    np.add.at(c, np.where(ok, idx, M), 1)
    return c


def ce_forward(z, t, counts=None, n=None):
    """(lse [M], row loss [M], loss): lse_r = max + log sum exp(z - max), l_r = lse_r -
    z[r, t_r] (NaN for a target outside [0, P)), loss = sum counts[r] l_r / n over the rows
    with counts[r] > 0 (every row once, n = M, when counts is None)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64)
    M, P = z.shape
    mx = z.max(axis=1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
    ok = (t >= 0) & (t < P)
    zt = np.where(ok, z[np.arange(M), np.where(ok, t, 0)], np.nan)
    row = lse - zt
    c = np.ones(M, dtype=np.int64) if counts is None else np.asarray(counts)[:M]
    n = M if n is None else n
    scored = c > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64((c[scored] * row[scored]).sum()) / n
    return lse, row, loss


def ce_backward(z, t, counts=None, n=None, g=1.0):
    """dlogits [M x P] = g * counts[r] / n * (softmax(z_r) - onehot(t_r)); rows with
    counts[r] == 0 are zero."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64)
    M, P = z.shape
    lse, _, _ = ce_forward(z, t, counts, n)
    c = np.ones(M, dtype=np.int64) if counts is None else np.asarray(counts)[:M]
    n = M if n is None else n
    d = np.exp(z - lse[:, None])
    ok = (t >= 0) & (t < P)
    d[np.arange(M)[ok], t[ok]] -= 1.0
    d *= (g * c / n)[:, None]
    d[c == 0] = 0.0
    return d


def adam_step(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """Step number t (>= 1) of torch's Adam (amsgrad=False, maximize=False) in float64:
    (p', m', v')."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    g = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps
    return p - (lr / (1.0 - beta1 ** t)) * m / denom, m, v


def ulp32(x):
    """The spacing of fp32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)
