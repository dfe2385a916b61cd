"""What the LDA GPU tests (test_topic_infer.py, test_topic_fit.py, test_topic_fit_online.py) share: uploads,
bit views, the table as the kernels read it, and the fit's three launches by their entry points alone, on a case
of lda_fit_cases.py / lda_online_cases.py, with guard entries around what a launch may write."""
import numpy as np
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, topic_fit

DEV = "cuda:0"
GUARD = -1.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def table(beta):
    """exp(E[log beta]) [K x V] as the kernels read it: transposed, rows padded to an even length."""
    K, V = beta.shape
    t = torch.zeros((V, (K + 1) // 2 * 2), dtype=torch.float64, device=DEV)
    t[:, :K] = dev(beta).t()
    return t


def _stream():
    return _lib.stream(torch.device(DEV))


def estep_fit(c, indptr=None, indices=None, counts=None, gamma0=None):
    """gcnk_lda_estep_fit_f64 alone on case c (or on the batch given) -> gamma, etheta, ratio, iters."""
    indptr = c["indptr"] if indptr is None else indptr
    indices = c["indices"] if indices is None else indices
    counts = c["counts"] if counts is None else counts
    gamma0 = c["gamma0"] if gamma0 is None else gamma0
    B, K, V, nnz = len(indptr) - 1, c["K"], c["V"], len(indices)
    tb = table(c["beta"])
    ip, g0 = dev(indptr), dev(gamma0)
    ix = dev(indices) if nnz else torch.zeros(1, dtype=torch.int32, device=DEV)
    ct = dev(counts) if nnz else torch.zeros(1, dtype=torch.float64, device=DEV)
    gamma = torch.full((B, K), GUARD, dtype=torch.float64, device=DEV)
    etheta = torch.full((B, K), GUARD, dtype=torch.float64, device=DEV)
    ratio = torch.full((max(nnz, 1) + 2,), GUARD, dtype=torch.float64, device=DEV)   # (two guard entries)
    iters = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    rc = _lib.load().gcnk_lda_estep_fit_f64(ip.data_ptr(), ix.data_ptr(), ct.data_ptr(), 0, B, V, K, tb.data_ptr(),
                                            tb.stride(0), c["alpha"], c["tol"], c["max_iter"], g0.data_ptr(), K, nnz,
                                            ratio.data_ptr(), etheta.data_ptr(), K, gamma.data_ptr(), K,
                                            iters.data_ptr(), _stream())
    _lib.check(rc, "gcnk_lda_estep_fit_f64")
    assert float(ratio[nnz:].max()) == GUARD == float(ratio[nnz:].min())   # nothing stored past the nnz ratios
    return gamma, etheta, ratio[:nnz], iters


def _mstep_operands(c):
    """-> the word-major index, table, etheta and ratio of an M-step case on the device (one-element stand-ins
    where the corpus holds no word: the entry points still want addresses)."""
    nnz = len(c["indices"])
    ix = topic_fit.word_index(dev(c["indptr"]), dev(c["indices"]), c["V"])
    if nnz == 0:
        ix.pos = ix.doc = torch.zeros(1, dtype=torch.int32, device=DEV)
    ratio = dev(c["ratio"]) if nnz else torch.zeros(1, dtype=torch.float64, device=DEV)
    return ix, table(c["beta"]), dev(c["etheta"]), ratio


def mstep(c):
    """gcnk_lda_mstep_f64 alone on case c -> lambda [K x V], the word-major index."""
    B, K, V, nnz = c["B"], c["K"], c["V"], len(c["indices"])
    ix, tb, etheta, ratio = _mstep_operands(c)
    lam = torch.full((K, V), GUARD, dtype=torch.float64, device=DEV)
    rc = _lib.load().gcnk_lda_mstep_f64(ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), nnz, ratio.data_ptr(),
                                        etheta.data_ptr(), K, B, V, K, tb.data_ptr(), tb.stride(0), c["eta"],
                                        lam.data_ptr(), V, _stream())
    _lib.check(rc, "gcnk_lda_mstep_f64")
    return lam, ix


def mstep_online(c):
    """gcnk_lda_mstep_online_f64 alone on case c -> lambda [K x (V + pad)], the guard columns included."""
    B, K, V, nnz = c["B"], c["K"], c["V"], len(c["indices"])
    ix, tb, etheta, ratio = _mstep_operands(c)
    lam = torch.full((K, V + c["pad"]), GUARD, dtype=torch.float64, device=DEV)
    lam[:, :V] = dev(c["lam"])
    rc = _lib.load().gcnk_lda_mstep_online_f64(
        ix.wptr.data_ptr(), ix.pos.data_ptr(), ix.doc.data_ptr(), nnz, c["doc_lo"], c["doc_hi"], ratio.data_ptr(),
        etheta.data_ptr(), K, B, V, K, tb.data_ptr(), tb.stride(0), c["eta"], c["rho"], c["doc_ratio"],
        lam.data_ptr(), lam.stride(0), _stream())
    _lib.check(rc, "gcnk_lda_mstep_online_f64")
    return lam
