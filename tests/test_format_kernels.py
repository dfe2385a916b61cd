"""The sparse-format and metrics kernels at their edge shapes, on the GPU.

tests/format_cases.py is the case table with its plain references; tests/test_format_cases.py
checks both on the CPU.  Here every case runs through the public entry -- sparse.from_torch
(gcnk_coo_to_csr), sparse.transpose (gcnk_csr_transpose), sparse.preprocess_adj
(gcnk_sym_normalize), metrics.class_stats (gcnk_class_stats) and, for gcnk_csr_to_dense, the C
ABI -- and every comparison is exact: integer arrays element for element, fp32 arrays by their
bits.  The one exception is the payload of the NaNs a negative row sum gives (their positions
are compared).

Wall time of the module on an MI355X: 2.9 s (75 tests, none above 0.4 s).  No case failed on the
library as it was.  What the cases catch, each run once as an in-bounds one-line change of the
kernel (profiles/r41_format_mutations.log): a key cut to 32 bits (wide); a run summed backwards
(one_run, runs); one radix bit too few in bits_for64 (wide, pow2 and most others) and in bits_for
(pow2-K1025); a poison flag not reset (every case after the first); gather_kernel's search wrong
on equal row pointers (empties, edges, pow2); repeated columns on to_dense's store path, or its
order check short of a row's 64th pair (lengths); the diagonal after the first larger column, or d
from an fp32 pow (weighted, n257, zero_sum, neg_sum); the argmax over ld columns, rows nclass
apart, FN for an out-of-range target, a target cut to 32 bits, the last maximum or a NaN that
never wins (the class_stats sizes with more than one row).  Not caught: the identity's 1 added
last to the float64 row sum, which is exact in any order at fp32 weights of like magnitude.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import format_cases as fc  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib, metrics, sparse  # noqa: E402
from graph_convolutional_networks_for_text_classification_amd.ops import _ptr, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7FC12345   # a bit pattern no kernel here computes (a NaN with a payload)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ints(t):
    return t.cpu().numpy().astype(np.int64)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _sentinel(n, dtype=torch.float32):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(dtype)


def _coo_tensor(c):
    idx = _dev(np.vstack([c["rows"], c["cols"]]), torch.int64)
    return torch.sparse_coo_tensor(idx, _dev(c["vals"], torch.float32), c["shape"])


def _assert_csr(a, rp, ci, v, what):
    assert np.array_equal(_ints(a.rowptr), rp), what + ": rowptr"
    assert np.array_equal(_ints(a.colind), ci), what + ": colind"
    assert np.array_equal(_bits(a.val), _bits(v)), what + ": val bits"


# ------------------------------------------------------------------------------ COO -> CSR

@pytest.mark.parametrize("name", list(fc.coo_cases()))
def test_coo_to_csr(name):
    c = fc.coo_cases()[name]
    a = sparse.from_torch(_coo_tensor(c))
    rp, ci, v = fc.coo_to_csr_f32(c["rows"], c["cols"], c["vals"], c["shape"])
    assert a.shape == c["shape"] and a.nnz == len(ci)
    _assert_csr(a, rp, ci, v, name)


@pytest.mark.parametrize("name", ["wide", "pow2-256x256", "pow2-1x65537", "empty_rows"])
def test_coo_to_csr_ignores_the_order_of_distinct_entries(name):
    c = fc.coo_cases()[name]
    _, first = np.unique(c["rows"] * c["shape"][1] + c["cols"], return_index=True)
    first = np.sort(first)   # the duplicate-free COO, in its input order
    perm = np.random.default_rng(7).permutation(len(first))
    one = dict(c, rows=c["rows"][first], cols=c["cols"][first], vals=c["vals"][first])
    two = dict(c, rows=one["rows"][perm], cols=one["cols"][perm], vals=one["vals"][perm])
    a, b = sparse.from_torch(_coo_tensor(one)), sparse.from_torch(_coo_tensor(two))
    assert a.nnz == len(first)
    _assert_csr(b, _ints(a.rowptr), _ints(a.colind), a.val, name)


@pytest.mark.parametrize("which", list(fc.BAD_ENTRIES))
def test_coo_to_csr_refuses_an_index_outside_the_shape(which):
    """One bad entry among valid ones poisons the result; the flag is reset: a valid conversion right
    after it, on the same stream, is correct."""
    with pytest.raises(RuntimeError, match="outside its shape"):
        sparse.from_torch(_coo_tensor(fc.coo_bad_case(which)))
    c = fc.coo_valid_case()
    a = sparse.from_torch(_coo_tensor(c))
    _assert_csr(a, *fc.coo_to_csr_f32(c["rows"], c["cols"], c["vals"], c["shape"]), "after " + which)


# ------------------------------------------------------------------------------ transpose

def _device_csr(c):
    return sparse.from_arrays(c["rowptr"], c["colind"], c["val"], c["shape"], DEV)


@pytest.mark.parametrize("name", list(fc.transpose_cases()))
def test_csr_transpose(name):
    c = fc.transpose_cases()[name]
    M, K = c["shape"]
    a = _device_csr(c)
    t = sparse.transpose(a)
    rp, ci, v = fc.csr_transpose(c["rowptr"], c["colind"], c["val"], c["shape"])
    assert t.shape == (K, M) and len(rp) == K + 1
    _assert_csr(t, rp, ci, v, name)
    if c["canonical"]:
        _assert_csr(sparse.transpose(t), c["rowptr"], c["colind"], c["val"], name + ": transposed twice")


# ------------------------------------------------------------------------------ normalise

def _device_d(a):
    """d = rowsum(A + I)^-0.5 as gcnk_sym_normalize computed it (the head of its workspace), for a failure's report."""
    lib = _lib.load()
    n = a.shape[0]
    rp = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    ci = torch.empty(a.nnz + n, dtype=torch.int32, device=DEV)
    v = torch.empty(a.nnz + n, dtype=torch.float32, device=DEV)
    wsb = int(lib.gcnk_sym_normalize_workspace_bytes(n, a.nnz))
    ws = torch.zeros((wsb + 7) // 8, dtype=torch.float64, device=DEV)
    _lib.check(lib.gcnk_sym_normalize(_ptr(a.rowptr), _ptr(a.colind), _ptr(a.val), n, a.nnz, _ptr(rp), _ptr(ci),
                                      _ptr(v), _ptr(ws), wsb, _stream(a.device)), "gcnk_sym_normalize")
    return ws[:n].cpu().numpy()


@pytest.mark.parametrize("name", list(fc.normalize_cases()))
def test_sym_normalize(name):
    c = fc.normalize_cases()[name]
    n = c["n"]
    A = _coo_tensor(dict(c, shape=(n, n)))
    a = sparse.preprocess_adj(A)
    rp, ci, v, rowsum, d = fc.sym_normalize_detail(c["rows"], c["cols"], c["vals"], n)
    assert a.shape == (n, n)
    assert np.array_equal(_ints(a.rowptr), rp), name + ": rowptr"
    assert np.array_equal(_ints(a.colind), ci), name + ": colind"
    got = a.val.cpu().numpy()
    nan = np.isnan(v)
    assert np.array_equal(np.isnan(got), nan), name + ": where the NaNs are"
    assert nan.any() == (name == "neg_sum")
    diff = np.flatnonzero((_bits(got) != _bits(v)) & ~nan)
    if diff.size:   # report the row, the row sum and both d (the device's double pow against the host's)
        rows = np.repeat(np.arange(n), np.diff(rp))
        dd = _device_d(sparse.from_torch(A))
        lines = [f"({rows[k]}, {ci[k]}): got {got[k]!r} want {v[k]!r}; rowsum {rowsum[rows[k]]!r}, "
                 f"d host {d[rows[k]]!r} device {dd[rows[k]]!r}; column's d host {d[ci[k]]!r} device {dd[ci[k]]!r}"
                 for k in diff[:10]]
        pytest.fail(f"{name}: {diff.size} of {len(v)} values differ in bits\n" + "\n".join(lines))


# ------------------------------------------------------------------------------ CSR -> dense

def _to_dense(c, out, M=None):
    M = c["shape"][0] if M is None else M
    t = [_dev(c["rowptr"], torch.int32), _dev(c["colind"], torch.int32), _dev(c["val"], torch.float32)]
    rc = _lib.load().gcnk_csr_to_dense(_ptr(t[0]), _ptr(t[1]), _ptr(t[2]), M, c["shape"][1], _ptr(out), c["ld"],
                                       _stream(out.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", list(fc.dense_cases()))
def test_csr_to_dense(name):
    """Every [r, :K] is overwritten with the row's sums in CSR order, every [r, K:ld] left as it was."""
    c = fc.dense_cases()[name]
    M, K = c["shape"]
    out = _sentinel(M * c["ld"] + 5)
    assert _to_dense(c, out) == _lib.OK
    got = out.view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.all(got[M * c["ld"]:] == SENTINEL), "written past the last row"
    got = got[:M * c["ld"]].reshape(M, c["ld"])
    assert np.all(got[:, K:] == SENTINEL), "columns past K written"
    want = _bits(fc.csr_to_dense_f32(c["rowptr"], c["colind"], c["val"], M, K))
    bad = np.argwhere(got[:, :K] != want)
    assert not len(bad), f"{name}: {len(bad)} elements differ, the first at {bad[0]}"


def test_csr_to_dense_of_no_rows_is_a_no_op():
    c = fc.dense_cases()["mixed"]
    out = _sentinel(2 * c["ld"])
    assert _to_dense(c, out, M=0) == _lib.OK
    assert np.all(out.view(torch.int32).cpu().numpy() == SENTINEL)
    assert _lib.load().gcnk_csr_to_dense(None, None, None, 0, 7, None, 7, None) == _lib.OK


# ------------------------------------------------------------------------------ class_stats

@pytest.mark.parametrize("nclass,n", fc.CLASS_SIZES)
def test_class_stats(nclass, n):
    """Every row set, on the logits as a view of the wider tensor (ld = nclass + 5, NaN and +inf in the padding:
    passed without a copy) and as a contiguous copy; then out= on a longer buffer of garbage."""
    c = fc.class_case(nclass, n)
    wide = _dev(c["wide"], torch.float32)
    view = wide[:, :nclass]
    assert view.stride(1) == 1 and view.stride(0) == c["ld"] and view.data_ptr() == wide.data_ptr()
    targ = _dev(c["targets"], torch.int64)
    for layout, pred in (("ld = nclass + 5", view), ("contiguous", view.contiguous())):
        for kind, idx in c["idx"].items():
            want = fc.class_want(nclass, n, kind)
            got = _ints(metrics.class_stats(pred, targ, None if idx is None else _dev(idx, torch.int64)))
            what = f"nclass {nclass}, n {n}, {layout}, idx {kind}"
            scored = n if idx is None else len(idx)
            assert got.shape == (3 * nclass + 1,), what
            assert got[:nclass].sum() == got[-1] and got[:2 * nclass].sum() == scored, what + ": invariants"
            assert np.array_equal(got, want), what
    words = 3 * nclass + 1
    buf = _sentinel(words + 7, torch.int32)
    assert metrics.class_stats(view, targ, out=buf) is buf
    assert np.array_equal(_ints(buf[:words]), fc.class_want(nclass, n, "none")), "out=: the head is reset and filled"
    assert np.all(_ints(buf[words:]) == SENTINEL), "out=: the tail is untouched"


def test_class_stats_refusals_launch_nothing():
    lib = _lib.load()
    counts = _sentinel(3 * 1025 + 1, torch.int32)
    x = torch.zeros(4, 1030, device=DEV)
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    assert lib.gcnk_class_stats(_ptr(x), 1030, _ptr(t), None, 4, 1025, _ptr(counts), _stream(x.device)) == _lib.EARG
    assert lib.gcnk_class_stats(_ptr(x), 7, _ptr(t), None, 4, 8, _ptr(counts), _stream(x.device)) == _lib.EARG
    assert b"gcnk_class_stats" in lib.gcnk_last_error()
    with pytest.raises(_lib.GcnkError):
        metrics.class_stats(x[:, :1025], t)
    torch.cuda.synchronize()
    assert np.all(_ints(counts) == SENTINEL)
    assert lib.gcnk_class_stats(_ptr(x), 1030, _ptr(t), None, 4, 1024, _ptr(counts), _stream(x.device)) == _lib.OK
    assert _ints(counts[:3 * 1024 + 1]).sum() == 2 * 4   # four rows of zeros against target 0: TP 4, correct 4


# ------------------------------------------------------------------------------ workspace refusals

def test_a_workspace_one_byte_short_is_refused_before_any_launch():
    """gcnk_coo_to_csr, gcnk_csr_transpose and gcnk_sym_normalize: GCNK_EARG, the outputs untouched; with the
    whole workspace the same call succeeds."""
    lib = _lib.load()
    c = fc.coo_valid_case()
    M, K = c["shape"]
    nnz = len(c["vals"])
    rows, cols, vals = _dev(c["rows"], torch.int64), _dev(c["cols"], torch.int64), _dev(c["vals"], torch.float32)
    s = _stream(rows.device)

    def outputs(n_rows, n_ent):
        return _sentinel(n_rows + 1, torch.int32), _sentinel(n_ent, torch.int32), _sentinel(n_ent)

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(np.all(t.view(torch.int32).cpu().numpy() == SENTINEL) for t in ts)

    need = int(lib.gcnk_coo_to_csr_workspace_bytes(nnz, M, K))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rp, ci, v = outputs(M, nnz)
    args = (_ptr(rows), _ptr(cols), _ptr(vals), nnz, M, K, _ptr(rp), _ptr(ci), _ptr(v), _ptr(ws))
    assert need > 0 and lib.gcnk_coo_to_csr(*args, need - 1, s) == _lib.EARG
    assert b"workspace" in lib.gcnk_last_error() and untouched(rp, ci, v)
    assert lib.gcnk_coo_to_csr(*args, need, s) == _lib.OK
    want = fc.coo_to_csr_f32(c["rows"], c["cols"], c["vals"], c["shape"])
    u = int(want[0][-1])
    a = sparse.CSR(rp, ci[:u], v[:u], (M, K))
    _assert_csr(a, *want, "coo_to_csr with the whole workspace")

    need = int(lib.gcnk_csr_transpose_workspace_bytes(M, K, a.nnz))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rpt, cit, vt = outputs(K, a.nnz)
    args = (_ptr(a.rowptr), _ptr(a.colind), _ptr(a.val), M, K, a.nnz, _ptr(rpt), _ptr(cit), _ptr(vt), _ptr(ws))
    assert need > 0 and lib.gcnk_csr_transpose(*args, need - 1, s) == _lib.EARG
    assert b"workspace" in lib.gcnk_last_error() and untouched(rpt, cit, vt)
    assert lib.gcnk_csr_transpose(*args, need, s) == _lib.OK
    _assert_csr(sparse.CSR(rpt, cit, vt, (K, M)), *fc.csr_transpose(*want, (M, K)), "transpose with the whole workspace")

    g = fc.normalize_cases()["n257"]
    n = g["n"]
    adj = sparse.from_torch(_coo_tensor(dict(g, shape=(n, n))))
    need = int(lib.gcnk_sym_normalize_workspace_bytes(n, adj.nnz))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rpn, cin, vn = outputs(n, adj.nnz + n)
    args = (_ptr(adj.rowptr), _ptr(adj.colind), _ptr(adj.val), n, adj.nnz, _ptr(rpn), _ptr(cin), _ptr(vn), _ptr(ws))
    assert need > 0 and lib.gcnk_sym_normalize(*args, need - 1, s) == _lib.EARG
    assert b"workspace" in lib.gcnk_last_error() and untouched(rpn, cin, vn)
    assert lib.gcnk_sym_normalize(*args, need, s) == _lib.OK
    want = fc.sym_normalize_f64(g["rows"], g["cols"], g["vals"], n)
    u = int(want[0][-1])
    _assert_csr(sparse.CSR(rpn, cin[:u], vn[:u], (n, n)), *want, "normalise with the whole workspace")
