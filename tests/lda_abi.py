"""The call harness of the LDA ABI test files (test_lda_abi.py, test_lda_fit_abi.py, test_lda_online_abi.py and
test_lda_bound_abi.py): one row per gcnk_lda_* entry point, the declared / exported / bound check they share, and
the whole of include/gcnk_lda.h against their names.  No GPU: every call made through here is refused before any HIP
call, so PTR is never dereferenced."""
import os

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

import abi_bound
from abi_bound import header  # noqa: F401  (the test files take it from here)

CSRC = os.path.join(abi_bound.ROOT, "graph-convolutional-networks-for-text-classification_amd", "csrc")
PTR = 0x10000   # an aligned address that no refused call dereferences


def _K(a):
    return a["K"]


def _V(a):
    return a["V"]


def _even_K(a):
    return (a["K"] + 1) // 2 * 2


_DOCS = (("indptr", PTR), ("indices", PTR), ("counts", PTR), ("kind", 0), ("B", 8), ("V", 100), ("K", 16), ("table", PTR),
         ("ldt", _even_K), ("alpha", 0.1), ("tol", 1e-3), ("max_iter", 100))
_INDEX = (("wptr", PTR), ("pos", PTR), ("doc", PTR), ("nnz", 50))
_MODEL = (("ratio", PTR), ("etheta", PTR), ("lde", _K), ("B", 8), ("V", 100), ("K", 16), ("table", PTR), ("ldt", _even_K),
          ("eta", 0.1))
_BUILDER = (("src", PTR), ("ld", 100), ("K", 16), ("V", 100), ("table", PTR), ("ldt", 16))
# entry point -> its operands in the declaration's order as (keyword, default); a function default is taken of the
# other operands.  The stream, always null, follows them.
ENTRY = {
    "gcnk_lda_exp_dirichlet_f64": _BUILDER,
    "gcnk_lda_table_from_exp_f64": _BUILDER,
    "gcnk_lda_estep_f64": _DOCS + (("theta", PTR), ("ldth", _K), ("gamma", None), ("iters", None), ("x", None),
                                   ("ldx", _K), ("a", None), ("lda", _K), ("thr", 0.02)),
    "gcnk_lda_estep_fit_f64": _DOCS + (("gamma0", PTR), ("ldg0", _K), ("nnz", 50), ("ratio", PTR), ("etheta", PTR),
                                       ("lde", _K), ("gamma", None), ("ldg", 0), ("iters", None)),
    "gcnk_lda_mstep_f64": _INDEX + _MODEL + (("lam", PTR), ("ldl", _V)),
    "gcnk_lda_mstep_online_f64": _INDEX + (("doc_lo", 2), ("doc_hi", 6)) + _MODEL + (
        ("rho", 0.5), ("doc_ratio", 4.0), ("lam", PTR), ("ldl", _V)),
}


def call(name, entry=ENTRY, **kw):
    """The entry point on its defaults (``entry``'s row) with ``kw`` over them -> (return code, gcnk_last_error)."""
    spec = entry[name]
    assert set(kw) <= {k for k, _ in spec}, (name, kw)
    given = {k: kw.get(k, d) for k, d in spec if not callable(d)}
    lib = _lib.load()
    rc = getattr(lib, name)(*[kw[k] if k in kw else d(given) if callable(d) else d for k, d in spec], None)
    return rc, lib.gcnk_last_error().decode()


def kernels_source():
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "lda_estep.hip" in f.read()
    with open(os.path.join(CSRC, "lda_estep.hip")) as f:
        return f.read()


def assert_declared_exported_bound(names, entry=ENTRY, restype=None):
    """names: entry point -> its argument count, the stream included (abi_bound's check against include/gcnk_lda.h,
    and ``entry``'s rows agree)."""
    abi_bound.assert_declared_exported_bound(names, restype=restype, header="gcnk_lda.h")
    for name, nargs in names.items():
        assert name not in entry or len(entry[name]) + 1 == nargs


def all_names():
    """The names of the four LDA ABI test files, which between them are to be all that gcnk_lda.h declares."""
    import test_lda_abi, test_lda_bound_abi, test_lda_fit_abi, test_lda_online_abi   # noqa: E401 (they import this)
    return (set(test_lda_abi.NAMES) | set(test_lda_fit_abi.NAMES) | {test_lda_online_abi.ONLINE}
            | set(test_lda_bound_abi.NAMES))
