"""The word counter's entry points without a GPU: gcnk_text_* declared in include/gcnk_text.h (which include/gcnk.h
includes), exported and bound within ABI 13, every refusal before any HIP call with its reason in gcnk_last_error,
the public names, from_sklearn's refusal of every setting it does not restate, and the table builder's stand-alone
check program under the host compiler's sanitizers (make table-sanitize; a CPU program of its own)."""
import ctypes
import os
import shutil
import subprocess
import types

import pytest
import torch

import gcn_amd
from graph_convolutional_networks_for_text_classification_amd import TextCounter, _lib, text_count

import abi_bound
from lda_abi import CSRC, PTR

COUNT, EMIT = "gcnk_text_count", "gcnk_text_emit"
NAMES = {"gcnk_text_table_slots": 1, "gcnk_text_table_bytes": 2, "gcnk_text_table_build": 6, "gcnk_text_token_bound": 2,
         "gcnk_text_workspace_bytes": 3, COUNT: 14, EMIT: 9}   # argument counts, the stream included
V, BLOB = 3, 11                                # "oil", "price", "sea": 8 slots
TABLE_BYTES = 32 + 8 * 8 + 4 * (V + 1) + BLOB + 5
BIG = 1 << 40                                  # a workspace size no refusal but its own looks at
# entry point -> its operands in the declaration's order as (keyword, default)
ENTRY = {
    COUNT: (("bytes", PTR), ("N", 100), ("offsets", PTR), ("B", 4), ("table", PTR), ("table_bytes", TABLE_BYTES), ("V", V),
            ("slots", 8), ("max_word", 5), ("blob_bytes", BLOB), ("indptr", PTR), ("workspace", PTR),
            ("workspace_bytes", BIG)),
    EMIT: (("N", 100), ("B", 4), ("V", V), ("nnz", 7), ("indices", PTR), ("counts", PTR), ("workspace", PTR),
           ("workspace_bytes", BIG)),
}


def call(name, **kw):
    """The entry point on its defaults with ``kw`` over them -> (return code, gcnk_last_error)."""
    spec = ENTRY[name]
    assert set(kw) <= {k for k, _ in spec}, (name, kw)
    lib = _lib.load()
    rc = getattr(lib, name)(*[kw.get(k, d) for k, d in spec], None)
    return rc, lib.gcnk_last_error().decode()


def _ids(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


def test_symbols_declared_exported_and_bound():
    text = abi_bound.header("gcnk_text.h")[0]
    assert '#include "gcnk_text.h"' in abi_bound.header("gcnk.h")[1]        # a C caller of gcnk.h sees them
    assert abi_bound.declared_names("gcnk_text.h") == set(NAMES) and len(NAMES) == 7   # these and nothing else
    abi_bound.assert_declared_exported_bound(NAMES, header="gcnk_text.h")
    assert all(name not in ENTRY or len(ENTRY[name]) + 1 == nargs for name, nargs in NAMES.items())
    want = {"gcnk_text_table_slots": ctypes.c_int32, "gcnk_text_table_bytes": ctypes.c_int64,
            "gcnk_text_token_bound": ctypes.c_int64, "gcnk_text_workspace_bytes": ctypes.c_int64}
    assert all(_lib.SIGNATURES[n][0] is want.get(n, ctypes.c_int) for n in NAMES)
    assert "within ABI 13" in text and "FNV-1a" in text and "CountVectorizer" in text
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert "text_count.hip" in make and "text_table.cpp" in make and "table-sanitize" in make
    with open(os.path.join(CSRC, "text_count.hip")) as f:
        kernels = f.read()
    with open(os.path.join(CSRC, "text_table.cpp")) as f:
        host = f.read()
    assert all(name in kernels + host for name in NAMES)
    assert "hip/" not in host and "hipLaunch" not in host and "gcnk_common.h" not in host   # plain C++, no HIP
    assert "__ballot" in kernels and "__global__" in kernels   # the tokeniser is hand-written HIP


def test_public_names():
    assert gcn_amd.TextCounter is TextCounter is text_count.TextCounter and gcn_amd.text_count is text_count
    assert {"TextCounter", "text_count"} <= set(gcn_amd.__all__)
    assert all(callable(getattr(TextCounter, k)) for k in ("from_sklearn", "pack", "count", "__call__"))
    doc = text_count.__doc__
    assert "Still on the host" in doc and "min_df" in doc and "pack" in doc


def test_sizes():
    lib = _lib.load()
    assert lib.gcnk_text_token_bound(0, 0) == 1 and lib.gcnk_text_token_bound(10, 3) == 7
    assert lib.gcnk_text_token_bound((1 << 32) - 3, 0) == (1 << 31) - 1      # the last the int32 CSR holds
    assert lib.gcnk_text_token_bound((1 << 32) - 2, 0) == _lib.EUNSUP
    assert lib.gcnk_text_token_bound((1 << 32) - 12, 10) == _lib.EUNSUP and "2^31" in lib.gcnk_last_error().decode()
    assert lib.gcnk_text_token_bound(-1, 0) == _lib.EARG and lib.gcnk_text_token_bound(5, -1) == _lib.EARG
    small, large = lib.gcnk_text_workspace_bytes(100, 4, V), lib.gcnk_text_workspace_bytes(100000, 400, V)
    assert 0 < small < large
    # two key arrays of 8 bytes and three of 4 a key slot, at the least
    assert large >= 28 * lib.gcnk_text_token_bound(100000, 400)
    assert lib.gcnk_text_workspace_bytes(100, 4, 0) == _lib.EARG
    assert lib.gcnk_text_workspace_bytes(100, 4, (1 << 29) + 1) == _lib.EUNSUP
    assert lib.gcnk_text_workspace_bytes((1 << 32), 4, V) == _lib.EUNSUP
    assert lib.gcnk_text_table_bytes(BLOB, V) == TABLE_BYTES and lib.gcnk_text_table_slots(V) == 8


@pytest.mark.parametrize("kw", [dict(N=-1), dict(B=-1), dict(V=0), dict(V=-2), dict(bytes=None), dict(offsets=None),
                                dict(table=None), dict(indptr=None), dict(table=PTR + 4), dict(slots=4), dict(slots=16),
                                dict(table_bytes=TABLE_BYTES - 8), dict(table_bytes=TABLE_BYTES + 8), dict(max_word=0),
                                dict(max_word=BLOB + 1), dict(blob_bytes=-1), dict(workspace=None),
                                dict(workspace_bytes=0), dict(workspace_bytes=1000)], ids=_ids)
def test_count_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = call(COUNT, **kw)
    assert rc == _lib.EARG and COUNT in msg


def test_count_workspace_boundary_and_unsupported_sizes():
    need = _lib.load().gcnk_text_workspace_bytes(100, 4, V)
    rc, msg = call(COUNT, workspace_bytes=need - 1)
    assert rc == _lib.EARG and "workspace" in msg and str(need) in msg
    for who in (COUNT, EMIT):
        rc, msg = call(who, N=(1 << 32) - 6)                      # N + B = 2^32 - 2
        assert rc == _lib.EUNSUP and who in msg and "2^31" in msg
        rc, msg = call(who, V=(1 << 29) + 1)
        assert rc == _lib.EUNSUP and who in msg
    rc, msg = call(COUNT, blob_bytes=1 << 31)
    assert rc == _lib.EUNSUP and COUNT in msg


@pytest.mark.parametrize("kw", [dict(N=-1), dict(B=-1), dict(V=0), dict(nnz=-1), dict(nnz=54), dict(indices=None),
                                dict(counts=None), dict(workspace=None), dict(workspace_bytes=1000),
                                dict(nnz=1, B=0), dict(nnz=1, N=0)], ids=_ids)
def test_emit_refuses_bad_arguments_before_any_hip_call(kw):
    rc, msg = call(EMIT, **kw)
    assert rc == _lib.EARG and EMIT in msg


def test_emit_of_nothing_is_no_launch():
    assert call(EMIT, nnz=0, indices=None, counts=None, workspace=None, workspace_bytes=0)[0] == _lib.OK


def _vectorizer(**kw):
    settings = dict(input="content", token_pattern=r"\S+", lowercase=False, ngram_range=(1, 1), stop_words=None,
                    strip_accents=None, tokenizer=None, preprocessor=None, analyzer="word", binary=False,
                    vocabulary_={"oil": 0, "price": 1})
    settings.update(kw)
    return types.SimpleNamespace(**settings)


@pytest.mark.parametrize("name,value", [
    ("token_pattern", r"(?u)\b\w\w+\b"), ("token_pattern", None), ("lowercase", True), ("ngram_range", (1, 2)),
    ("ngram_range", (2, 2)), ("stop_words", "english"), ("stop_words", ["the"]), ("strip_accents", "unicode"),
    ("strip_accents", "ascii"), ("tokenizer", str.split), ("preprocessor", str.strip), ("analyzer", "char"),
    ("analyzer", "char_wb"), ("analyzer", str.split), ("binary", True), ("input", "filename"), ("input", "file")])
def test_from_sklearn_refuses_every_setting_it_does_not_restate(name, value):
    with pytest.raises(RuntimeError, match=name):
        TextCounter.from_sklearn(_vectorizer(**{name: value}), "cuda")


def test_python_refusals_that_need_no_device():
    with pytest.raises(RuntimeError, match="ROCm GPU"):      # never a host fallback
        TextCounter(["oil", "price"], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        TextCounter.from_sklearn(_vectorizer(), "cpu")       # (the supported settings pass from_sklearn's check)
    unfitted = _vectorizer()
    del unfitted.vocabulary_
    with pytest.raises(RuntimeError, match="not fitted"):
        TextCounter.from_sklearn(unfitted, "cuda")
    sk = pytest.importorskip("sklearn.feature_extraction.text")
    with pytest.raises(RuntimeError, match="token_pattern"):
        TextCounter.from_sklearn(sk.CountVectorizer().fit(["oil price"]), "cuda")
    with pytest.raises(RuntimeError, match="lowercase"):
        TextCounter.from_sklearn(sk.CountVectorizer(token_pattern=r"\S+").fit(["oil price"]), "cuda")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        TextCounter.from_sklearn(sk.CountVectorizer(token_pattern=r"\S+", lowercase=False).fit(["oil price"]), "cpu")
    assert not torch.zeros(1).is_cuda


def test_table_sanitize_builds_and_runs_clean(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None and shutil.which("make"), "make and a host C++ compiler are needed (csrc/Makefile's HOSTCXX)"
    run = subprocess.run(["make", "table-sanitize", f"OUTDIR={tmp_path}", f"HOSTCXX={cxx}"], cwd=CSRC,
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.rstrip().splitlines()[-1]
    assert last.startswith("text_table_check:") and last.endswith("words ok")
    assert "-fsanitize=address,undefined" in run.stdout and "runtime error" not in run.stderr
