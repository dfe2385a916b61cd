"""CPU checks of gcnk_keep_best_f32's C-ABI (include/gcnk.h) and of its rule:
the ctypes mirrors of gcnk_keep_tensor and gcnk_keep_state match the C layout,
every documented GCNK_EARG case is refused on the host before any launch, and
the Python model of the rule (tests/keep_ref.py) keeps exactly the epoch at
which oracle.gcn_ref.EarlyStopping last took a ``best_score = score`` branch.
No compute without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, train
import graph_convolutional_networks_for_text_classification_amd as pkg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_ref  # noqa: E402
from abi_bound import assert_declared_exported_bound  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = ctypes.c_void_p(4096)   # a plausible, suitably aligned device address: never dereferenced on the host


def _table(*tensors):
    tab = (_lib.KeepTensor * max(1, len(tensors)))()
    for k, (src, dst, numel) in enumerate(tensors):
        tab[k].src, tab[k].dst, tab[k].numel = src, dst, numel
    return tab


def _keep(lib, **kw):
    a = dict(t=_table((1 << 20, 2 << 20, 100)), nt=1, es=P16, st=P16, flags=0)
    a.update(kw)
    return lib.gcnk_keep_best_f32(a["t"], a["nt"], a["es"], a["st"], a["flags"], None)


BAD = {
    "ntensors=-1": dict(nt=-1),
    "ntensors=9": dict(nt=9, t=_table(*[((k + 1) << 20, (k + 21) << 20, 4) for k in range(9)])),
    "null table": dict(t=None),
    "null epoch_state": dict(es=None),
    "null state": dict(st=None),
    "numel<0": dict(t=_table((1 << 20, 2 << 20, -1))),
    "null src": dict(t=_table((None, 2 << 20, 4))),
    "null dst": dict(t=_table((1 << 20, None, 4))),
    "src is its own dst": dict(t=_table((1 << 20, 1 << 20, 4))),
    "src overlaps its own dst by one element": dict(t=_table((1 << 20, (1 << 20) + 12, 4))),
    "dst overlaps its own src from below": dict(t=_table(((1 << 20) + 12, 1 << 20, 4))),
    "src overlaps another tensor's dst": dict(nt=2, t=_table((1 << 20, 2 << 20, 100), (3 << 20, (1 << 20) + 396, 8))),
    "unknown flag bit 2": dict(flags=2),
    "unknown flag bits 1|4": dict(flags=5),
    "state not 4-B aligned": dict(st=ctypes.c_void_p(4098)),
}


@pytest.mark.parametrize("label", list(BAD))
def test_keep_rejects_bad_arguments_on_the_host(label):
    lib = _lib.load()
    assert _keep(lib, **BAD[label]) == _lib.EARG
    assert b"gcnk_keep_best_f32" in lib.gcnk_last_error()


def test_keep_of_no_tensors_succeeds_and_launches_nothing():
    lib = _lib.load()
    assert _keep(lib, nt=0) == _lib.OK
    assert _keep(lib, nt=0, t=None, flags=_lib.KEEP_HOLD_STATE) == _lib.OK
    # with HOLD_STATE a launch of empty tensors has nothing to do at all: decided on the host, nothing launched
    assert _keep(lib, t=_table((None, None, 0)), flags=_lib.KEEP_HOLD_STATE) == _lib.OK


C_LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gcnk.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(gcnk_keep_tensor), offsetof(gcnk_keep_tensor, src),
         offsetof(gcnk_keep_tensor, dst), offsetof(gcnk_keep_tensor, numel), sizeof(gcnk_keep_state),
         offsetof(gcnk_keep_state, seen), offsetof(gcnk_keep_state, best), offsetof(gcnk_keep_state, arrivals),
         offsetof(gcnk_keep_state, copies), GCNK_KEEP_MAX_TENSORS, GCNK_KEEP_CHUNK, GCNK_KEEP_HOLD_STATE);
  return 0;
}
"""


def _members(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(d.replace("*", " * ").split()) for d in body.split(";") if d.strip()]


def test_ctypes_mirrors_of_the_keep_structs_match_the_c_layout(tmp_path):
    T, S = _lib.KeepTensor, _lib.KeepState
    mirror = ([ctypes.sizeof(T)] + [getattr(T, f).offset for f in ("src", "dst", "numel")] +
              [ctypes.sizeof(S)] + [getattr(S, f).offset for f in ("seen", "best", "arrivals", "copies")])
    assert mirror == [24, 0, 8, 16, 16, 0, 4, 8, 12]
    assert [name for name, _ in T._fields_] == ["src", "dst", "numel"]
    assert [name for name, _ in S._fields_] == ["seen", "best", "arrivals", "copies"]
    # the header's own text: the structs' members in this order, and the constants
    with open(os.path.join(ROOT, "include", "gcnk.h")) as f:
        src = f.read()
    assert _members(src, "gcnk_keep_tensor") == [("const", "float", "*", "src"), ("float", "*", "dst"),
                                                 ("int64_t", "numel")]
    assert _members(src, "gcnk_keep_state") == [("int32_t", "seen"), ("int32_t", "best"), ("int32_t", "arrivals"),
                                                ("int32_t", "copies")]
    assert "#define GCNK_KEEP_MAX_TENSORS 8\n" in src and "#define GCNK_KEEP_CHUNK 8192\n" in src
    assert re.search(r"#define GCNK_KEEP_HOLD_STATE 1\b", src)
    assert (_lib.KEEP_MAX_TENSORS, _lib.KEEP_CHUNK, _lib.KEEP_HOLD_STATE) == (8, 8192, 1)
    assert "#define GCNK_ABI_VERSION 13\n" in src   # an addition within ABI 13
    # and, where a C compiler is at hand, what it lays out
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        (tmp_path / "layout.c").write_text(C_LAYOUT)
        exe = str(tmp_path / "layout")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == mirror + [8, 8192, 1]


def test_python_surface():
    assert pkg.BestKeeper is train.BestKeeper and "BestKeeper" in pkg.__all__
    import inspect
    assert inspect.signature(train.fit).parameters["restore_best"].default is False
    assert inspect.signature(train.run_epoch).parameters["keeper"].default is None
    assert train.FitResult._fields == ("history", "epochs", "stop_reason", "optimizer", "log")
    assert _lib.SIGNATURES["gcnk_keep_best_f32"][0] is ctypes.c_int
    assert_declared_exported_bound({"gcnk_keep_best_f32": 6}, restype=ctypes.c_int, newer=False)


# ------------------------------------------------------------------------------ the rule

@pytest.mark.parametrize("label", list(keep_ref.SCRIPTS))
def test_the_rule_keeps_the_epoch_of_the_reference_s_last_checkpoint(label):
    patience, delta, max_epoch, losses, kept_at_the_end = keep_ref.SCRIPTS[label]
    py = keep_ref.TracedStopping(patience, delta)
    tail = keep_ref.TailWords(py, max_epoch)
    keep = keep_ref.KeepModel()
    stopped_at = None
    for e, loss in enumerate(losses):
        was = (keep.words, tail.epoch, tail.counter, tail.stopped)
        saved_before = len(py.saved)
        tail.record(loss)
        copied = keep.look(tail.epoch, tail.counter)
        if stopped_at is not None:   # behind the stop nothing moves
            assert not copied and (keep.words, tail.epoch, tail.counter, tail.stopped) == was, f"{label}: epoch {e}"
            continue
        # a copy exactly where the reference assigned best_score (utils.py:244, :254) in this call
        assert copied == (len(py.saved) == saved_before + 1), f"{label}: epoch {e}"
        assert keep.kept == py.saved[-1], f"{label}: epoch {e}"
        assert keep.words == (e + 1, py.saved[-1] + 1, 0, len(py.saved))
        # a second look at the same tail (a launch repeated without a tail between) never copies
        twice = keep_ref.KeepModel()
        twice.seen, twice.best, twice.copies = keep.seen, keep.best, keep.copies
        assert not twice.look(tail.epoch, tail.counter) and twice.words == keep.words
        if tail.stopped:
            stopped_at = e
            if tail.stopped == 1:
                assert not copied, f"{label}: a patience stop never copies"
    assert stopped_at is not None and len(losses) - 1 - stopped_at == 5, f"{label}: five launches behind the stop"
    assert keep.kept == py.saved[-1] == kept_at_the_end
    if label.startswith("max_epoch"):
        assert tail.stopped == 2 and keep.kept == stopped_at   # copied in the stopping epoch's own launch


def test_hold_state_decides_the_same_and_moves_no_word():
    m = keep_ref.KeepModel()
    assert m.look(1, 0, hold=True) and m.words == (0, 0, 0, 0)
    assert m.look(1, 0) and m.words == (1, 1, 0, 1)
    assert not m.look(2, 1, hold=True) and not m.look(2, 1) and m.words == (2, 1, 0, 1)
    assert not m.look(2, 0, hold=True) and not m.look(2, 0) and m.words == (2, 1, 0, 1)   # not fresh
