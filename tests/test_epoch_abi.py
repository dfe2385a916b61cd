"""CPU checks of the epoch tail's and the gated Adam's C-ABI (include/gcnk.h:
gcnk_epoch_tail_f32, gcnk_epoch_tail_workspace_bytes, gcnk_adam_gated_f32):
the symbols exist, validate their arguments on the host before any launch, the
ctypes mirror of gcnk_epoch_state matches the C layout, and train.fit refuses
CPU tensors like the rest of the product path.  No compute without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, _lib, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = ctypes.c_void_p(4096)   # a plausible, suitably aligned device address: never dereferenced on the host


def _tail(lib, **kw):
    a = dict(logits=P16, ld=8, M=100, P=8, target=P16, counts=P16, n=10, train_loss=None, state=P16, history=P16,
             max_epoch=5, patience=3, delta=0.0, workspace=P16, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.gcnk_epoch_tail_f32(*(a[k] for k in ("logits", "ld", "M", "P", "target", "counts", "n", "train_loss",
                                                    "state", "history", "max_epoch", "patience", "delta", "workspace",
                                                    "workspace_bytes", "stream")))


@pytest.mark.parametrize("bad", [
    dict(state=None), dict(history=None), dict(workspace=None),
    dict(P=0), dict(P=1025, ld=1025), dict(ld=7),
    dict(workspace_bytes=0), dict(workspace=ctypes.c_void_p(4100)), dict(state=ctypes.c_void_p(4100)),
    dict(patience=-1), dict(max_epoch=0), dict(n=-1), dict(M=-1), dict(delta=float("nan")),
    dict(logits=None), dict(target=None),
], ids=lambda b: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in b.items()))
def test_epoch_tail_rejects_bad_arguments_on_the_host(bad):
    lib = _lib.load()
    assert _tail(lib, **bad) == _lib.EARG
    assert b"gcnk_epoch_tail_f32" in lib.gcnk_last_error()


def test_epoch_tail_workspace_size_is_the_loss_forward_s_partition():
    lib = _lib.load()
    for M, P in ((1, 2), (127, 3), (7724, 8), (300, 257), (40000, 8)):
        nb = lib.gcnk_epoch_tail_workspace_bytes(M, P)
        assert nb == lib.gcnk_ce_workspace_bytes(M, P) > 0 and nb % 8 == 0
        # one byte short is refused
        assert _tail(lib, M=M, P=P, ld=P, workspace_bytes=nb - 1) == _lib.EARG
    assert lib.gcnk_epoch_tail_workspace_bytes(0, 8) == 8       # an empty set still runs the state machine
    assert lib.gcnk_epoch_tail_workspace_bytes(10, 0) == _lib.EARG
    assert lib.gcnk_epoch_tail_workspace_bytes(10, 1025) == _lib.EARG
    assert lib.gcnk_epoch_tail_workspace_bytes(-1, 8) == _lib.EARG


def test_gated_adam_has_adam_s_argument_errors():
    lib = _lib.load()
    tab = (_lib.AdamTensor * 1)()
    tab[0].p = tab[0].g = tab[0].m = tab[0].v = 4096
    tab[0].numel = 4
    ok = dict(t=tab, nt=1, lr=0.02, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, state=P16, flags=0)

    def call(fn, extra, **kw):
        a = dict(ok, **kw)
        return fn(a["t"], a["nt"], a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["state"], a["flags"], *extra, None)

    for kw in (dict(nt=-1), dict(nt=9), dict(lr=-1.0), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1e-8), dict(wd=-0.1),
               dict(flags=4), dict(t=None), dict(state=None), dict(lr=float("nan"))):
        assert call(lib.gcnk_adam_f32, (), **kw) == _lib.EARG, kw
        assert call(lib.gcnk_adam_gated_f32, (P16,), **kw) == _lib.EARG, kw
        assert b"gcnk_adam_gated_f32" in lib.gcnk_last_error()
        assert call(lib.gcnk_adam_gated_f32, (None,), **kw) == _lib.EARG, kw
    bad = (_lib.AdamTensor * 1)()
    bad[0].p = bad[0].g = bad[0].m = 4096   # v is NULL
    bad[0].numel = 4
    assert call(lib.gcnk_adam_gated_f32, (P16,), t=bad) == _lib.EARG
    bad[0].v, bad[0].numel = 4096, -1
    assert call(lib.gcnk_adam_gated_f32, (P16,), t=bad) == _lib.EARG
    assert call(lib.gcnk_adam_gated_f32, (P16,), nt=0) == _lib.OK   # nothing to do, nothing launched


C_LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "gcnk.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(gcnk_epoch_state), offsetof(gcnk_epoch_state, epoch),
         offsetof(gcnk_epoch_state, stopped), offsetof(gcnk_epoch_state, stop_epoch),
         offsetof(gcnk_epoch_state, counter), offsetof(gcnk_epoch_state, best), offsetof(gcnk_epoch_state, arrivals),
         offsetof(gcnk_epoch_state, reserved), GCNK_EPOCH_STOP_PATIENCE, GCNK_EPOCH_STOP_MAX_EPOCH,
         GCNK_EPOCH_ROW_WORDS(8));
  return 0;
}
"""


def test_ctypes_mirror_of_the_epoch_state_matches_the_c_layout(tmp_path):
    S = _lib.EpochState
    mirror = [ctypes.sizeof(S)] + [getattr(S, f).offset for f in ("epoch", "stopped", "stop_epoch", "counter", "best",
                                                                 "arrivals", "reserved")]
    assert mirror == [32, 0, 4, 8, 12, 16, 24, 28]
    assert [name for name, _ in S._fields_] == ["epoch", "stopped", "stop_epoch", "counter", "best", "arrivals",
                                                "reserved"]
    # the header's own text: the struct's members in this order, and the constants
    with open(os.path.join(ROOT, "include", "gcnk.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct gcnk_epoch_state \{(.*?)\} gcnk_epoch_state;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [tuple(d.split()) for d in body.split(";") if d.strip()]
    assert decl == [("int32_t", "epoch"), ("int32_t", "stopped"), ("int32_t", "stop_epoch"), ("int32_t", "counter"),
                    ("double", "best"), ("int32_t", "arrivals"), ("int32_t", "reserved")]
    assert "#define GCNK_EPOCH_STOP_PATIENCE 1\n" in src and "#define GCNK_EPOCH_STOP_MAX_EPOCH 2\n" in src
    assert (_lib.EPOCH_STOP_PATIENCE, _lib.EPOCH_STOP_MAX_EPOCH) == (1, 2)
    assert _lib.epoch_row_words(8) == 27
    # and, where a C compiler is at hand, what it lays out
    import shutil
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        (tmp_path / "layout.c").write_text(C_LAYOUT)
        exe = str(tmp_path / "layout")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
        assert [int(x) for x in out] == mirror + [1, 2, 27]


def test_fit_and_the_epoch_log_refuse_cpu_tensors(r8):
    """No silent CPU fallback: fit on CPU inputs raises instead of training."""
    torch.manual_seed(0)
    m = GCN(nfeat=r8["nfeat"], nhid=16, nclass=r8["nclass"], dropout=0.5)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        train.fit(m, r8["features"], r8["adj"], torch.as_tensor(r8["target"]), torch.arange(10), torch.arange(10, 20))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        train.EpochLog(5, 8, "cpu")
    assert sys.modules[train.__name__].FitResult._fields == ("history", "epochs", "stop_reason", "optimizer", "log")
