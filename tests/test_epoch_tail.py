"""GPU checks of the fused epoch tail (csrc/epoch.hip, gcnk_epoch_tail_f32),
called through ctypes on a fresh state.

The yardsticks are the kernels it fuses, on the same buffers: the validation
loss must be BITWISE gcnk_ce_forward_f32's and the class counts exactly
gcnk_class_stats's; the early-stopping state machine is held, launch by launch,
to oracle.gcn_ref.EarlyStopping (utils.py:216-255) driven by the same losses."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib
from oracle import gcn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Tail:
    """A fresh (zeroed) state and history, and the launch."""

    def __init__(self, P, max_epoch, patience=100, delta=0.0):
        self.P, self.max_epoch, self.patience, self.delta = P, max_epoch, patience, delta
        self.state = torch.zeros(8, dtype=torch.int32, device=DEV)
        self.hist = torch.zeros(max_epoch, _lib.epoch_row_words(P), dtype=torch.int32, device=DEV)

    def launch(self, z, tgt, counts, n, train_loss=None):
        lib = _lib.load()
        M = z.shape[0]
        nb = lib.gcnk_epoch_tail_workspace_bytes(M, self.P)
        assert nb > 0
        ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device=DEV)   # never zeroed by anyone
        _lib.check(lib.gcnk_epoch_tail_f32(_ptr(z), z.stride(0), M, self.P, _ptr(tgt), _ptr(counts), n,
                                           _ptr(train_loss), _ptr(self.state), _ptr(self.hist), self.max_epoch,
                                           self.patience, self.delta, _ptr(ws), nb, _stream()), "gcnk_epoch_tail_f32")
        torch.cuda.synchronize()

    def host_state(self):
        return _lib.EpochState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def row(self, e):
        r = self.hist[e].cpu().numpy()
        return r[:2].copy(), r[2:].copy()   # (train loss, val loss) bits; TP | FP | FN | correct


def _reference(z, tgt, idx, counts, n):
    """(loss bits, counts) of gcnk_ce_forward_f32 and gcnk_class_stats on the same buffers."""
    lib = _lib.load()
    M, P = z.shape
    nb = lib.gcnk_ce_workspace_bytes(M, P)
    ws = torch.empty(max(1, nb // 8), dtype=torch.float64, device=DEV)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    _lib.check(lib.gcnk_ce_forward_f32(_ptr(z), z.stride(0), M, P, _ptr(tgt), _ptr(counts), n, _ptr(loss), None,
                                       _ptr(ws), nb, _stream()), "gcnk_ce_forward_f32")
    stats = torch.empty(3 * P + 1, dtype=torch.int32, device=DEV)
    _lib.check(lib.gcnk_class_stats(_ptr(z), z.stride(0), _ptr(tgt), _ptr(idx), idx.numel(), P, _ptr(stats),
                                    _stream()), "gcnk_class_stats")
    torch.cuda.synchronize()
    return loss.view(torch.int32).item(), stats.cpu().numpy()


def _row_counts(idx, M):
    counts = torch.empty(M + 1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().gcnk_ce_row_counts(_ptr(idx), idx.numel(), M, _ptr(counts), _stream()), "gcnk_ce_row_counts")
    return counts


def _inputs(M, P, pad, seed):
    """Logits on a 0.5 grid (ties: the first maximum must win) in a buffer of leading dimension P + pad
    whose padding is NaN; an index set with duplicates that leaves rows unscored; labels that are garbage
    on exactly the unscored rows."""
    rng = np.random.default_rng(seed)
    back = torch.full((M, P + pad), float("nan"), device=DEV)
    zh = (np.round(rng.normal(0, 2, (M, P)) * 2) / 2).astype(np.float32)
    back[:, :P] = torch.from_numpy(zh).to(DEV)
    z = back[:, :P]
    if M == 1:
        idx_h = np.array([0, 0, 0])
    else:
        some = rng.choice(M, max(1, M // 2), replace=False)
        idx_h = np.concatenate([some, some[: max(1, len(some) // 7)], some[:1], some[:1]])   # duplicates, a triple
        rng.shuffle(idx_h)
    tgt_h = rng.integers(0, P, M).astype(np.int64)
    unscored = np.ones(M, bool)
    unscored[idx_h] = False
    tgt_h[unscored] = rng.choice(np.array([-7, P, 2 ** 40, -2 ** 40]), int(unscored.sum()))
    idx = torch.from_numpy(idx_h.astype(np.int64)).to(DEV)
    tgt = torch.from_numpy(tgt_h).to(DEV)
    return z, tgt, idx, _row_counts(idx, M)


SHAPES = [(1, 2), (127, 3), (129, 8), (7724, 8), (5000, 20), (300, 257), (40000, 8)]


def _check_against_the_fused_kernels(z, tgt, idx, counts, label):
    M, P = z.shape
    n = idx.numel()
    ref_loss, ref_stats = _reference(z, tgt, idx, counts, n)
    tl = torch.tensor([1.25], device=DEV)
    t = Tail(P, max_epoch=3)
    t.launch(z, tgt, counts, n, tl)
    t.launch(z, tgt, counts, n, tl)
    (l0, c0), (l1, c1), (l2, c2) = t.row(0), t.row(1), t.row(2)
    print(f"{label}: val loss bits {int(l0[1]) & 0xffffffff:#010x} reference {ref_loss & 0xffffffff:#010x} "
          f"correct {c0[-1]} reference {ref_stats[-1]} of n = {n}")
    assert int(l0[1]) == ref_loss, f"{label}: the validation loss is not bitwise gcnk_ce_forward_f32's"
    assert np.array_equal(c0, ref_stats), f"{label}: the class counts differ from gcnk_class_stats's"
    assert int(l0[0]) == np.float32(1.25).view(np.int32), f"{label}: the train loss was not copied in"
    assert np.array_equal(l0, l1) and np.array_equal(c0, c1), f"{label}: a second launch wrote a different row"
    assert not l2.any() and not c2.any(), f"{label}: a row past the recorded epochs was written"
    st = t.host_state()
    assert (st.epoch, st.stopped, st.arrivals) == (2, 0, 0)
    return ref_loss, ref_stats


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("M,P", SHAPES)
def test_loss_is_bitwise_the_loss_kernel_s_and_counts_are_the_stats_kernel_s(M, P, pad):
    z, tgt, idx, counts = _inputs(M, P, pad, seed=1000 * M + P + pad)
    if (M, P) == (40000, 8):
        nb = _lib.load().gcnk_epoch_tail_workspace_bytes(M, P)
        assert nb // 8 > 256   # the reduce's runs are longer than one partial
    ref_loss, _ = _check_against_the_fused_kernels(z, tgt, idx, counts, f"M={M} P={P} ld={P + pad}")
    assert not math.isnan(np.int32(ref_loss).view(np.float32))


@pytest.mark.parametrize("M,P", [(129, 8), (300, 257)])
def test_a_nan_logit_in_a_scored_row_wins_the_argmax_and_makes_the_loss_nan(M, P):
    z, tgt, idx, counts = _inputs(M, P, 3, seed=5)
    r = int(idx[0])
    c = P // 2
    z[r, c] = float("nan")
    tgt[r] = c
    ref_loss, ref_stats = _check_against_the_fused_kernels(z, tgt, idx, counts, f"NaN logit M={M} P={P}")
    assert math.isnan(np.int32(ref_loss).view(np.float32))
    assert ref_stats[c] >= 1   # the NaN column is the prediction, and here the label: a true positive


@pytest.mark.parametrize("bad", [-1, 8, 2 ** 33])
def test_a_scored_target_outside_the_classes_is_a_nan_loss_an_fp_and_no_fn(bad):
    M, P = 129, 8
    z, tgt, idx, counts = _inputs(M, P, 0, seed=9)
    clean_loss, clean = _reference(z, tgt, idx, counts, idx.numel())
    r = int(idx[0])
    mult = int(counts[r])
    tgt[r] = bad
    ref_loss, stats = _check_against_the_fused_kernels(z, tgt, idx, counts, f"target {bad}")
    assert math.isnan(np.int32(ref_loss).view(np.float32)) and not math.isnan(np.int32(clean_loss).view(np.float32))
    tp, fp, fn = stats[:P], stats[P:2 * P], stats[2 * P:3 * P]
    cfp, cfn = clean[P:2 * P], clean[2 * P:3 * P]
    assert mult >= 1 and cfn.sum() == cfp.sum()   # with every label in range a miss is an FP and an FN
    assert tp.sum() + fp.sum() == idx.numel()     # every scored occurrence is a TP or an FP: this row's are FPs
    assert fn.sum() == fp.sum() - mult            # ... and they alone have no FN
    assert stats[-1] == tp.sum()


def test_an_empty_index_set_is_the_nan_loss_of_the_loss_kernel():
    M, P = 40, 8
    z, tgt, _, _ = _inputs(M, P, 0, seed=2)
    idx = torch.empty(0, dtype=torch.int64, device=DEV)
    counts = _row_counts(idx, M)
    ref_loss, ref_stats = _check_against_the_fused_kernels(z, tgt, idx, counts, "n = 0")
    assert math.isnan(np.int32(ref_loss).view(np.float32)) and not ref_stats.any()


# ------------------------------------------------------------------------------ the state machine

def _x_for(loss):
    return float("nan") if math.isnan(loss) else math.log(math.expm1(loss))   # log(1 + e^x) = loss


SCRIPTS = {
    # label: (patience, delta, max_epoch, the validation losses aimed at)
    "improve, equal, worse to patience": (3, 0.0, 20, [1.0, 0.8, 0.8, 0.9, 0.95, 0.5, 0.9, 0.9, 0.9, 0.1, 0.1]),
    "delta > 0": (2, 0.05, 20, [1.0, 0.97, 0.90, 0.88, 0.86, 0.2, 0.2]),
    "a NaN becomes best": (2, 0.0, 20, [1.0, float("nan"), 0.5, 2.0, 0.4, 2.0, 2.0, 2.0, 0.1]),
    "NaN first": (1, 0.0, 20, [float("nan"), 0.5, 0.6, 0.7, 0.1]),
    "patience 0": (0, 0.0, 20, [1.0, 0.5, 0.6, 0.1, 0.1]),
    "ends on max_epoch": (10, 0.0, 4, [1.0, 0.9, 0.8, 0.7, 0.6, 0.5]),
    "max_epoch 1": (10, 0.0, 1, [1.0, 0.9, 0.8]),
}


@pytest.mark.parametrize("label", list(SCRIPTS))
def test_state_machine_follows_the_reference_early_stopping(label):
    patience, delta, max_epoch, losses = SCRIPTS[label]
    t = Tail(2, max_epoch, patience, delta)
    py = gcn_ref.EarlyStopping(patience, delta)
    z = torch.zeros(1, 2, device=DEV)
    tgt = torch.zeros(1, dtype=torch.int64, device=DEV)
    tl = torch.zeros(1, device=DEV)
    stopped_at = None
    for e, want in enumerate(losses):
        z[0, 1] = _x_for(want)
        tl[0] = 10.0 + e
        before_state, before_hist = t.state.clone(), t.hist.clone()
        t.launch(z, tgt, None, 1, tl)
        st = t.host_state()
        if stopped_at is not None:   # launches after the stop: nothing at all is written
            assert torch.equal(t.state, before_state) and torch.equal(t.hist, before_hist), f"{label}: epoch {e}"
            continue
        (tl_bits, vl_bits), cnt = t.row(e)
        val_loss = float(np.int32(vl_bits).view(np.float32))
        assert math.isnan(want) == math.isnan(val_loss) and (math.isnan(want) or abs(val_loss - want) < 1e-5)
        assert float(np.int32(tl_bits).view(np.float32)) == 10.0 + e
        assert cnt.sum() == 2 and cnt[-1] in (0, 1)   # one row: a TP and correct, or an FP and an FN
        stop = py(val_loss)                           # utils.py:238-255 on the loss the loop would read
        reason = 1 if stop else (2 if e + 1 == max_epoch else 0)
        print(f"{label}: epoch {e} val loss {val_loss!r}: counter {st.counter} (reference {py.counter}) best "
              f"{st.best!r} (reference {py.best_score!r}) stopped {st.stopped} (reference {reason})")
        assert st.epoch == e + 1 and st.arrivals == 0
        assert st.counter == py.counter
        assert st.best == py.best_score or (math.isnan(st.best) and math.isnan(py.best_score))
        assert st.stopped == reason
        if reason:
            stopped_at = e
            assert st.stop_epoch == e
    assert stopped_at is not None and stopped_at + 2 < len(losses), \
        f"{label}: the script must stop and be followed by two more launches"
    # the rows past stop_epoch are still zero
    assert not t.hist[stopped_at + 1:].any()
    assert t.host_state().epoch == stopped_at + 1
