"""GPU checks of "keep the parameters of the best epoch" (csrc/keep.hip,
gcnk_keep_best_f32; train.BestKeeper; train.fit(restore_best=True)).

Every comparison is bitwise on int32 views: the feature copies, it computes
nothing, so there is no tolerance anywhere.

  1. the kernel alone, through ctypes: the decision matrix, every size and
     alignment at which it takes another path, padding around every buffer;
  2. behind the real gcnk_epoch_tail_f32 on a one-row logit matrix whose
     validation loss is scripted per epoch (tests/test_epoch_tail.py's
     construction), launch by launch against tests/keep_ref.py's model driven
     by oracle.gcn_ref.EarlyStopping -- eager, and captured once in a hipGraph;
  3. train.fit(restore_best=True) against the loop written by hand that clones
     the parameters whenever oracle.gcn_ref.EarlyStopping improves."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, _lib, datasets, metrics, train

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keep_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CHUNK = _lib.KEEP_CHUNK
NAN_BITS = 0x7FC00000
PAD = 8   # words of padding in front of a buffer: a multiple of 4, so a buffer's offset from a 16-B boundary is `off`


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Buf:
    """`numel` 32-bit words, `off` words past a 16-B boundary, inside a larger NaN-filled allocation."""

    def __init__(self, numel, off, fill=None):
        self.numel, self.lo = numel, PAD + off
        self.back = torch.full((self.lo + numel + PAD + 3,), NAN_BITS, dtype=torch.int32, device=DEV)
        assert self.back.data_ptr() % 16 == 0
        self.view = self.back[self.lo:self.lo + numel]
        if fill is not None:
            self.view.copy_(fill)

    @property
    def ptr(self):
        return self.back.data_ptr() + 4 * self.lo

    def holds(self, words):
        """The buffer holds `words` and its padding is untouched, bit for bit."""
        want = torch.full_like(self.back, NAN_BITS)
        want[self.lo:self.lo + self.numel] = words
        return torch.equal(self.back, want)


SPECIAL = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF,   # NaNs with payloads, a signalling one
                    0x80000000, 0x00000000,                           # -0.0, +0.0
                    0x00000001, 0x807FFFFF, 0x00400000,               # denormals
                    0x7F800000, 0xFF800000], dtype=np.uint32)         # +-inf


def random_bits(rng, n):
    w = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    pick = rng.random(n) < 0.3
    w[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return torch.from_numpy(w.view(np.int32).copy()).to(DEV)


def pattern(n, tag):
    return (torch.arange(n, dtype=torch.int32, device=DEV) & 0xFFFFF) | (tag << 20)


def epoch_state(epoch, counter):
    """A device gcnk_epoch_state written by the host."""
    s = _lib.EpochState()
    s.epoch, s.counter = epoch, counter
    return torch.from_numpy(np.frombuffer(bytes(s), dtype=np.int32).copy()).to(DEV)


def keep(pairs, es, st, flags=0):
    """One gcnk_keep_best_f32 launch over (src Buf, dst Buf) pairs."""
    tab = (_lib.KeepTensor * max(1, len(pairs)))()
    for k, (s, d) in enumerate(pairs):
        assert s.numel == d.numel
        tab[k].src, tab[k].dst, tab[k].numel = s.ptr, d.ptr, s.numel
    _lib.check(_lib.load().gcnk_keep_best_f32(tab, len(pairs), _ptr(es), _ptr(st), flags, _stream()),
               "gcnk_keep_best_f32")
    torch.cuda.synchronize()


def words(st):
    return tuple(st.cpu().tolist())


def decision_matrix(shapes, seed, label):
    """The three cases of the matrix on one launch over `shapes` = [(numel, src offset, dst offset)]:
    (fresh, counter == 1) does not copy, (fresh, counter == 0) copies, (not fresh, counter == 0) -- the same
    launch repeated after src was overwritten -- does not.  The four state words are checked in each."""
    rng = np.random.default_rng(seed)
    first = [random_bits(rng, n) for n, _, _ in shapes]
    src = [Buf(n, so, fill=w) for (n, so, _), w in zip(shapes, first)]
    pat = [pattern(n, 0x5A0 + k) for k, (n, _, _) in enumerate(shapes)]
    dst = [Buf(n, do, fill=p) for (n, _, do), p in zip(shapes, pat)]
    pairs = list(zip(src, dst))
    st = torch.zeros(4, dtype=torch.int32, device=DEV)

    keep(pairs, epoch_state(1, 1), st)                      # an epoch was recorded; it did not improve
    assert all(d.holds(p) for d, p in zip(dst, pat)), f"{label}: a launch that must not copy wrote dst"
    assert words(st) == (1, 0, 0, 0), f"{label}: (fresh, counter 1)"

    keep(pairs, epoch_state(2, 0), st)                      # the next epoch improved
    for k, (s, d, w) in enumerate(zip(src, dst, first)):
        assert s.holds(w), f"{label}: tensor {k}: src changed"
        assert d.holds(w), f"{label}: tensor {k} {shapes[k]}: dst is not src bit for bit, or its padding was written"
    assert words(st) == (2, 2, 0, 1), f"{label}: (fresh, counter 0)"

    for s, (n, _, _) in zip(src, shapes):                   # the parameters move on ...
        s.view.copy_(random_bits(rng, n))
    keep(pairs, epoch_state(2, 0), st)                      # ... and the same launch comes again: nothing new to see
    assert all(d.holds(w) for d, w in zip(dst, first)), f"{label}: a launch that is not fresh wrote dst"
    assert words(st) == (2, 2, 0, 1), f"{label}: (not fresh, counter 0)"


NUMELS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
# both 16-B aligned; both offset by 1, 2, 3 floats (a scalar head of 3, 2, 1); disagreeing offsets (all scalar)
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (3, 2), (2, 0)]


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: f"src+{o[0]},dst+{o[1]}")
def test_kernel_decision_matrix_at_every_size_and_alignment(offs):
    for numel in NUMELS:   # one tensor per launch: numel <= CHUNK at equal offsets is a grid of ONE workgroup
        decision_matrix([(numel, offs[0], offs[1])], seed=100 * numel + 10 * offs[0] + offs[1],
                        label=f"numel={numel} offsets={offs}")


def test_kernel_eight_tensors_over_several_hundred_workgroups():
    # 300 chunks and a ragged tail in the first tensor, an empty tensor in the middle, mixed alignments:
    # 301 + 1 + 0 + 1 + 1 + 3 + 1 + 1 = 309 workgroups in one launch
    shapes = [(300 * CHUNK + 5, 0, 0), (1, 3, 3), (0, 0, 0), (CHUNK, 1, 1), (3, 0, 2), (2 * CHUNK + 7, 2, 1),
              (5, 2, 2), (CHUNK - 1, 0, 0)]
    assert len(shapes) == _lib.KEEP_MAX_TENSORS
    decision_matrix(shapes, seed=7, label="eight tensors")


def test_kernel_nine_tensors_in_two_launches_update_the_state_once():
    rng = np.random.default_rng(9)
    shapes = [(CHUNK + 1, 0, 0), (5, 1, 1), (4, 0, 3), (0, 0, 0), (2 * CHUNK + 7, 3, 3), (1, 0, 0), (3, 2, 2),
              (CHUNK - 1, 1, 0), (CHUNK, 2, 2)]
    first = [random_bits(rng, n) for n, _, _ in shapes]
    src = [Buf(n, so, fill=w) for (n, so, _), w in zip(shapes, first)]
    pat = [pattern(n, 0x600 + k) for k, (n, _, _) in enumerate(shapes)]
    dst = [Buf(n, do, fill=p) for (n, _, do), p in zip(shapes, pat)]
    pairs = list(zip(src, dst))
    es = epoch_state(5, 0)
    st = torch.tensor([4, 3, 0, 2], dtype=torch.int32, device=DEV)   # mid-run: epoch 2 kept, 4 epochs seen
    keep(pairs[:8], es, st, _lib.KEEP_HOLD_STATE)
    assert words(st) == (4, 3, 0, 2), "a HOLD_STATE launch touched the state"
    assert all(d.holds(w) for d, w in zip(dst[:8], first[:8])) and dst[8].holds(pat[8])
    keep(pairs[8:], es, st)
    assert all(d.holds(w) for d, w in zip(dst, first)), "not all nine tensors were copied"
    assert words(st) == (5, 5, 0, 3), "the state must be updated once, by the launch without HOLD_STATE"
    # the same two launches again see nothing fresh
    for s, (n, _, _) in zip(src, shapes):
        s.view.copy_(random_bits(rng, n))
    keep(pairs[:8], es, st, _lib.KEEP_HOLD_STATE)
    keep(pairs[8:], es, st)
    assert all(d.holds(w) for d, w in zip(dst, first)) and words(st) == (5, 5, 0, 3)
    # and a non-improving epoch behind HOLD_STATE copies nothing either
    es = epoch_state(6, 1)
    keep(pairs[:8], es, st, _lib.KEEP_HOLD_STATE)
    keep(pairs[8:], es, st)
    assert all(d.holds(w) for d, w in zip(dst, first)) and words(st) == (6, 5, 0, 3)


def test_kernel_accepts_ranges_that_touch_and_refuses_ranges_that_overlap():
    back = torch.full((64,), NAN_BITS, dtype=torch.int32, device=DEV)
    back[8:12] = pattern(4, 1)
    tab = (_lib.KeepTensor * 1)()
    tab[0].src, tab[0].dst, tab[0].numel = back.data_ptr() + 32, back.data_ptr() + 48, 4   # [8, 12) -> [12, 16)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    _lib.check(lib.gcnk_keep_best_f32(tab, 1, _ptr(epoch_state(1, 0)), _ptr(st), 0, _stream()), "gcnk_keep_best_f32")
    torch.cuda.synchronize()
    want = torch.full((64,), NAN_BITS, dtype=torch.int32, device=DEV)
    want[8:12] = pattern(4, 1)
    want[12:16] = pattern(4, 1)
    assert torch.equal(back, want) and words(st) == (1, 1, 0, 1)
    tab[0].dst = back.data_ptr() + 44   # [11, 15): one word of src
    assert lib.gcnk_keep_best_f32(tab, 1, _ptr(epoch_state(2, 0)), _ptr(st), 0, _stream()) == _lib.EARG
    torch.cuda.synchronize()
    assert torch.equal(back, want) and words(st) == (1, 1, 0, 1)


# ------------------------------------------------------------------------------ behind the real tail

def _x_for(loss):
    return float("nan") if math.isnan(loss) else math.log(math.expm1(loss))   # log(1 + e^x) = loss


class TailAndKeep:
    """gcnk_epoch_tail_f32 on a one-row logit matrix (two classes, label 0: the loss is log(1 + e^x) of the
    second logit) followed by gcnk_keep_best_f32 over two "parameter" buffers, every buffer allocated once."""
    SHAPES = [(5, 1, 1), (CHUNK + 1, 0, 2)]   # a scalar head + 16-B body; disagreeing offsets

    def __init__(self, patience, delta, max_epoch):
        lib = _lib.load()
        self.patience, self.delta, self.max_epoch = patience, delta, max_epoch
        self.state = torch.zeros(8, dtype=torch.int32, device=DEV)
        self.hist = torch.zeros(max_epoch, _lib.epoch_row_words(2), dtype=torch.int32, device=DEV)
        self.nb = lib.gcnk_epoch_tail_workspace_bytes(1, 2)
        assert self.nb > 0
        self.ws = torch.full((self.nb // 8,), float("nan"), dtype=torch.float64, device=DEV)
        self.z = torch.zeros(1, 2, device=DEV)
        self.tgt = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.tl = torch.zeros(1, device=DEV)
        self.src = [Buf(n, so) for n, so, _ in self.SHAPES]
        self.init = [torch.full((n,), -1, dtype=torch.int32, device=DEV) for n, _, _ in self.SHAPES]
        self.dst = [Buf(n, do, fill=w) for (n, _, do), w in zip(self.SHAPES, self.init)]
        self.kst = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.tab = (_lib.KeepTensor * 2)()
        for k, (s, d) in enumerate(zip(self.src, self.dst)):
            self.tab[k].src, self.tab[k].dst, self.tab[k].numel = s.ptr, d.ptr, s.numel

    def params_of(self, e):
        """The parameters as they are before epoch e's tail: a pattern that encodes e."""
        return [pattern(n, 16 * (e + 1) + k) for k, (n, _, _) in enumerate(self.SHAPES)]

    def set_epoch(self, e, loss):
        self.z[0, 1] = _x_for(loss)
        self.tl[0] = 10.0 + e
        for s, w in zip(self.src, self.params_of(e)):
            s.view.copy_(w)

    def pair(self):
        """The tail and, right behind it on the stream, the keep."""
        lib = _lib.load()
        z = self.z
        _lib.check(lib.gcnk_epoch_tail_f32(_ptr(z), z.stride(0), 1, 2, _ptr(self.tgt), None, 1, _ptr(self.tl),
                                           _ptr(self.state), _ptr(self.hist), self.max_epoch, self.patience,
                                           self.delta, _ptr(self.ws), self.nb, _stream()), "gcnk_epoch_tail_f32")
        _lib.check(lib.gcnk_keep_best_f32(self.tab, 2, _ptr(self.state), _ptr(self.kst), 0, _stream()),
                   "gcnk_keep_best_f32")

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.state, self.hist, self.kst, *(d.back for d in self.dst))]

    def host_state(self):
        return _lib.EpochState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def val_loss(self, e):
        return float(self.hist[e, 1:2].cpu().numpy().view(np.float32)[0])


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def run_script(label, launch):
    """The script `label`, pair by pair, held to keep_ref's model; `launch(loop)` issues one tail + keep pair.
    Returns the snapshots after every pair."""
    patience, delta, max_epoch, losses, kept_at_the_end = keep_ref.SCRIPTS[label]
    loop = TailAndKeep(patience, delta, max_epoch)
    py = keep_ref.TracedStopping(patience, delta)
    tail = keep_ref.TailWords(py, max_epoch)
    model = keep_ref.KeepModel()
    shots, stopped_at = [], None
    for e, want in enumerate(losses):
        loop.set_epoch(e, want)
        before = loop.snapshot()
        launch(loop)
        shots.append(loop.snapshot())
        if stopped_at is not None:   # pairs queued past the stop change no byte of state, history, dst or keeper state
            assert same(shots[-1], before), f"{label}: pair {e}, behind the stop at {stopped_at}, wrote something"
            continue
        val_loss = loop.val_loss(e)
        assert math.isnan(want) == math.isnan(val_loss) and (math.isnan(want) or abs(val_loss - want) < 1e-5)
        tail.record(val_loss)   # utils.py:238-255 on the loss the loop would read
        copied = model.look(tail.epoch, tail.counter)
        st = loop.host_state()
        print(f"{label}: epoch {e} val loss {val_loss!r}: counter {st.counter} stopped {st.stopped}; model "
              f"{'copies' if copied else 'does not copy'}, keeps epoch {model.kept}; keeper state {words(loop.kst)}")
        assert (st.epoch, st.counter, st.stopped, st.arrivals) == (tail.epoch, tail.counter, tail.stopped, 0)
        assert model.kept == py.saved[-1]
        for d, w in zip(loop.dst, loop.params_of(model.kept)):
            assert d.holds(w), f"{label}: after epoch {e} dst must hold the parameters of epoch {model.kept}"
        assert words(loop.kst) == model.words == (e + 1, model.kept + 1, 0, len(py.saved))
        if tail.stopped:
            stopped_at = e
    assert stopped_at is not None and len(losses) - 1 - stopped_at == 5
    assert model.kept == kept_at_the_end
    if label.startswith("max_epoch"):
        assert tail.stopped == 2 and model.kept == stopped_at   # copied in the stopping epoch's own launch
    return shots


@pytest.mark.parametrize("label", list(keep_ref.SCRIPTS))
def test_keep_behind_the_real_tail_follows_the_reference_early_stopping(label):
    run_script(label, lambda loop: loop.pair())


@pytest.mark.parametrize("label", ["patience stop after a non-monotone run", "max_epoch on an improving last epoch"])
def test_tail_and_keep_captured_once_and_replayed_give_the_eager_bytes(label):
    eager = run_script(label, lambda loop: loop.pair())   # (also loads both kernels before any capture)
    graphs = {}

    def replay(loop):
        if id(loop) not in graphs:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                loop.pair()
            graphs[id(loop)] = g   # (the capture itself launched nothing)
        graphs[id(loop)].replay()

    replayed = run_script(label, replay)
    assert len(graphs) == 1 and len(eager) == len(replayed)
    for e, (a, b) in enumerate(zip(eager, replayed)):
        assert same(a, b), f"{label}: pair {e}: the replayed bytes differ from the eager ones"
    graphs.clear()


# ------------------------------------------------------------------------------ BestKeeper and fit(restore_best=True)

def test_best_keeper_over_nine_parameters_restores_in_place():
    torch.manual_seed(0)
    params = [torch.randn(n, device=DEV) for n in (5, CHUNK + 3, 1, 7, 4, 2 * CHUNK, 3, 9, 11)]
    log = train.EpochLog(10, 2, DEV, patience=5)
    keeper = train.BestKeeper(params, log)
    assert log.keeper is keeper and keeper.best_epoch is None and log.best_epoch is None
    with pytest.raises(RuntimeError, match="nothing was kept"):
        keeper.restore()
    z = torch.zeros(1, 2, device=DEV)
    tgt = torch.zeros(1, dtype=torch.int64, device=DEV)
    ptrs = [p.data_ptr() for p in params]
    kept = None
    for e, x in enumerate([0.0, -1.0, 1.0, -2.0, 3.0]):   # improves at 0, 1 and 3
        z[0, 1] = x
        log.record(z, tgt, None)
        keeper.keep()
        if e in (0, 1, 3):
            kept = [p.clone() for p in params]
        assert keeper.best_epoch == log.best_epoch == (e if e in (0, 1, 3) else e - 1)
        for p in params:
            p.add_(1.0)
    st = keeper.state()
    assert (st.seen, st.best, st.arrivals, st.copies) == (5, 4, 0, 3)
    assert keeper.restore() == 3
    assert [p.data_ptr() for p in params] == ptrs
    assert all(torch.equal(p.view(torch.int32), k.view(torch.int32)) for p, k in zip(params, kept))
    # what it refuses, in train.Adam's words
    for bad in (torch.randn(4, 6, device=DEV).t(), torch.randn(4, device=DEV, dtype=torch.float64), torch.randn(4)):
        with pytest.raises(RuntimeError, match="contiguous dense fp32"):
            train.BestKeeper([bad], log)


@functools.lru_cache(maxsize=None)
def small():
    """The 310-node graph of tests/test_fit.py, by the same generator call: 300 documents + 10 topics, 60
    features, 4 classes, 200 training and 100 validation documents."""
    g = datasets.doc_topic_graph(300, 10, 4, seed=3, emb_dim=60)
    assert g["nfeat"] == 60 and g["nodes"] == 310
    target = (np.argmax(g["features_dense"][:300, :10], axis=1) % 4).astype(np.int64)
    perm = np.random.default_rng(4).permutation(300)
    return {"features": g["features"].to(DEV), "adj": g["adj"].to(DEV), "target": torch.from_numpy(target).to(DEV),
            "train_idx": torch.from_numpy(perm[:200]).to(DEV), "val_idx": torch.from_numpy(perm[200:]).to(DEV),
            "nfeat": 60, "nclass": 4, "nodes": 310}


def make_model(d, seed, nhid, dropout, rng):
    torch.manual_seed(seed)                                 # trainer.py:295
    np.random.seed(seed)                                    # trainer.py:296
    return GCN(nfeat=d["nfeat"], nhid=nhid, nclass=d["nclass"], dropout=dropout, dropout_rng=rng).to(DEV)


def hand_loop(d, seed, nhid=16, dropout=0.5, rng="device", lr=0.02, max_epoch=200, patience=10):
    """tests/test_fit.py's hand_loop (trainer.py:349-376 on the native loss, optimiser and metrics, one host
    decision per epoch) plus the clone: the parameters are cloned whenever oracle.gcn_ref.EarlyStopping
    assigns best_score, which is where utils.py:244 / :254 would save the checkpoint.
    Returns (history, model, optimiser, cloned parameters, their epoch, the epochs that improved)."""
    model = make_model(d, seed, nhid, dropout, rng)
    opt = train.Adam(model.parameters(), lr=lr)             # trainer.py:308
    crit = train.IndexedCrossEntropy()                      # trainer.py:307
    stopper = keep_ref.TracedStopping(patience)
    history, best = [], None
    for epoch in range(max_epoch):                          # trainer.py:349-376
        model.train()
        opt.zero_grad()
        loss = crit(model(d["features"], d["adj"]), d["target"], d["train_idx"])
        loss.backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            acc, f1, p, r, vl = metrics.evaluate_with_loss(model(d["features"], d["adj"]), d["target"], d["val_idx"],
                                                           d["nclass"])
        history.append({"epoch": epoch, "train_loss": loss.item(), "val_loss": vl, "acc": acc, "macro_f1": f1,
                        "precision": p, "recall": r})
        saved = len(stopper.saved)
        stop = stopper(vl)
        if len(stopper.saved) > saved:                      # utils.py:244, :254 self.save_checkpoint(val_loss, model)
            best = [q.detach().clone() for q in model.parameters()]
        if stop:
            break
    return history, model, opt, best, stopper.saved[-1], list(stopper.saved)


def fit_run(d, seed, nhid=16, dropout=0.5, rng="device", lr=0.02, max_epoch=200, patience=10, **kw):
    model = make_model(d, seed, nhid, dropout, rng)
    res = train.fit(model, d["features"], d["adj"], d["target"], d["train_idx"], d["val_idx"], lr=lr,
                    max_epoch=max_epoch, patience=patience, **kw)
    return res, model


def f64_bits(x):
    return np.float64(x).view(np.int64)


def same_history(a, b):
    return len(a) == len(b) and all(
        ha.keys() == hb.keys() and ha["epoch"] == hb["epoch"] and
        all(f64_bits(ha[k]) == f64_bits(hb[k]) for k in ha if k != "epoch") for ha, hb in zip(a, b))


def same_tensors(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and all(torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))
                                    for x, y in zip(a, b))


def same_moments(ma, oa, mb, ob):
    return oa.steps == ob.steps and all(
        torch.equal(oa.state[pa][k].view(torch.int32), ob.state[pb][k].view(torch.int32))
        for pa, pb in zip(ma.parameters(), mb.parameters()) for k in ("exp_avg", "exp_avg_sq"))


# seed, patience (tests/test_fit.py's SMALL is the starting point): the loop stops on patience inside a group of
# 7 replays, and a non-improving epoch lies before its best epoch
SMALL = dict(seed=11, nhid=16, dropout=0.5, rng="device", lr=0.02, max_epoch=200, patience=3)


@functools.lru_cache(maxsize=None)
def the_loop(max_epoch, patience):
    """The hand-written loop, run twice (it must repeat bitwise), shared by the tests below and left unchanged."""
    hyper = dict(SMALL, max_epoch=max_epoch, patience=patience)
    h1, m1, o1, b1, e1, s1 = hand_loop(small(), **hyper)
    h2, m2, o2, b2, e2, s2 = hand_loop(small(), **hyper)
    assert same_history(h1, h2) and same_tensors(m1.parameters(), m2.parameters()) and same_moments(m1, o1, m2, o2) \
        and same_tensors(b1, b2) and (e1, s1) == (e2, s2), "the hand-written loop does not repeat"
    return h1, m1, o1, b1, e1, s1


@functools.lru_cache(maxsize=None)
def plain_fit(max_epoch, patience, graph, poll_every):
    return fit_run(small(), **dict(SMALL, max_epoch=max_epoch, patience=patience), graph=graph, poll_every=poll_every)


def check_fit(max_epoch, patience, graph, poll_every, label):
    d = small()
    h, m, o, best, best_epoch, improved = the_loop(max_epoch, patience)
    plain, mp = plain_fit(max_epoch, patience, graph, poll_every)
    res, mf = fit_run(d, **dict(SMALL, max_epoch=max_epoch, patience=patience), graph=graph, poll_every=poll_every,
                      restore_best=True)
    keeper = res.log.keeper
    print(f"{label}: loop {len(h)} epochs, improved at {improved}, best epoch {best_epoch}; fit {res.epochs} epochs, "
          f"stop reason {res.stop_reason}, best_epoch {res.log.best_epoch}, keeper state {keeper.state().copies} copies")
    # without the option: no keeper, and the loop's own end state (tests/test_fit.py holds that in full)
    assert plain.log.keeper is None and plain.log.best_epoch is None
    assert same_history(plain.history, h) and same_tensors(mp.parameters(), m.parameters())
    # with it: the parameters are the clone's, the best epoch the loop's
    assert isinstance(keeper, train.BestKeeper)
    assert same_tensors(mf.parameters(), best), f"{label}: the restored parameters are not the loop's clone"
    assert res.log.best_epoch == keeper.best_epoch == best_epoch
    st = keeper.state()
    assert (st.seen, st.best, st.arrivals, st.copies) == (len(h), best_epoch + 1, 0, len(improved))
    # everything else is bitwise fit()'s without the option: history, moments, step count, the log's state
    assert tuple(res)[1:3] == tuple(plain)[1:3] == (len(h), res.stop_reason)
    assert same_history(res.history, plain.history), f"{label}: a history entry differs"
    assert same_moments(mf, res.optimizer, mp, plain.optimizer), f"{label}: a moment or the step count differs"
    assert res.optimizer.steps == len(h)
    assert torch.equal(res.log._state, plain.log._state) and torch.equal(res.log._history, plain.log._history)
    assert not mf.training
    # an eval forward of the restored model gives the best epoch's validation loss, which is the history's minimum
    with torch.no_grad():
        vl = train.cross_entropy(mf(d["features"], d["adj"]), d["target"], d["val_idx"])
    vl_bits = vl.view(torch.int32).item()
    hist_vl = [np.float32(r["val_loss"]) for r in res.history]
    assert all(float(x) == r["val_loss"] for x, r in zip(hist_vl, res.history))   # (fp32 values, held as floats)
    assert vl_bits == int(hist_vl[best_epoch].view(np.int32)), f"{label}: the restored model's validation loss"
    assert hist_vl[best_epoch] == min(hist_vl)   # delta = 0
    return h, res, best_epoch, improved


def test_the_hand_written_loop_is_a_test_that_keep_first_and_keep_every_epoch_fail():
    h, m, o, best, best_epoch, improved = the_loop(SMALL["max_epoch"], SMALL["patience"])
    print(f"loop: {len(h)} epochs, improved at {improved}, best epoch {best_epoch}")
    assert len(h) < SMALL["max_epoch"], "the loop must stop on patience"
    assert (len(h) - 1) % 7 != 0 and len(h) > 8, "the stop must fall inside a group of 7 replays, after a whole group"
    assert best_epoch == len(h) - 1 - SMALL["patience"]
    assert any(e not in improved for e in range(best_epoch)), "a non-improving epoch must lie before the best epoch"
    assert best_epoch > 0 and not same_tensors(best, m.parameters())


@pytest.mark.parametrize("graph,poll_every", [(True, 7), (False, 1)], ids=["graph,poll_every=7", "eager"])
def test_fit_restore_best_is_the_hand_written_loop_s_clone(graph, poll_every):
    h, res, best_epoch, _ = check_fit(SMALL["max_epoch"], SMALL["patience"], graph, poll_every,
                                      "graph" if graph else "eager")
    assert res.stop_reason == 1
    assert best_epoch == res.log.state().stop_epoch - SMALL["patience"]


def test_fit_restore_best_when_max_epoch_ends_the_run_on_its_best_epoch():
    h, res, best_epoch, _ = check_fit(5, 50, True, 7, "max_epoch first")
    assert len(h) == 5 and res.stop_reason == 2
    assert best_epoch == 4, "the best epoch must be the last: it is copied in the stopping epoch's own launch"
