"""The trainer's loss and optimiser on the GPU in three launches (an opt-in swap
outside the module drop-in, like ``metrics``):

  trainer.py:307      criterion = nn.CrossEntropyLoss()     -> IndexedCrossEntropy()
  trainer.py:308      optimizer = th.optim.Adam(...)        -> train.Adam(...)
  trainer.py:358      criterion(logits[idx], target[idx])   -> criterion(logits, target, idx)

``cross_entropy(logits, target, idx)`` is the mean cross-entropy of the rows
``idx`` of ``logits`` with labels ``target`` (indexed like the rows of
``logits``): ``F.cross_entropy(logits[idx], target[idx])`` without the gather
and, in the backward, without the sort + scatter behind ``logits[idx]``.  The
index set is turned once into per-row multiplicities (kept under the
``derived`` rule: same tensor object, same stamp); the forward and the
backward are then dense passes over the rows, with fixed-order float64 sums
(bitwise reproducible).  The gradient is the dense ``dlogits`` the GCN's own
backward takes.

``Adam`` is ``torch.optim.Adam`` (amsgrad=False, maximize=False) with one
launch per 8 tensors of a parameter group and its step count on the device, so
a step captured in a hipGraph advances on every replay.  Checkpoints
interchange with ``torch.optim.Adam`` (``step`` / ``exp_avg`` / ``exp_avg_sq``).

``fit`` is the loop itself (trainer.py:349-376) at replay speed: the epoch's
bookkeeping -- validation loss and class counts, the early-stopping decision,
the history row -- is one launch on the device (``EpochLog``,
gcnk_epoch_tail_f32), the optimiser step is gated by that launch's stop word
(gcnk_adam_gated_f32), and one epoch is captured in a hipGraph and replayed;
the host looks at the stop word once per ``poll_every`` epochs.  With
``restore_best=True`` one more launch per epoch keeps the parameters of the
best epoch on the device (``BestKeeper``, gcnk_keep_best_f32: the checkpoint
utils.py:244 / :254 leave commented out) and ``fit`` ends on those.
"""
import collections

import numpy as np
import torch

from . import _lib, derived
from .sparse import require_device


def _workspace(query, what, device, M, P, ws=None):
    """(float64 workspace, its bytes) for the size ``query(M, P)``; ``ws`` is reused when large enough."""
    nb = query(M, P)
    if nb < 0:
        _lib.check(int(nb), what)
    if ws is None or ws.numel() * 8 < nb:
        ws = torch.empty(max(1, nb // 8), dtype=torch.float64, device=device)
    return ws, nb


class RowCounts:
    """Multiplicities of an index set over M rows: ``counts`` int32 [M + 1] on the
    device (gcnk_ce_row_counts; counts[M], the entries out of range, checked to
    be 0 when built) and ``n`` = len(idx)."""
    __slots__ = ("counts", "n", "pinned")

    def __init__(self, counts, n):
        self.counts, self.n, self.pinned = counts, n, False


_COUNTS = derived.Cache(capacity=16)


def _counts_n(rc, M):
    """(counts pointer, n) of a RowCounts; of every one of M rows once for None."""
    return (rc.counts.data_ptr(), rc.n) if rc is not None else (None, M)


def _build_counts(idx, M, T, device):
    i = idx.to(device=device, dtype=torch.int64).contiguous().view(-1)
    # counted over the T <= M rows that have a label: the rows past them stay 0 (never scored, so their
    # missing labels are never read), and counts[T] collects the entries outside [0, T)
    counts = torch.zeros(M + 1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().gcnk_ce_row_counts(i.data_ptr(), i.numel(), T, counts.data_ptr(), _lib.stream(device)),
                   "gcnk_ce_row_counts")
    bad = int(counts[T].item())   # the one-time synchronising check, like a plan build
    if bad:
        raise IndexError(f"cross_entropy: {bad} of the {i.numel()} entries of idx are outside [0, {T})")
    return RowCounts(counts, i.numel())


def row_counts(idx, M, device, labels=None):
    """The RowCounts of ``idx`` over M rows (of which the first ``labels`` have a
    label: all by default), built on first use of this tensor object with these
    values and reused while it is unchanged (anything but a tensor is
    converted, and so rebuilt, on every call)."""
    if not isinstance(idx, torch.Tensor):
        idx = torch.as_tensor(idx)
    T = M if labels is None else labels
    rc = _COUNTS.get((id(idx), M, T, str(device)), (idx,), _build_counts, idx, M, T, device)
    if not rc.pinned and torch.cuda.is_current_stream_capturing():
        rc.pinned = True   # a captured graph points into counts
    return rc


def _forward(logits, target, rc, want_lse, loss=None):
    """Launch the loss forward on the current stream: (loss [1] fp32, lse [M] or None)."""
    M, P = logits.shape
    dev = logits.device
    lib = _lib.load()
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    if M == 0:
        return loss.fill_(float("nan")), None
    lse = torch.empty(M, dtype=torch.float32, device=dev) if want_lse else None
    ws, nb = _workspace(lib.gcnk_ce_workspace_bytes, "gcnk_ce_workspace_bytes", dev, M, P)
    with torch.cuda.device(dev):
        _lib.check(lib.gcnk_ce_forward_f32(
            logits.data_ptr(), logits.stride(0), M, P, target.data_ptr(), *_counts_n(rc, M),
            loss.data_ptr(), lse.data_ptr() if lse is not None else None, ws.data_ptr(), nb, _lib.stream(dev)),
            "gcnk_ce_forward_f32")
    return loss, lse


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, rc, need):
        loss, lse = _forward(logits, target, rc, need)
        if need:
            ctx.save_for_backward(logits, target, lse)
            ctx.rc = rc
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_out):
        logits, target, lse = ctx.saved_tensors
        rc = ctx.rc
        M, P = logits.shape
        dev = logits.device
        dlogits = torch.empty(M, P, dtype=torch.float32, device=dev)
        if M == 0:
            return dlogits, None, None, None
        g = grad_out.to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gcnk_ce_backward_f32(
                logits.data_ptr(), logits.stride(0), M, P, target.data_ptr(), *_counts_n(rc, M),
                lse.data_ptr(), g.data_ptr(), dlogits.data_ptr(), P, _lib.stream(dev)),
                "gcnk_ce_backward_f32")
        return dlogits, None, None, None


def _prepare(logits, target, idx):
    require_device(logits, "logits")
    if logits.dim() != 2:
        raise ValueError(f"cross_entropy: logits must be [rows x classes] (got {tuple(logits.shape)})")
    if logits.dtype != torch.float32 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        logits = logits.float().contiguous()
    target = target.to(device=logits.device, dtype=torch.int64).contiguous()
    M, T = logits.shape[0], target.numel()
    if T > M or (T < M and idx is None):
        raise ValueError(f"cross_entropy: target has {T} labels for {M} rows of logits (target is indexed like the "
                         "rows of logits, not like idx; it may be shorter only when idx names labelled rows)")
    rc = row_counts(idx, M, logits.device, T) if idx is not None else None
    return logits, target, rc


def cross_entropy(logits, target, idx=None):
    """Mean cross-entropy of the rows ``idx`` (all rows when None; duplicates
    count as often as they occur) of ``logits`` [rows x classes] against
    ``target`` (labels of the rows; as in the reference it may stop short of
    the last rows when ``idx`` names none of those): F.cross_entropy(logits[idx],
    target[idx]) of trainer.py:358, and under no_grad the validation loss of trainer.py:383."""
    logits, target, rc = _prepare(logits, target, idx)
    # lse is kept only when a backward can follow (grad mode is off inside Function.forward: decided here)
    return _CrossEntropyFn.apply(logits, target, rc, torch.is_grad_enabled() and logits.requires_grad)


class IndexedCrossEntropy(torch.nn.Module):
    """nn.CrossEntropyLoss of trainer.py:307 taking the node set as an argument:
    ``criterion(logits, target, idx)`` for ``criterion(logits[idx], target[idx])``."""

    def forward(self, logits, target, idx=None):
        return cross_entropy(logits, target, idx)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) of trainer.py:308 on
    gcnk_adam_f32: one launch per 8 tensors of a parameter group, the step count
    on the device (one word shared by all parameters).
    ``zero_grad_in_step``: the step also zeroes the gradients it read (no
    zero_grad() fills; gradients must then be kept, zero_grad(set_to_none=False),
    or not zeroed by the caller at all).
    ``gate`` (settable): an int32 device word, written earlier on the stream
    (``EpochLog.stop_word``); while it is non-zero a step changes nothing at
    all (gcnk_adam_gated_f32), so steps queued past the stopping epoch are
    no-ops."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, zero_grad_in_step=False,
                 amsgrad=False, maximize=False, foreach=None, fused=None, capturable=None, differentiable=False,
                 gate=None):
        if amsgrad or maximize or differentiable:
            raise ValueError("train.Adam implements amsgrad=False, maximize=False, differentiable=False only")
        if foreach or fused:
            raise ValueError("train.Adam is its own single-launch implementation: foreach / fused do not apply")
        if isinstance(lr, torch.Tensor):
            raise ValueError("train.Adam takes lr as a number")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.zero_grad_in_step = bool(zero_grad_in_step)
        self.gate = gate
        self._step_word = None    # int32 [4] on the device: steps taken, arrival counter, padding
        self._with_grad = None    # ids of the parameters that carried gradients at the first step
        self._tables = _lib.LaunchTables(_lib.AdamTensor, _lib.ADAM_MAX_TENSORS)

    # -- the device step word -------------------------------------------------------------------
    def _word(self, device):
        if self._step_word is None:
            self._step_word = torch.zeros(4, dtype=torch.int32, device=device)
        elif self._step_word.device != device:
            raise RuntimeError("train.Adam: all parameters must be on one device (one shared step word)")
        return self._step_word

    @property
    def steps(self):
        """Steps taken (reads the device word: synchronises)."""
        return 0 if self._step_word is None else int(self._step_word[0].item())

    def _state_of(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            for p in ps:
                require_device(p, "parameter")
                g = p.grad
                if (p.dtype != torch.float32 or g.dtype != torch.float32 or g.layout != torch.strided
                        or not p.is_contiguous() or not g.is_contiguous()):
                    raise RuntimeError("train.Adam: parameters and gradients must be contiguous dense fp32 tensors")
            if ps:
                work.append((gi, group, ps))
        ids = tuple(id(p) for _, _, ps in work for p in ps)
        if self._with_grad is None:
            self._with_grad = ids
        elif ids != self._with_grad:
            raise RuntimeError("train.Adam: the set of parameters that carry gradients changed after the first step "
                               "(they share one step word)")
        if not ids:
            return loss
        dev = work[0][2][0].device
        word = self._word(dev)
        lib = _lib.load()
        zero = _lib.ADAM_ZERO_GRAD if self.zero_grad_in_step else 0
        gate = self.gate
        if gate is not None and (not isinstance(gate, torch.Tensor) or gate.device != dev or gate.dtype != torch.int32
                                 or gate.numel() < 1):
            raise ValueError("train.Adam: gate must be an int32 tensor on the parameters' device")
        with torch.cuda.device(dev):
            stream = _lib.stream(dev)
            li = 0
            for wi, (gi, group, ps) in enumerate(work):   # a launch holds tensors of one group: its coefficients
                ptrs = [(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
                        for p, st in ((p, self._state_of(p)) for p in ps)]
                b1, b2 = group["betas"]
                coef = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
                for tab, n, hold in self._tables.launches(ptrs, [p.numel() for p in ps], li, wi + 1 == len(work)):
                    args = (tab, n, *coef, word.data_ptr(), zero | (_lib.ADAM_HOLD_STEP if hold else 0))
                    if gate is None:
                        _lib.check(lib.gcnk_adam_f32(*args, stream), "gcnk_adam_f32")
                    else:   # every launch of the step, the HOLD_STEP ones included
                        _lib.check(lib.gcnk_adam_gated_f32(*args, gate.data_ptr(), stream), "gcnk_adam_gated_f32")
                    li += 1
        return loss

    # -- checkpoints in torch.optim.Adam's keys -------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        if sd["state"]:   # (the per-parameter dicts are the optimiser's own: copied, not extended)
            t = float(self.steps)
            sd["state"] = {k: dict(st, step=torch.tensor(t, dtype=torch.float32)) for k, st in sd["state"].items()}
        sd["param_groups"] = [dict(g, amsgrad=False, maximize=False, foreach=None, capturable=False,
                                   differentiable=False, fused=None) for g in sd["param_groups"]]
        return sd

    def load_state_dict(self, state_dict):
        steps = {float(st["step"]) for st in state_dict["state"].values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"train.Adam: parameters at different steps {sorted(steps)} (one shared step word)")
        if any(g.get("amsgrad") or g.get("maximize") for g in state_dict["param_groups"]):
            raise ValueError("train.Adam implements amsgrad=False, maximize=False only")
        super().load_state_dict(state_dict)
        keep = set(self.defaults)
        for g in self.param_groups:
            for k in [k for k in g if k not in keep and k != "params"]:
                del g[k]
        dev = None
        for p, st in self.state.items():
            st.pop("step", None)
            for k in ("exp_avg", "exp_avg_sq"):
                st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
            dev = p.device
        self._tables.clear()
        if dev is not None:
            self._word(dev).copy_(torch.tensor([int(steps.pop()) if steps else 0, 0, 0, 0], dtype=torch.int32))


class EpochLog:
    """The per-epoch bookkeeping of trainer.py:372-398 on the device: the state of
    gcnk_epoch_tail_f32 (epoch, early-stopping counter and best score, stop
    reason), the history buffer (``max_epoch`` rows of train loss | validation
    loss | TP | FP | FN | correct) and the launch's workspace.  ``record`` is
    one launch and no host sync; once a stop reason is set, further ``record``
    calls write nothing."""

    def __init__(self, max_epoch, nclass, device, patience=10, delta=0.0):
        if max_epoch < 1 or patience < 0 or not 1 <= nclass <= 1024:
            raise ValueError(f"EpochLog: max_epoch >= 1, patience >= 0, 1 <= nclass <= 1024 "
                             f"(got {max_epoch}, {patience}, {nclass})")
        device = torch.device(device)
        if device.type != "cuda":
            require_device(torch.empty(0, device=device), "EpochLog's device")
        self.max_epoch, self.nclass, self.patience, self.delta = int(max_epoch), int(nclass), int(patience), float(delta)
        self.device = device
        self._state = torch.zeros(8, dtype=torch.int32, device=device)   # gcnk_epoch_state: all-zero is initial
        self._history = torch.zeros(self.max_epoch, _lib.epoch_row_words(self.nclass), dtype=torch.int32, device=device)
        self._ws = None
        self._n = None   # the validation set's size (the metrics' denominator)
        self.graph = None   # fit: the captured epoch (the parameters' .grad live in its memory pool)
        self.keeper = None  # the BestKeeper built on this log (fit(restore_best=True)), if any

    @property
    def best_epoch(self):
        """The keeper's ``best_epoch`` (None without a keeper)."""
        return None if self.keeper is None else self.keeper.best_epoch

    @property
    def stop_word(self):
        """int32 [1] device view of the state's ``stopped`` word: train.Adam's gate."""
        return self._state[1:2]

    def record(self, logits, target, val_idx, train_loss=None):
        """Close an epoch: validation loss and counts of ``logits`` on ``val_idx``,
        ``train_loss`` (a device scalar) copied in, the early-stopping decision
        and the history row -- one launch on the current stream."""
        with torch.no_grad():
            logits, target, rc = _prepare(logits, target, val_idx)
            if logits.device != self.device or logits.shape[1] != self.nclass:
                raise ValueError(f"EpochLog.record: logits [{tuple(logits.shape)}] on {logits.device}, expected "
                                 f"{self.nclass} classes on {self.device}")
            M, P = logits.shape
            counts, n = _counts_n(rc, M)
            if self._n is None:
                self._n = n
            elif self._n != n:
                raise ValueError(f"EpochLog.record: the validation set changed size ({self._n} -> {n})")
            if train_loss is not None:
                require_device(train_loss, "train_loss")
                train_loss = train_loss.detach()
                if train_loss.dtype != torch.float32 or train_loss.numel() != 1:
                    raise ValueError("EpochLog.record: train_loss must be one fp32 value on the device")
            lib = _lib.load()
            self._ws, nb = _workspace(lib.gcnk_epoch_tail_workspace_bytes, "gcnk_epoch_tail_workspace_bytes",
                                      self.device, M, P, self._ws)
            with torch.cuda.device(self.device):
                _lib.check(lib.gcnk_epoch_tail_f32(
                    logits.data_ptr(), logits.stride(0), M, P, target.data_ptr(), counts, n,
                    train_loss.data_ptr() if train_loss is not None else None,
                    self._state.data_ptr(), self._history.data_ptr(), self.max_epoch, self.patience, self.delta,
                    self._ws.data_ptr(), nb, _lib.stream(self.device)), "gcnk_epoch_tail_f32")

    def state(self):
        """The device state as a host _lib.EpochState (one 32-byte copy: synchronises)."""
        return _lib.EpochState.from_buffer_copy(self._state.cpu().numpy().tobytes())

    def poll(self):
        """(epochs recorded, stop reason: 0 running, 1 patience, 2 max_epoch) from
        one small device->host copy."""
        st = self.state()
        return st.epoch, st.stopped

    def history(self, num_classes=None):
        """The list of dicts the reference's loop builds (trainer.py:372-376), one per
        recorded epoch: epoch, train_loss, val_loss, acc, macro_f1, precision,
        recall -- the four metrics from the counts by the reference's numpy
        arithmetic (``num_classes``: utils.py:53-54; by default the model's)."""
        from . import metrics
        epochs, _ = self.poll()
        rows = self._history[:epochs].cpu().numpy()
        P = self.nclass
        out = []
        for e in range(epochs):
            tl, vl = (float(x) for x in rows[e, :2].view(np.float32))
            acc, f1, p, r = metrics._from_counts(rows[e, 2:].astype(np.int64), P,
                                                 P if num_classes is None else num_classes, self._n)
            out.append({"epoch": e, "train_loss": tl, "val_loss": vl, "acc": acc, "macro_f1": f1, "precision": p,
                        "recall": r})
        return out


class BestKeeper:
    """EarlyStopping.save_checkpoint (utils.py:257-262, called -- commented out --
    at utils.py:244 and :254) on the device: one ``best`` buffer per parameter
    and the 16-byte state of gcnk_keep_best_f32.  ``keep()``, queued right after
    ``log.record``, copies the parameters into the buffers if that record
    improved the validation loss and writes nothing otherwise -- one launch per
    8 tensors, no host decision, capturable with the epoch.  One ``keep()`` per
    ``record``.  The buffers are allocated here, before any capture."""

    def __init__(self, params, log):
        self.params = list(params)
        for p in self.params:
            if (not isinstance(p, torch.Tensor) or p.device != log.device or p.dtype != torch.float32
                    or p.layout != torch.strided or not p.is_contiguous()):
                raise RuntimeError("train.BestKeeper: parameters must be contiguous dense fp32 tensors on the "
                                   f"log's device ({log.device})")
        self.log = log
        self.best = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in self.params]
        self._state = torch.zeros(4, dtype=torch.int32, device=log.device)   # gcnk_keep_state: all-zero is initial
        self._tables = _lib.LaunchTables(_lib.KeepTensor, _lib.KEEP_MAX_TENSORS)
        log.keeper = self

    @torch.no_grad()
    def keep(self):
        """The launch (or launches: 8 tensors each, all but the last holding the
        state) on the current stream."""
        lib = _lib.load()
        dev = self.log.device
        ptrs = [(p.data_ptr(), b.data_ptr()) for p, b in zip(self.params, self.best)]
        with torch.cuda.device(dev):
            stream = _lib.stream(dev)
            for tab, n, hold in self._tables.launches(ptrs, [p.numel() for p in self.params]):
                _lib.check(lib.gcnk_keep_best_f32(tab, n, self.log._state.data_ptr(), self._state.data_ptr(),
                                                  _lib.KEEP_HOLD_STATE if hold else 0, stream), "gcnk_keep_best_f32")

    def state(self):
        """The device state as a host _lib.KeepState (one 16-byte copy: synchronises)."""
        return _lib.KeepState.from_buffer_copy(self._state.cpu().numpy().tobytes())

    @property
    def best_epoch(self):
        """The 0-based epoch whose parameters the buffers hold; None while nothing
        is kept (reads the device state: synchronises)."""
        best = self.state().best
        return None if best == 0 else best - 1

    @torch.no_grad()
    def restore(self):
        """Copy the kept parameters back IN PLACE (data pointers stay valid for
        launch records and captured graphs); returns ``best_epoch``."""
        e = self.best_epoch
        if e is None:
            raise RuntimeError("train.BestKeeper: nothing was kept (no keep() has followed an improving record)")
        for p, b in zip(self.params, self.best):
            p.copy_(b)
        return e


FitResult = collections.namedtuple("FitResult", "history epochs stop_reason optimizer log")


def run_epoch(model, features, adj, target, train_idx, val_idx, optimizer, log, criterion=cross_entropy,
              keeper=None):
    """One epoch of trainer.py:354-398 with nothing read back: the training step
    (forward in train mode, loss on ``train_idx``, backward, ``optimizer.step()``),
    the forward in eval mode under no_grad, and ``log.record`` on ``val_idx``
    with the step's loss -- then, with a ``keeper`` (BestKeeper), its ``keep()``.
    Every call is a launch on the current stream, so an
    epoch can be captured in a hipGraph and replayed (the index tensors must be
    the same objects from call to call: their row counts are cached by
    identity).  ``fit`` is this in a loop."""
    model.train()
    optimizer.zero_grad()   # to None, as the reference's call does: no fills, and autograd stores, not adds
    loss = criterion(model(features, adj), target, train_idx)
    loss.backward()
    optimizer.step()
    model.eval()
    with torch.no_grad():
        log.record(model(features, adj), target, val_idx, loss)
        if keeper is not None:
            keeper.keep()


def fit(model, features, adj, target, train_idx, val_idx, *, lr=0.02, max_epoch=200, patience=10, delta=0.0,
        weight_decay=0, poll_every=None, graph=None, restore_best=False):
    """The reference's training loop (trainer.py:349-376) to early stopping:
    Adam(lr, weight_decay) on the mean cross-entropy of ``train_idx``, the
    validation loss and metrics on ``val_idx`` after every epoch,
    EarlyStopping(patience, delta), at most ``max_epoch`` epochs.  Returns
    FitResult(history, epochs, stop_reason, optimizer, log): the history the
    reference prints (``EpochLog.history``), the number of epochs run, why it
    stopped (1: patience, 2: max_epoch), the train.Adam and the EpochLog.

    Nothing is decided on the host.  An epoch is: the training step (forward,
    loss, backward, Adam gated by the log's stop word), the forward in eval
    mode under no_grad, and ``log.record``.  The host queues ``poll_every``
    epochs and then reads the stop word once; the epochs queued past the
    stopping one are no-ops on the parameters, the optimiser's moments and step
    count, the state and the history.

    Graph mode (``graph=True``; the default when the model draws its dropout
    masks on the device, dropout_rng="device", or has dropout 0): epoch 0 runs
    eagerly (a real, counted epoch: plans, launch records and row counts are
    built there), then ONE epoch is captured in a hipGraph -- a single chain on
    one stream -- and replayed, ``poll_every`` (default 16) replays per look.
    Eager mode (``graph=False``; forced for dropout_rng="cpu", whose masks are
    drawn on the host): the same calls per epoch without capture, by default
    ``poll_every=1``, which leaves torch's CPU generator exactly where the
    reference's loop leaves it.  graph=True with CPU masks raises ValueError.

    After ``fit`` returns, the parameters, ``exp_avg``, ``exp_avg_sq`` and the
    optimiser's step count are those of the loop that breaks at the stopping
    epoch, and the model is in eval mode.  The parameters' ``.grad`` and the
    model's mask offset ``_rng_base`` (and with CPU masks and poll_every > 1
    torch's CPU generator) may be those of up to ``poll_every - 1`` gated epochs
    later: the forward and backward of a queued epoch still run, only their
    effect on the model is gated.

    ``restore_best=True``: what EarlyStopping.save_checkpoint (utils.py:257-262)
    was written for and the reference leaves commented out (utils.py:244, :254).
    A BestKeeper is built before epoch 0 and its ``keep()`` follows every
    ``log.record`` (captured with the epoch in graph mode): one more launch per
    epoch, still no host decision.  After the stop the parameters of the epoch
    with the best validation loss (the last one that reset the early-stopping
    counter) are copied back in place; ``result.log.keeper`` is the keeper and
    ``result.log.best_epoch`` that epoch.  Only the parameters go back:
    ``exp_avg``, ``exp_avg_sq`` and the step count stay those of the stopping
    epoch, and so does the history.  With ``restore_best=False`` nothing is
    allocated, launched or changed, and ``result.log.keeper`` is None."""
    require_device(features, "features")
    require_device(adj, "adj")
    params = list(model.parameters())
    if not params:
        raise ValueError("fit: the model has no parameters")
    require_device(params[0], "the model")
    dev = params[0].device
    host_masks = getattr(model, "dropout_rng", "device") == "cpu" and float(getattr(model, "dropout", 0.0)) > 0.0
    if graph is None:
        graph = not host_masks
    elif graph and host_masks:
        raise ValueError("fit: graph=True needs masks drawn on the device (dropout_rng='device') or dropout 0: "
                         "dropout_rng='cpu' draws them on the host every step")
    if poll_every is None:
        poll_every = 16 if graph else 1
    if poll_every < 1:
        raise ValueError(f"fit: poll_every must be >= 1 (got {poll_every})")
    target = torch.as_tensor(target).to(device=dev, dtype=torch.int64).contiguous()
    tr = torch.as_tensor(train_idx).to(device=dev, dtype=torch.int64).contiguous()
    va = torch.as_tensor(val_idx).to(device=dev, dtype=torch.int64).contiguous()
    gc2 = getattr(model, "gc2", None)
    nclass = gc2.out_features if hasattr(gc2, "out_features") else int(target.max().item()) + 1

    log = EpochLog(max_epoch, nclass, dev, patience, delta)
    # the gate is closed by the epoch that stops: every later step is a no-op
    opt = Adam(params, lr=lr, weight_decay=weight_decay, gate=log.stop_word)
    keeper = BestKeeper(params, log) if restore_best else None   # its buffers exist before any capture

    def epoch():
        run_epoch(model, features, adj, target, tr, va, opt, log, keeper=keeper)

    def done():
        epochs, reason = log.poll()
        if keeper is not None:
            keeper.restore()
        return FitResult(log.history(), epochs, reason, opt, log)

    def run(one):   # the host queues poll_every epochs, then looks at the stop word once
        while True:
            for _ in range(poll_every):
                one()
            if log.poll()[1]:
                return done()

    if not graph:
        return run(epoch)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        epoch()   # epoch 0, eager: builds the plans, the launch records and both sets' row counts
    torch.cuda.current_stream(dev).wait_stream(side)
    if log.poll()[1]:   # (max_epoch == 1)
        return done()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        epoch()
    log.graph = g
    return run(g.replay)   # (the capture itself launched nothing: the first replay is epoch 1)
