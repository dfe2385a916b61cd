"""Python model of gcnk_keep_best_f32's rule (include/gcnk.h: fresh, copy, the
state update), of the two words gcnk_epoch_tail_f32 leaves for it, and the
scripted validation-loss sequences tests/test_keep_abi.py (CPU) and
tests/test_keep_best.py (GPU) both run.

The yardstick is the reference's own object: oracle.gcn_ref.EarlyStopping
(utils.py:216-255).  ``TracedStopping`` is that class with its ``best_score``
attribute observed, so the epochs at which it took a ``best_score = score``
branch -- utils.py:244 and :254, where save_checkpoint is called (commented
out) -- are recorded by the assignment itself, not re-derived from the rule."""
from oracle import gcn_ref

NAN = float("nan")
EXTRA = [0.01] * 5   # launches queued past the stop: losses that WOULD improve, were anything still decided

SCRIPTS = {
    # label: (patience, delta, max_epoch, validation losses aimed at, the epoch kept at the end)
    "strictly improving, then worse to patience": (3, 0.0, 20, [1.0, 0.9, 0.8, 0.7, 0.6, 0.65, 0.66, 0.67] + EXTRA, 4),
    "an equal loss keeps": (3, 0.0, 20, [1.0, 0.8, 0.8, 0.9, 0.8, 0.95, 0.96, 0.97] + EXTRA, 4),
    "delta > 0": (2, 0.05, 20, [1.0, 0.97, 0.90, 0.88, 0.86] + EXTRA, 2),
    "a NaN loss keeps": (2, 0.0, 20, [1.0, NAN, 0.5, 2.0, 0.4, 2.0, 2.0] + EXTRA, 4),
    "patience 0": (0, 0.0, 20, [1.0, 0.5, 0.6] + EXTRA, 1),
    "patience stop after a non-monotone run": (3, 0.0, 20, [1.0, 0.8, 0.9, 0.95, 0.5, 0.9, 0.6, 0.4, 0.9, 0.9, 0.9]
                                               + EXTRA, 7),
    "max_epoch on an improving last epoch": (10, 0.0, 4, [1.0, 0.9, 0.95, 0.7] + EXTRA, 3),
}


class TracedStopping(gcn_ref.EarlyStopping):
    """oracle.gcn_ref.EarlyStopping; ``saved`` lists the calls (0-based epochs) that assigned best_score."""

    def __init__(self, patience=7, delta=0.0):
        self.saved, self._calls, self._best = [], 0, None
        super().__init__(patience, delta)

    @property
    def best_score(self):
        return self._best

    @best_score.setter
    def best_score(self, value):
        self._best = value
        if value is not None:   # (the constructor's None is no checkpoint)
            self.saved.append(self._calls)

    def __call__(self, val_loss):
        stop = super().__call__(val_loss)
        self._calls += 1
        return stop


class TailWords:
    """The words of gcnk_epoch_state that gcnk_keep_best_f32 reads, as gcnk_epoch_tail_f32 leaves them
    when the loop's EarlyStopping is ``stopper``: once stopped, a record writes nothing."""

    def __init__(self, stopper, max_epoch):
        self.stopper, self.max_epoch = stopper, max_epoch
        self.epoch = self.counter = self.stopped = 0

    def record(self, val_loss):
        if self.stopped or self.epoch >= self.max_epoch:
            return
        stop = self.stopper(val_loss)
        self.counter = self.stopper.counter
        self.epoch += 1
        self.stopped = 1 if stop else (2 if self.epoch == self.max_epoch else 0)


class KeepModel:
    """gcnk_keep_state and the decision of one keep (all its launches) after one tail."""

    def __init__(self):
        self.seen = self.best = self.arrivals = self.copies = 0

    def look(self, epoch, counter, hold=False):
        """One launch: returns whether it copies; updates the state unless ``hold``."""
        fresh = epoch > self.seen
        copy = fresh and counter == 0
        if not hold:
            self.seen = epoch
            if copy:
                self.best = epoch
                self.copies += 1
        return copy

    @property
    def words(self):
        return (self.seen, self.best, self.arrivals, self.copies)

    @property
    def kept(self):
        return None if self.best == 0 else self.best - 1
