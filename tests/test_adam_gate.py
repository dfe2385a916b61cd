"""GPU checks of the gated Adam step (csrc/adam.hip, gcnk_adam_gated_f32) on the
tensor mixes of test_native_adam.py, at nine tensors so that a step is two
launches (the first with GCNK_ADAM_HOLD_STEP).

Gate closed (the device word is 1): every buffer and both state words are
bitwise unchanged, with GCNK_ADAM_ZERO_GRAD too.  Gate open (the word is 0) or
absent (NULL): bitwise gcnk_adam_f32's step from the same buffers."""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CHUNK = _lib.ADAM_CHUNK
LR, B1, B2, EPS = 0.02, 0.9, 0.999, 1e-8
NAN_BITS = 0x7FC00000
GUARD = 8
A4 = (0, 0, 0, 0)
# (numel, offsets of p, g, m, v from a 16-B boundary in floats): the seven sizes around the chunk aligned, and
# test_native_adam.py's misaligned mixes (a scalar head then 16-B accesses; buffers that disagree: all scalar)
ALIGNED = [(n, A4) for n in (1, 3, 8, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)] + [(CHUNK + 7, A4), (5, A4)]
MISALIGNED = [(CHUNK + 1, (1, 1, 1, 1)), (2 * CHUNK + 5, (3, 3, 3, 3)), (CHUNK + 1, (0, 1, 0, 3)), (2, (3, 3, 3, 3)),
              (1, A4), (CHUNK, (2, 2, 2, 2)), (CHUNK + 7, (1, 1, 1, 1)), (5, (0, 0, 1, 0)), (2 * CHUNK + 5, A4)]
MIXES = {"aligned": ALIGNED, "misaligned": MISALIGNED}


def _hosts(specs, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n, _ in specs:
        p, g, m = (rng.normal(0, 1, n).astype(np.float32) for _ in range(3))
        v = (rng.normal(0, 1, n) ** 2).astype(np.float32)
        out.append((p, g, m, v))
    return out


class Buf:
    """A device fp32 buffer `off` floats past a 16-B boundary between NaN guards."""

    def __init__(self, host, off):
        n = host.size
        self.back = torch.full((GUARD + off + n + GUARD + 3,), float("nan"), device=DEV)
        self.lo = GUARD + off
        self.t = self.back[self.lo:self.lo + n]
        self.t.copy_(torch.from_numpy(host))
        assert self.back.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * (off % 4)

    def bits(self):
        return self.back.view(torch.int32).cpu().numpy()   # the guards included


def _step(specs, hosts, t, wd, flags, gate):
    """One optimiser step over nine tensors (two launches) from fresh buffers: (bits of every buffer, state)."""
    assert len(specs) == 9
    lib = _lib.load()
    bufs = [tuple(Buf(h, o) for h, o in zip(host, offs)) for host, (_, offs) in zip(hosts, specs)]
    state = torch.tensor([t - 1, 0, 0, 0], dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    groups = [bufs[:8], bufs[8:]]
    for k, grp in enumerate(groups):
        tab = (_lib.AdamTensor * len(grp))()
        for i, (p, g, m, v) in enumerate(grp):
            tab[i].p, tab[i].g, tab[i].m, tab[i].v = (x.t.data_ptr() for x in (p, g, m, v))
            tab[i].numel = p.t.numel()
        fl = flags | (_lib.ADAM_HOLD_STEP if k == 0 else 0)
        args = (tab, len(grp), LR, B1, B2, EPS, wd, ctypes.c_void_p(state.data_ptr()), fl)
        if gate == "plain":
            _lib.check(lib.gcnk_adam_f32(*args, stream), "gcnk_adam_f32")
        else:
            g = ctypes.c_void_p(gate.data_ptr()) if gate is not None else None
            _lib.check(lib.gcnk_adam_gated_f32(*args, g, stream), "gcnk_adam_gated_f32")
    torch.cuda.synchronize()
    return [[b.bits() for b in quad] for quad in bufs], state.tolist()


def _same(a, b):
    return all(np.array_equal(x, y) for qa, qb in zip(a, b) for x, y in zip(qa, qb))


@pytest.mark.parametrize("flags", [0, _lib.ADAM_ZERO_GRAD], ids=["keep_grad", "zero_grad"])
@pytest.mark.parametrize("t,wd", [(1, 0.0), (10, 0.01)])
@pytest.mark.parametrize("mix", list(MIXES))
def test_gate(mix, t, wd, flags):
    specs = MIXES[mix]
    hosts = _hosts(specs, seed=31 * t + len(mix))
    plain, plain_state = _step(specs, hosts, t, wd, flags, "plain")
    assert plain_state == [t, 0, 0, 0]

    # what "unchanged" means: the buffers as they were put on the device
    untouched = [[b.bits() for b in (Buf(h, o) for h, o in zip(host, offs))] for host, (_, offs) in zip(hosts, specs)]
    assert not _same(plain, untouched)

    closed = torch.tensor([1], dtype=torch.int32, device=DEV)
    got, state = _step(specs, hosts, t, wd, flags, closed)
    assert state == [t - 1, 0, 0, 0], f"gate closed: step word / arrival counter {state}"
    assert _same(got, untouched), "gate closed: a parameter, gradient, moment or guard was written"
    assert closed.tolist() == [1]

    for label, gate in (("open", torch.tensor([0], dtype=torch.int32, device=DEV)), ("NULL", None)):
        got, state = _step(specs, hosts, t, wd, flags, gate)
        assert state == [t, 0, 0, 0], f"gate {label}: step word / arrival counter {state}"
        assert _same(got, plain), f"gate {label}: not bitwise gcnk_adam_f32's step"
    if flags & _lib.ADAM_ZERO_GRAD:
        for quad, (n, offs) in zip(plain, specs):
            lo = GUARD + offs[1]
            assert not quad[1][lo:lo + n].any()


def test_optimizer_passes_its_gate_to_every_launch():
    """train.Adam with nine tensors (two launches): closed, a step changes nothing; opened again by a
    store to the same device word, the next step is the ungated optimiser's."""
    rng = np.random.default_rng(5)
    shapes = [(5,), (CHUNK + 3,), (7, 9), (1,), (40, 8), (3,), (2, 2), (11,), (6,)]
    host = [rng.normal(0, 1, s).astype(np.float32) for s in shapes]
    grads = [rng.normal(0, 1, s).astype(np.float32) for s in shapes]

    def mk(gate):
        ps = [torch.nn.Parameter(torch.from_numpy(h.copy()).to(DEV)) for h in host]
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g.copy()).to(DEV)
        return ps, train.Adam(ps, lr=LR, weight_decay=0.01, gate=gate)

    gate = torch.ones(1, dtype=torch.int32, device=DEV)
    ps, opt = mk(gate)
    opt.step()
    assert opt.steps == 0 and opt._step_word.tolist() == [0, 0, 0, 0]
    assert all(torch.equal(p.detach().cpu(), torch.from_numpy(h)) for p, h in zip(ps, host))
    assert all(not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any() for p in ps)
    gate.zero_()
    opt.step()
    qs, ref = mk(None)
    ref.step()
    assert opt.steps == ref.steps == 1
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k].view(torch.int32), ref.state[q][k].view(torch.int32))
    with pytest.raises(ValueError, match="gate"):
        bad = train.Adam(qs, lr=LR, gate=torch.zeros(1, dtype=torch.int64, device=DEV))
        bad.step()
