"""GPU checks of the native Adam step (csrc/adam.hip, gcnk_adam_f32) and of
train.Adam on top of it, against the float64 restatement tests/train_ref.py.

Closeness is measured against the reference trainer's own optimiser, not fixed:
with p'64 the float64 step from a given fp32 state,
    E(x) = max_elem |x - p'64| / (ulp32(|p'64|) + ulp32(lr))
is taken for the kernel and for torch.optim.Adam on the CPU in fp32 from the
same state (state['step'] = t - 1), and E(kernel) <= 2 * E(torch) is required:
the margin covers the roundings the kernel may place differently (a contracted
multiply-add where torch rounds the product first), each about one rounding of
an update of size lr.  m' and v' are held the same way."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, train

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CHUNK = _lib.ADAM_CHUNK
LR, B1, B2, EPS = 0.02, 0.9, 0.999, 1e-8
SIZES = (1, 3, 8, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
NAN_BITS = 0x7FC00000
GUARD = 8   # NaN guard floats on either side of a buffer


def test_chunk_constant_is_the_header_s():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcnk.h")) as f:
        src = f.read()
    assert f"#define GCNK_ADAM_CHUNK {CHUNK}\n" in src and f"#define GCNK_ADAM_MAX_TENSORS {_lib.ADAM_MAX_TENSORS}\n" in src
    assert "#define GCNK_ADAM_ZERO_GRAD 1\n" in src and "#define GCNK_ADAM_HOLD_STEP 2\n" in src


@functools.lru_cache(maxsize=None)
def _state(numel, t, wd, seed, gscale=1.0, zeros=False):
    """fp32 (p, m, v) after t - 1 float64 steps on random gradients, and the gradient of step t."""
    rng = np.random.default_rng(seed)
    p, m, v = rng.normal(0, 1, numel), np.zeros(numel), np.zeros(numel)

    def grad():
        g = gscale * rng.normal(0, 1, numel)
        if zeros:
            g[rng.random(numel) < 0.2] = 0.0
        return g.astype(np.float32).astype(np.float64)

    for s in range(1, t):
        p, m, v = train_ref.adam_step(p, grad(), m, v, s, LR, B1, B2, EPS, wd)
    out = tuple(x.astype(np.float32) for x in (p, grad(), m, v))
    for x in out:
        x.setflags(write=False)
    return out


class Buf:
    """A device fp32 buffer `off` floats past a 16-B boundary between NaN guards."""

    def __init__(self, host, off):
        n = host.size
        self.back = torch.full((GUARD + off + n + GUARD + 3,), float("nan"), device=DEV)
        assert self.back.data_ptr() % 16 == 0
        self.lo = GUARD + off
        self.t = self.back[self.lo:self.lo + n]
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
        assert self.t.data_ptr() % 16 == 4 * (off % 4)

    def guards_intact(self):
        b = self.back.view(torch.int32)
        return bool((b[:self.lo] == NAN_BITS).all()) and bool((b[self.lo + self.t.numel():] == NAN_BITS).all())


def _call(bufs, state, wd, flags=0):
    """One optimiser step over `bufs` = [(p, g, m, v) Bufs]: a call per 8 tensors, the step held until the last."""
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    groups = [bufs[i:i + 8] for i in range(0, len(bufs), 8)]
    for k, grp in enumerate(groups):
        tab = (_lib.AdamTensor * len(grp))()
        for i, (p, g, m, v) in enumerate(grp):
            tab[i].p, tab[i].g, tab[i].m, tab[i].v = (x.t.data_ptr() for x in (p, g, m, v))
            tab[i].numel = p.t.numel()
        hold = _lib.ADAM_HOLD_STEP if k + 1 < len(groups) else 0
        _lib.check(lib.gcnk_adam_f32(tab, len(grp), LR, B1, B2, EPS, wd, ctypes.c_void_p(state.data_ptr()),
                                     flags | hold, stream), "gcnk_adam_f32")


def _torch_cpu_step(p, g, m, v, t, wd):
    """The reference trainer's optimiser (trainer.py:308) on the CPU in fp32, from the given state."""
    q = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([q], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()),
                    "exp_avg_sq": torch.from_numpy(v.copy())}
    q.grad = torch.from_numpy(g.copy())
    opt.step()
    st = opt.state[q]
    assert float(st["step"]) == t
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _E(x, ref):
    return float(np.max(np.abs(x.astype(np.float64) - ref) / (train_ref.ulp32(ref) + train_ref.ulp32(LR))))


def _run_case(label, specs, t, wd, flags=0):
    """specs: [(numel, (off_p, off_g, off_m, off_v), state kwargs)].  Runs step t on the GPU twice from
    identical buffers and holds it to the float64 step and to torch's CPU fp32 step."""
    hosts = [_state(n, t, wd, 17 * i + n % 1000, **kw) for i, (n, _, kw) in enumerate(specs)]

    def device_run():
        bufs = [tuple(Buf(h, o) for h, o in zip(host, offs)) for host, (_, offs, _) in zip(hosts, specs)]
        state = torch.tensor([t - 1, 0, 0, 0], dtype=torch.int32, device=DEV)
        _call(bufs, state, wd, flags)
        torch.cuda.synchronize()
        assert state.tolist() == [t, 0, 0, 0], f"{label}: step word / counter {state.tolist()}"
        for quad in bufs:
            for b in quad:
                assert b.guards_intact(), f"{label}: a guard element was written"
        return [tuple(b.t.cpu().numpy() for b in quad) for quad in bufs]

    got = device_run()
    again = device_run()
    Ek, Et = {"p": 0.0, "m": 0.0, "v": 0.0}, {"p": 0.0, "m": 0.0, "v": 0.0}
    for (p, g, m, v), (pk, gk, mk, vk), (pa, ga, ma, va) in zip(hosts, got, again):
        for a, b in ((pk, pa), (gk, ga), (mk, ma), (vk, va)):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{label}: a second call differs"
        if flags & _lib.ADAM_ZERO_GRAD:
            assert not gk.view(np.int32).any(), f"{label}: g must be +0.0 after GCNK_ADAM_ZERO_GRAD"
        else:
            assert np.array_equal(gk.view(np.int32), g.view(np.int32)), f"{label}: g changed"
        ref = train_ref.adam_step(p, g, m, v, t, LR, B1, B2, EPS, wd)
        tor = _torch_cpu_step(p, g, m, v, t, wd)
        for key, r, xk, xt in zip("pmv", ref, (pk, mk, vk), tor):
            Ek[key], Et[key] = max(Ek[key], _E(xk, r)), max(Et[key], _E(xt, r))
    print(f"{label}: " + "  ".join(f"E_{k}(kernel) {Ek[k]:.4g} E_{k}(torch) {Et[k]:.4g}" for k in "pmv"))
    for k in "pmv":
        assert Ek[k] <= 2 * Et[k], f"{label}: E_{k}(kernel) {Ek[k]:.4g} > 2 * E_{k}(torch) {Et[k]:.4g}"


A4 = (0, 0, 0, 0)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_single_step_every_size_in_one_call(t, wd):
    """The seven sizes around the chunk (scalar tiny tensors, ragged tails, more than one workgroup)."""
    _run_case(f"sizes t={t} wd={wd}", [(n, A4, {}) for n in SIZES], t, wd)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_single_step_four_tensors_misaligned(t, wd):
    """Four tensors in one call: buffers one and three floats past a 16-B boundary (scalar head, then
    16-B accesses), buffers that disagree (all scalar), aligned ones; and the gradients zeroed in the step."""
    specs = [(CHUNK + 1, (1, 1, 1, 1), {}), (2 * CHUNK + 5, (3, 3, 3, 3), {}), (CHUNK + 1, (0, 1, 0, 3), {}),
             (2, (3, 3, 3, 3), {})]
    _run_case(f"four t={t} wd={wd}", specs, t, wd)
    _run_case(f"four zero_grad t={t} wd={wd}", specs, t, wd, flags=_lib.ADAM_ZERO_GRAD)


@pytest.mark.parametrize("t,wd", [(1, 0.0), (10, 0.01)])
def test_single_step_nine_tensors_take_a_second_launch(t, wd):
    specs = [(n, A4, {}) for n in SIZES] + [(CHUNK + 7, (1, 1, 1, 1), {}), (5, A4, {})]
    _run_case(f"nine t={t} wd={wd}", specs, t, wd)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 2, 10])
def test_single_step_tiny_gradients_see_eps(t, wd):
    """Gradients of 1e-7 * N(0, 1) with exact zeros: sqrt(v') is of eps's size, so a missing eps
    (or one added inside the root) moves the update by a large factor."""
    _run_case(f"tiny t={t} wd={wd}", [(CHUNK + 1, A4, {"gscale": 1e-7, "zeros": True})], t, wd)


def test_empty_tensors_and_an_empty_call():
    """numel == 0 tensors are skipped; a call of only such tensors still advances the step."""
    lib = _lib.load()
    state = torch.tensor([4, 0, 0, 0], dtype=torch.int32, device=DEV)
    tab = (_lib.AdamTensor * 2)()
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    args = (LR, B1, B2, EPS, 0.0, ctypes.c_void_p(state.data_ptr()))
    _lib.check(lib.gcnk_adam_f32(tab, 2, *args, 0, stream), "gcnk_adam_f32")
    assert state.tolist() == [5, 0, 0, 0]
    _lib.check(lib.gcnk_adam_f32(tab, 2, *args, _lib.ADAM_HOLD_STEP, stream), "gcnk_adam_f32")
    _lib.check(lib.gcnk_adam_f32(tab, 0, *args, 0, stream), "gcnk_adam_f32")
    assert state.tolist() == [5, 0, 0, 0]


# ------------------------------------------------------------------------------ train.Adam

def _loss_step(z, opt, crit, tgt, idx):
    if not opt.zero_grad_in_step:
        opt.zero_grad(set_to_none=False)
    loss = crit(z, tgt, idx)
    loss.backward()
    opt.step()


@pytest.mark.parametrize("zero_in_step", [False, True])
def test_replayed_step_is_bitwise_the_eager_steps(zero_in_step):
    """A leaf logits parameter [257 x 8], the native loss on an index set, backward, the native Adam:
    one eager warm-up step, one such step captured (a capture runs nothing) and replayed 4 times, against
    1 + 4 eager steps from the same start -- parameters, m, v bitwise, the device step word 5.  The
    captured launch's arguments are frozen: only a step word on the device can advance under replay."""
    rng = np.random.default_rng(77)
    M, P, replays = 257, 8, 4
    z0 = torch.from_numpy(rng.normal(0, 2, (M, P)).astype(np.float32)).to(DEV)
    tgt = torch.from_numpy(rng.integers(0, P, M).astype(np.int64)).to(DEV)
    idx = torch.from_numpy(np.concatenate([rng.choice(M, 90, replace=False), [7, 7, 7]])).to(DEV)
    crit = train.IndexedCrossEntropy()

    def fresh():
        z = torch.nn.Parameter(z0.clone())
        return z, train.Adam([z], lr=LR, weight_decay=0.01, zero_grad_in_step=zero_in_step)

    z_e, opt_e = fresh()
    for _ in range(1 + replays):
        _loss_step(z_e, opt_e, crit, tgt, idx)
    torch.cuda.synchronize()

    z_g, opt_g = fresh()
    _loss_step(z_g, opt_g, crit, tgt, idx)         # warm-up: builds the multiplicities, the state, .grad
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _loss_step(z_g, opt_g, crit, tgt, idx)
    assert opt_g.steps == 1
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    assert opt_g.steps == opt_e.steps == 1 + replays
    assert opt_g._step_word.tolist() == [1 + replays, 0, 0, 0]
    assert not torch.equal(z_g, z0)
    assert torch.equal(z_g.detach().view(torch.int32), z_e.detach().view(torch.int32))
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(opt_g.state[z_g][k].view(torch.int32), opt_e.state[z_e][k].view(torch.int32)), k
    del g


def test_optimizer_matches_torch_over_steps_and_refuses_a_changed_gradient_set():
    """train.Adam against torch.optim.Adam (CPU fp32) over 5 steps on two parameter groups with their
    own hyper-parameters and nine tensors in the first (two launches)."""
    rng = np.random.default_rng(3)
    shapes = [(5,), (CHUNK + 3,), (7, 9), (1,), (40, 8), (3,), (2, 2), (11,), (6,), (300, 8)]
    host = [rng.normal(0, 1, s).astype(np.float32) for s in shapes]
    pn = [torch.nn.Parameter(torch.from_numpy(h.copy()).to(DEV)) for h in host]
    pt = [torch.nn.Parameter(torch.from_numpy(h.copy())) for h in host]
    groups = lambda ps: [{"params": ps[:9]}, {"params": ps[9:], "lr": 0.005, "weight_decay": 0.01}]  # noqa: E731
    on, ot = train.Adam(groups(pn), lr=LR), torch.optim.Adam(groups(pt), lr=LR)
    for step in range(5):
        for a, b in zip(pn, pt):
            g = rng.normal(0, 1, tuple(b.shape)).astype(np.float32)
            a.grad, b.grad = torch.from_numpy(g.copy()).to(DEV), torch.from_numpy(g.copy())
        on.step()
        ot.step()
    assert on.steps == 5
    for a, b in zip(pn, pt):
        # per step torch's fp32 update stays within E = 12.5 units of ulp32(p) + ulp32(lr) of the float64 step
        # (the figure the closeness rule is set against) and the kernel within twice that (the tests above),
        # so two 5-step trajectories part by at most 5 * (12.5 + 25) units; a wrong group's lr or weight
        # decay, or a tensor missed by the second launch, moves a parameter by 1e-3 and more
        bn = b.detach().numpy()
        unit = float(train_ref.ulp32(np.abs(bn).max()) + train_ref.ulp32(LR))
        assert np.abs(a.detach().cpu().numpy() - bn).max() <= 5 * 37.5 * unit
    pn[0].grad = None
    with pytest.raises(RuntimeError, match="set of parameters"):
        on.step()


def test_state_dict_round_trip_with_torch_adam():
    """3 native steps, the state loaded into torch.optim.Adam; and the reverse.  One further step of
    each is held to the float64 step by the closeness rule of this file."""
    rng = np.random.default_rng(11)
    shapes = [(CHUNK + 9,), (33, 8)]
    host = [rng.normal(0, 1, s).astype(np.float32) for s in shapes]
    grads = [[rng.normal(0, 1, s).astype(np.float32) for s in shapes] for _ in range(4)]
    wd = 0.01

    def steps(opt, params, dev, which):
        for k in which:
            for p, g in zip(params, grads[k]):
                p.grad = torch.from_numpy(g.copy()).to(dev)
            opt.step()

    def mk(dev, cls):
        ps = [torch.nn.Parameter(torch.from_numpy(h.copy()).to(dev)) for h in host]
        return ps, cls(ps, lr=LR, weight_decay=wd)

    def E_of(ps, ref_state):
        worst = 0.0
        for p, (p3, m3, v3), g in zip(ps, ref_state, grads[3]):
            ref = train_ref.adam_step(p3, g, m3, v3, 4, LR, B1, B2, EPS, wd)[0]
            worst = max(worst, _E(p.detach().cpu().numpy(), ref))
        return worst

    for src_cls, src_dev, dst_cls, dst_dev in ((train.Adam, DEV, torch.optim.Adam, "cpu"),
                                               (torch.optim.Adam, "cpu", train.Adam, DEV)):
        ps, opt = mk(src_dev, src_cls)
        steps(opt, ps, src_dev, range(3))
        sd = opt.state_dict()
        assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and float(sd["state"][1]["step"]) == 3
        after3 = [(p.detach().cpu().numpy().copy(), opt.state[p]["exp_avg"].cpu().numpy().copy(),
                   opt.state[p]["exp_avg_sq"].cpu().numpy().copy()) for p in ps]
        qs, opt2 = mk(dst_dev, dst_cls)
        with torch.no_grad():
            for q, p in zip(qs, ps):
                q.copy_(p.detach().to(dst_dev))
        opt2.load_state_dict(sd)
        steps(opt, ps, src_dev, [3])
        steps(opt2, qs, dst_dev, [3])
        E_src, E_dst = E_of(ps, after3), E_of(qs, after3)
        E_native, E_torch = (E_src, E_dst) if src_cls is train.Adam else (E_dst, E_src)
        print(f"{src_cls.__module__}.Adam -> {dst_cls.__module__}.Adam: step 4 E(native) {E_native:.4g} "
              f"E(torch) {E_torch:.4g}")
        assert E_native <= 2 * E_torch
        native = opt if src_cls is train.Adam else opt2
        assert native.steps == 4 and "step" not in native.state[native.param_groups[0]["params"][0]]

    # one shared step word: a checkpoint whose parameters are at different steps is refused
    ps, opt = mk(DEV, train.Adam)
    steps(opt, ps, DEV, range(2))
    sd = opt.state_dict()
    sd["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="different steps"):
        mk(DEV, train.Adam)[1].load_state_dict(sd)
