"""gcnk_score_docs_f32 on the GPU, through ctypes, against the float64
restatement tests/score_ref.py.  Every launch follows one that filled all LDS
with NaN bits; every operand is a strided view inside a NaN-filled allocation."""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

import score_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7
WORST = {}   # shape -> worst |err| / atol seen (printed per case)


def _inside(arr, row0, col0, pad_rows, ld, fill=float("nan")):
    """(buffer, view): `arr` as the view buf[row0 : row0 + rows, col0 : col0 + cols] of a `fill`-filled
    [rows + row0 + pad_rows x ld] device buffer."""
    t = torch.from_numpy(np.atleast_2d(arr))
    rows, cols = t.shape
    buf = torch.full((rows + row0 + pad_rows, ld), fill, dtype=t.dtype, device=DEV)
    view = buf[row0:row0 + rows, col0:col0 + cols]
    view.copy_(t)
    return buf, view


class _Device:
    """One case's operands on the device.  x, a, W1, S_T start 16 bytes into rows of a multiple of 4 floats
    (the kernel's operand form); W2, S2_T, b1, b2 at odd offsets in odd-length rows."""

    def __init__(self, c):
        B, Kc, H, F, P, k0 = self.shape = c["shape"]
        r4 = lambda n: (n + 3) // 4 * 4
        W1 = c["W1"].copy()
        W1[:k0] = np.nan           # rows outside k0 .. k0 + Kc are never read
        W1[k0 + Kc:] = np.nan
        self.keep = []
        for name, arr, col0, ld in (("x", c["x"], 4, r4(Kc) + 8), ("a", c["a"], 4, r4(H) + 12), ("W1", W1, 4, F + 8),
                                    ("S_T", c["S_T"], 4, F + 4), ("W2", c["W2"], 1, P + 3),
                                    ("S2_T", c["S2_T"], 3, P + 4), ("b1", c["b1"], 1, F + 2), ("b2", c["b2"], 1, P + 2),
                                    ("dh", c["dh"], 1, H + 1)):
            buf, view = _inside(arr, 1, col0, 1, ld)
            self.keep.append(buf)
            setattr(self, name, view)
        self.ldo = P + 5

    def launch(self, b1=True, b2=True, labels=True):
        """(out buffer, out view, labels buffer or None) of one launch right after gcnk_debug_poison_lds."""
        B, Kc, H, F, P, k0 = self.shape
        lib = _lib.load()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        obuf = torch.full((B + 2, self.ldo), float("nan"), dtype=torch.float32, device=DEV)
        out = obuf[1:B + 1, 2:2 + P]
        lbuf = torch.full((B + 8,), SENTINEL, dtype=torch.int32, device=DEV) if labels else None
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(lib.gcnk_debug_poison_lds(0xFFFFFFFF, stream), "gcnk_debug_poison_lds")
        _lib.check(lib.gcnk_score_docs_f32(
            B, F, Kc, H, P, k0, p(self.x), self.x.stride(0), p(self.a), self.a.stride(0), p(self.W1),
            self.W1.stride(0), p(self.S_T), self.S_T.stride(0), p(self.W2), self.W2.stride(0), p(self.S2_T),
            self.S2_T.stride(0), p(self.dh), p(self.b1) if b1 else None, p(self.b2) if b2 else None, p(out),
            self.ldo, p(lbuf[4:]) if labels else None, stream), "gcnk_score_docs_f32")
        return obuf, out, lbuf


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _padding_untouched(shape, obuf, lbuf):
    B, P = shape[0], shape[4]
    o = _bits(obuf)
    mask = np.ones(o.shape, bool)
    mask[1:B + 1, 2:2 + P] = False
    assert (o[mask] == _bits(torch.full((1,), float("nan")))[0]).all(), "out padding written"
    if lbuf is not None:
        lab = lbuf.cpu().numpy()
        assert (lab[:4] == SENTINEL).all() and (lab[4 + B:] == SENTINEL).all(), "labels padding written"


def _check(shape, ref, out, lbuf, what):
    """out within atol of the float64 reference; labels its argmax on every decided row.  Returns err / atol."""
    atol = score_ref.atol_of(ref)
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - ref).max())
    decided = score_ref.top2_gap(ref) > 2 * atol
    near = int((~decided).sum())
    print(f"{shape} {what}: max err {err:.3e} = {err / atol:.3f} of atol {atol:.3e}; {near} rows within 2 atol of a tie")
    assert err <= atol, what
    assert near <= shape[0] // 100
    if lbuf is not None:
        lab = lbuf.cpu().numpy()[4:4 + shape[0]].astype(np.int64)
        assert ((lab >= 0) & (lab < shape[4])).all()
        assert np.array_equal(lab[decided], score_ref.labels(ref)[decided]), what
        assert np.array_equal(lab, score_ref.labels(got)), "labels are not the argmax of the launch's own out"
    WORST[shape] = max(WORST.get(shape, 0.0), err / atol)
    return err / atol


@pytest.mark.parametrize("shape", score_ref.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_score_docs_against_float64(shape):
    """Every shape the kernel takes another path at (one document; a partial, a
    full, a just-over block; two n-tiles of P; B staged in chunks; k0 > 0 with
    nothing a multiple of anything; more blocks than a residency round), with a
    row without edges, a row with all H edges and a row of zeros in x: out
    within 2e-5 max(1, max|ref|) of float64, labels its argmax on every decided
    row, b1 / b2 null each and both, the padding of out and labels bitwise
    untouched, a second launch bitwise equal, labels null giving the same out."""
    c = score_ref.make_case(shape)
    d = _Device(c)
    obuf, out, lbuf = d.launch()
    _padding_untouched(shape, obuf, lbuf)
    _check(shape, score_ref.case_ref(c), out, lbuf, "b1 b2")
    obuf2, _, lbuf2 = d.launch()
    assert torch.equal(_bits_t(obuf2), _bits_t(obuf)) and torch.equal(lbuf2, lbuf), "second launch differs"
    obuf3, _, none = d.launch(labels=False)
    assert none is None and torch.equal(_bits_t(obuf3), _bits_t(obuf)), "labels = null changes out"
    for b1, b2 in ((False, True), (True, False), (False, False)):
        ob, o, lb = d.launch(b1, b2)
        _padding_untouched(shape, ob, lb)
        _check(shape, score_ref.case_ref(c, b1, b2), o, lb, f"b1={b1} b2={b2}")
    print(f"{shape}: worst err / atol = {WORST[shape]:.3f}")


def _bits_t(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("row", [17, 32])
def test_nan_in_one_row_of_x_stays_in_that_row(row):
    """A NaN in one document's features: that row of out is NaN and its label
    the first NaN column (th.relu keeps a NaN, class_stats' rule calls it
    maximal); every other row is bitwise what it was."""
    shape = (33, 50, 50, 200, 8, 0)
    c = score_ref.make_case(shape)
    d = _Device(c)
    obuf, out, lbuf = d.launch()
    d.x[row, 7] = float("nan")
    obuf2, out2, lbuf2 = d.launch()
    _padding_untouched(shape, obuf2, lbuf2)
    others = [r for r in range(shape[0]) if r != row]
    assert bool(torch.isnan(out2[row]).all())
    assert int(lbuf2[4 + row]) == 0
    assert torch.equal(_bits_t(out2[others]), _bits_t(out[others]))
    assert torch.equal(lbuf2[4:][others], lbuf[4:][others])
    cn = dict(c, x=d.x.cpu().numpy())
    assert score_ref.labels(score_ref.case_ref(cn))[row] == 0
