"""The case table of the narrow-feature gc1 kernel (test infrastructure, no GPU import).

gcnk_dense_gc1_f32 launches one of 18 instantiations dense_gc1_kernel<KS, NI,
NPM, PV> (csrc/dense_gc1.hip).  Each Case below names the route it is meant to
reach, as gcnk_dense_gc1_route (include/gcnk.h) reports it: (KS, NI, NPM, PV,
tail, ntiles).  tests/test_dense_gc1_routes.py checks on the CPU that every
case reaches the route it names and that the table reaches every entry of
INSTANTIATIONS and both sides of every cut, and on the GPU runs every case by
bits against float64.

The cuts, as dense_gc1_route (csrc/dense_gc1.hip) makes them:
  KS   = the smallest of 8 / 13 / 16 / 25 / 32 with K <= 4 KS
  NI   = 3 while KS <= 25, F <= 208 and P <= 20, else 4
  NPM  = 2 on NI = 4 past P = 16, else 1;  PV = 4 on NI = 3 past P = 16, else 0
  tail = NI = 3 and F > 192: columns 192 .. 207 are one n-tile that moves from
         wave to wave; the wave of a workgroup's first tile is
         (blockIdx / 8 + blockIdx / 256) & 3, so M = 515 (33 tiles, workgroups
         0 .. 32) starts it on every wave
Inside an instantiation: a lane of NI = 3 whose three columns straddle F reads
the row's last three and shifts them down (F % 3 = 1: shift 2, F % 3 = 2:
shift 1); one wave of NI = 3 holds 48 columns, of NI = 4 64; K % 4 != 0 leaves
the last k-step's upper quadrants to the `k < K` mask.

Every operand of a case is strided: ldax = K + 1 ("odd": the entry asks no
alignment of AX) or roundup4(K) + 4 ("r4"), ldw1 = F + 4, ldw2 = P + 3,
ldh = F + 4, ldc2 = P + 5, the dropout mask's ldm = F + 3.

PERSISTENT_CASES take M from the device's CU count (persistent_M): with two
workgroups per CU, 2 CU 4 + 4 tiles give four workgroups five tiles and the
rest four, so both LDS buffers are reused twice and the tail's wave wraps.
Their routes are checked where the count is known, on the GPU.

operands(case) draws AX, W1, W2 and b1 on binary quanta (see there) so that
every fp32 sum is exact in any order: H1 and S2 must EQUAL float64.
"""
from typing import NamedTuple

import numpy as np

# Every instantiation the library compiles (csrc/dense_gc1.hip, the comment above dense_gc1_route)
INSTANTIATIONS = ([(ks, *rest) for ks in (8, 13, 16, 25) for rest in ((3, 1, 0), (3, 1, 4), (4, 1, 0), (4, 2, 0))]
                  + [(32, 4, 1, 0), (32, 4, 2, 0)])
KS_VALUES = (8, 13, 16, 25, 32)
REQUIRED_K = (1, 3, 32, 33, 52, 53, 64, 65, 100, 101, 127, 128)
REQUIRED_K_KS = (8, 8, 8, 13, 13, 16, 16, 25, 25, 32, 32, 32)
REQUIRED_F_NI3 = (4, 8, 48, 52, 188, 192, 196, 200, 204, 208)
REQUIRED_F_NI4 = (4, 64, 68, 212, 252, 256)
REQUIRED_P = (1, 15, 16, 17, 18, 19, 20, 21, 31, 32)
REQUIRED_M = (1, 15, 16, 17, 70)
TAIL_M = 515            # 33 tiles: the first tile's tail wave takes all four values
SCALE = 2.0             # the dropout scale of every case (exactly 2: H1 stays on its quantum)
GUARD = 3               # NaN / sentinel rows before and after every two-dimensional operand
GUARD_B1 = 16           # NaN floats before and after b1 (64 B: b1 stays 16-B aligned)
SENTINEL = -12345.0     # what the output parents hold before a launch


class Case(NamedTuple):
    name: str
    M: int              # 0: taken from the device (PERSISTENT_CASES)
    K: int
    F: int
    P: int
    ldax: int
    ldw1: int
    ldw2: int
    ldh: int
    ldc2: int
    route: tuple        # (KS, NI, NPM, PV, tail, ntiles); ntiles 0 where M is the device's

    @property
    def ldm(self):      # the uint8 dropout mask's
        return self.F + 3


def _case(M, K, F, P, ax, inst):
    ks, ni, npm, pv = inst
    ldax = K + 1 if ax == "odd" else (K + 3) // 4 * 4 + 4
    tail = int(ni == 3 and F > 192)
    name = f"ks{ks}n{ni}p{npm}v{pv}{'t' if tail else ''}-{M or 'cu'}x{K}x{F}x{P}-{ax}"
    return Case(name, M, K, F, P, ldax, F + 4, P + 3, F + 4, P + 5, (ks, ni, npm, pv, tail, (M + 15) // 16))


CASES = [
    # --- KS 8 (K <= 32)
    _case(17, 1, 4, 1, "odd", (8, 3, 1, 0)),            # one column unit: lane 0 reads W1's columns 1 .. 3, shift 2
    _case(70, 3, 52, 15, "r4", (8, 3, 1, 0)),           # one past a wave's 48 columns; shift 2 on wave 1
    _case(16, 32, 192, 16, "r4", (8, 3, 1, 0)),         # every lane whole, no tail
    _case(TAIL_M, 32, 196, 16, "odd", (8, 3, 1, 0)),    # a tail of 4 columns
    _case(15, 3, 8, 17, "odd", (8, 3, 1, 4)),           # shift 1
    _case(70, 32, 48, 20, "odd", (8, 3, 1, 4)),         # exactly one wave's columns
    _case(TAIL_M, 5, 200, 19, "r4", (8, 3, 1, 4)),      # a tail of 8
    _case(70, 1, 212, 1, "r4", (8, 4, 1, 0)),
    _case(17, 32, 256, 16, "odd", (8, 4, 1, 0)),
    _case(16, 3, 4, 21, "r4", (8, 4, 2, 0)),            # NI = 4 by P alone, F = 4
    _case(70, 32, 64, 32, "odd", (8, 4, 2, 0)),
    _case(16, 5, 212, 19, "odd", (8, 4, 2, 0)),
    # --- KS 13 (K <= 52)
    _case(70, 33, 188, 15, "odd", (13, 3, 1, 0)),       # shift 1 on wave 3's last lane
    _case(1, 52, 48, 16, "odd", (13, 3, 1, 0)),
    _case(TAIL_M, 50, 200, 8, "r4", (13, 3, 1, 0)),     # R8 with a 50-topic theta as X
    _case(17, 33, 52, 20, "r4", (13, 3, 1, 4)),
    _case(TAIL_M, 52, 204, 18, "odd", (13, 3, 1, 4)),   # a tail of 12
    _case(70, 52, 212, 16, "r4", (13, 4, 1, 0)),
    _case(16, 33, 252, 15, "odd", (13, 4, 1, 0)),
    _case(15, 50, 256, 32, "odd", (13, 4, 2, 0)),
    _case(70, 33, 68, 21, "r4", (13, 4, 2, 0)),
    _case(17, 52, 212, 17, "odd", (13, 4, 2, 0)),
    # --- KS 16 (K <= 64)
    _case(70, 53, 192, 1, "odd", (16, 3, 1, 0)),
    _case(TAIL_M, 64, 208, 16, "r4", (16, 3, 1, 0)),    # a whole tail of 16
    _case(16, 64, 188, 19, "odd", (16, 3, 1, 4)),
    _case(TAIL_M, 53, 196, 17, "r4", (16, 3, 1, 4)),
    _case(17, 64, 256, 1, "odd", (16, 4, 1, 0)),
    _case(70, 53, 212, 15, "r4", (16, 4, 1, 0)),
    _case(70, 64, 64, 31, "r4", (16, 4, 2, 0)),
    _case(15, 53, 252, 17, "odd", (16, 4, 2, 0)),
    _case(1, 64, 252, 18, "r4", (16, 4, 2, 0)),
    # --- KS 25 (K <= 100)
    _case(70, 65, 8, 16, "r4", (25, 3, 1, 0)),
    _case(TAIL_M, 100, 204, 15, "odd", (25, 3, 1, 0)),
    _case(17, 65, 192, 18, "odd", (25, 3, 1, 4)),
    _case(TAIL_M, 100, 208, 20, "r4", (25, 3, 1, 4)),   # the 20ng shape's widths
    _case(70, 100, 212, 16, "odd", (25, 4, 1, 0)),
    _case(1, 65, 256, 15, "r4", (25, 4, 1, 0)),
    _case(16, 65, 68, 32, "odd", (25, 4, 2, 0)),
    _case(70, 100, 208, 21, "r4", (25, 4, 2, 0)),       # NI = 4 by P alone at F = 208
    # --- KS 32 (K <= 128): NI = 4 whatever F and P
    _case(70, 101, 4, 1, "odd", (32, 4, 1, 0)),
    _case(17, 128, 200, 16, "r4", (32, 4, 1, 0)),
    _case(15, 127, 256, 15, "odd", (32, 4, 1, 0)),
    _case(70, 127, 64, 17, "r4", (32, 4, 2, 0)),
    _case(17, 101, 208, 20, "odd", (32, 4, 2, 0)),
    _case(16, 128, 256, 32, "odd", (32, 4, 2, 0)),
]

# M from the device: more than one tile per workgroup, both LDS buffers reused, the tail's wave wrapping
PERSISTENT_CASES = [
    _case(0, 5, 200, 19, "r4", (8, 3, 1, 4)),
    _case(0, 50, 256, 32, "odd", (13, 4, 2, 0)),
]

# one per NI / tail kind: a NaN in one row of AX stays in that row (tests/test_dense_gc1_routes.py)
NAN_ROW_CASES = [next(c for c in CASES if (c.M, c.K, c.F, c.P) == k)
                 for k in ((70, 100, 212, 16), (70, 33, 188, 15), (TAIL_M, 50, 200, 8))]


def persistent_M(cus):
    """16 (2 CU 4 + 3) + 5 rows: 2 CU 4 + 4 tiles over 2 CU workgroups, the last tile of 5 rows."""
    return 16 * (2 * cus * 4 + 3) + 5


def with_M(case, M):
    return case._replace(M=M, name=case.name.replace("-cux", f"-{M}x"), route=(*case.route[:5], (M + 15) // 16))


def hash_args(case):
    """(seed, offset, ldm, rng_base) of the case's hash-dropout launch: a seed with high bits set, an offset and a
    device base that are no multiple of anything, an ldm of its own."""
    seed = 0xC0FFEE0000000000 | (case.K << 20) | (case.F << 8) | case.P
    return seed, 1000003 * case.K + 17 * case.F + case.P, case.F + 1 + case.P % 5, 3 * case.F * max(case.M, 1) + 1


def _embed(vals, ld, fill=np.nan, dtype=np.float32, guard=GUARD):
    """[guard rows | rows x ld | guard rows], all `fill` but vals in the first columns of the middle rows."""
    rows, cols = vals.shape
    parent = np.full((rows + 2 * guard, ld), fill, dtype)
    parent[guard:guard + rows, :cols] = vals
    return parent


def operands(case):
    """The case's seeded operands, their NaN-filled parents and the float64 answers.

    AX, W1 and W2 are drawn from {-4 .. 4} / 4 and b1 from the same values with one -4 and one +4, so AX W1 + b1
    lies on the quantum 2^-4 and, with the dropout scale exactly 2, every term of H1 W2 on 2^-6.  The function asserts on the float64
    reference that every operand and every answer is an fp32 number and that the largest sum of absolute terms,
    from the case's own maxima, stays below 2^24 quanta -- then every partial sum, in any order, is exact in fp32 --
    and that at least a quarter of Z = AX W1 is positive and at least a quarter negative, and Z + b1 has both signs
    (ReLU has something to cut and something to keep).

    Returned: float64 "AX" [M x K], "W1", "W2", "b1", uint8 "mask" [M x F]; the parents "AXp" ((GUARD + M + GUARD)
    x ldax: NaN in the columns K .. ldax - 1 and in the guard rows), "W1p", "W2p" (likewise), "b1p" (GUARD_B1 NaN
    floats, b1, GUARD_B1 NaN floats), "maskp" (M x ldm plus guard rows, 255 in the pad); "ref": {(bias, drop): (H1,
    S2)} for bias in (True, False) and drop in (False, True: the mask at SCALE); "pre": {bias: Z + b1 or Z}; "bits":
    log2 of the largest sum of absolute terms in quanta, per sum.
    """
    M, K, F, P = case.M, case.K, case.F, case.P
    rng = np.random.default_rng([M, K, F, P, case.ldax])
    o = {"AX": rng.integers(-4, 5, (M, K)) / 4.0, "W1": rng.integers(-4, 5, (K, F)) / 4.0,
         "W2": rng.integers(-4, 5, (F, P)) / 4.0, "b1": rng.integers(-4, 5, F) / 4.0,
         "mask": rng.integers(0, 2, (M, F)).astype(np.uint8)}
    o["b1"][F // 2], o["b1"][F - 1] = -4.0, 4.0
    Z = o["AX"] @ o["W1"]
    o["pre"] = {True: Z + o["b1"], False: Z}
    o["ref"] = {}
    for bias in (True, False):
        H = np.maximum(o["pre"][bias], 0.0) + 0.0
        Hd = np.where(o["mask"] != 0, H * SCALE, 0.0)
        o["ref"][bias, False] = (H, H @ o["W2"] + 0.0)
        o["ref"][bias, True] = (Hd, Hd @ o["W2"] + 0.0)
    # the precondition of comparing by bits
    for x in (o["AX"], o["W1"], o["W2"], o["b1"], *(a for pair in o["ref"].values() for a in pair)):
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x), case.name
    zmax = (np.abs(o["AX"]) @ np.abs(o["W1"])).max() + np.abs(o["b1"]).max()
    smax = ((SCALE * (np.abs(o["AX"]) @ np.abs(o["W1"]) + np.abs(o["b1"]))) @ np.abs(o["W2"])).max()
    o["bits"] = {"Z + b1": float(np.log2(zmax / 2.0**-4)), "H1 W2": float(np.log2(max(smax, 2.0**-6) / 2.0**-6))}
    assert max(o["bits"].values()) < 24, (case.name, o["bits"])
    assert zmax <= 128 + 4 and smax < 2.0**17, (case.name, zmax, smax)
    assert (Z > 0).mean() >= 0.25 and (Z < 0).mean() >= 0.25, (case.name, (Z > 0).mean(), (Z < 0).mean())
    # (not a quarter: at K = 1 a bias of +-4 owns its column)
    assert (o["pre"][True] > 0).any() and (o["pre"][True] < 0).any(), case.name
    o["AXp"] = _embed(o["AX"], case.ldax)
    o["W1p"] = _embed(o["W1"], case.ldw1)
    o["W2p"] = _embed(o["W2"], case.ldw2)
    o["b1p"] = _embed(o["b1"][None, :], F, guard=0).reshape(-1)
    o["b1p"] = np.concatenate([np.full(GUARD_B1, np.nan, np.float32), o["b1p"], np.full(GUARD_B1, np.nan, np.float32)])
    o["maskp"] = _embed(o["mask"], case.ldm, fill=255, dtype=np.uint8)
    return o
