"""The case table of the fused gc2 backward (test infrastructure, no GPU import).

gcnk_gcn_bwd2_f32 launches one of eight instantiations gcn_bwd2_kernel<VEC, PM>
(csrc/bwd.hip) and the kernel picks, from its arguments, how it stages gS2 / G
(LDS-DMA or scalar loads), how it loads W2 (16-B row runs or guarded 4-B loads)
and how it sums its row lanes (float4 pieces or per float).  Each Case below
names the route it is meant to reach, as gcnk_gcn_bwd2_route (include/gcnk.h)
reports it: (vec, pm, slices, nblk, rpb, flags).  tests/test_bwd2_routes.py
checks on the CPU that every case reaches the route it names and that the table
reaches every entry of INSTANTIATIONS, every flag set and clear and every row /
slice / workgroup count at which the kernel's loops take another turn, and on
the GPU runs every case exactly against float64.

A case's operands are views into wider buffers:
  H   [M x N], ldh = N + pad_h, base h_off floats past a 16-byte boundary
  gZ1 [M x N], ldz = N + pad_z, base z_off floats past one
  gS2 [M x P], ldgs = P + pad_gs;  G [M x P] (with_g), ldg = P + pad_g
  W2  [N x P], ldw = P + pad_w, base w_off floats past a 16-byte boundary
The geometry, as bwd2_geometry (csrc/bwd.hip) computes it:
  pm = P padded to 8 / 16 / 32;  vec = 4 (N, ldh, ldz % 4 == 0, H and gZ1 16-B
  aligned, pm <= 16), else 2 (the same with 2 and 8 B), else 1
  slices = 256-column slices;  rpb = min(256, ceil(M / 256)) rows per workgroup,
  nblk = ceil(M / rpb) workgroups per slice
Inside a slice of CT column units (CT = 256 / vec but for the last slice) a
workgroup has RL = 256 / CT row lanes, each taking its rows 8 at a time: a lane
has a second batch where rpb > 8 RL.  The side reduce sums 256 workgroups'
partials per round: a second round where nblk > 256.
"""
from typing import NamedTuple

DMA, W_RUNS, VEC_REDUCE = 1, 2, 4   # route flags: out9[6], out9[7], out9[8] of gcnk_gcn_bwd2_route
ALL = DMA | W_RUNS | VEC_REDUCE

# Every instantiation the library compiles (csrc/bwd.hip, the comment above ptr_align)
INSTANTIATIONS = [(v, pm) for v in (4, 2, 1) for pm in (8, 16, 32) if (v, pm) != (4, 32)]
# the reference datasets' class counts (mr, R8, 20ng, ohsumed) and the edges of pm
REQUIRED_P = (2, 8, 20, 23, 1, 9, 16, 17, 32)


class Case(NamedTuple):
    M: int
    N: int
    P: int
    route: tuple        # (vec, pm, slices, nblk, rpb, flags)
    pad_h: int = 0
    pad_z: int = 0
    pad_gs: int = 0
    pad_g: int = 0
    pad_w: int = 0
    h_off: int = 0
    z_off: int = 0
    w_off: int = 0
    with_g: bool = True

    @property
    def ldh(self):
        return self.N + self.pad_h

    @property
    def ldz(self):
        return self.N + self.pad_z

    @property
    def ldgs(self):
        return self.P + self.pad_gs

    @property
    def ldg(self):
        return self.P + self.pad_g

    @property
    def ldw(self):
        return self.P + self.pad_w

    @property
    def h_align(self):
        return align_of(self.h_off)

    @property
    def z_align(self):
        return align_of(self.z_off)

    @property
    def name(self):
        vec, pm, slices, nblk, rpb, fl = self.route
        pads = "".join(f"{k}{v}" for k, v in (("h", self.pad_h), ("z", self.pad_z), ("s", self.pad_gs), ("g", self.pad_g),
                                              ("w", self.pad_w)) if v)
        offs = "".join(f"{k}{v}" for k, v in (("H", self.h_off), ("Z", self.z_off), ("W", self.w_off)) if v)
        return (f"v{vec}p{pm}{'d' if fl & DMA else ''}{'w' if fl & W_RUNS else ''}{'r' if fl & VEC_REDUCE else ''}-"
                f"{self.M}x{self.N}x{self.P}{'-' + pads if pads else ''}{'-off' + offs if offs else ''}"
                f"{'' if self.with_g else '-noG'}")


def align_of(off):
    """Largest of 16, 8, 4 bytes that a pointer `off` floats past a 16-byte boundary is aligned to."""
    return 16 if off % 4 == 0 else 8 if off % 2 == 0 else 4


CASES = []

# --- every instantiation, everything contiguous: DMA staging and W2 row runs wherever P == pm, the float4
# lane sum on VEC 4.  1300 rows: rpb = 6, nblk = 217, the last workgroup has 4 rows; at N = 200 every row lane
# (5 on VEC 4, 2 on VEC 2) has a row.  VEC 2: N = 50, or an H whose base is only 8-B aligned; VEC 1: an odd N, an
# odd ldh, or a base that is only 4-B aligned.
CASES += [
    Case(1300, 200, 8, (4, 8, 1, 217, 6, ALL)),                               # R8's classes at nhid 200
    Case(1300, 200, 16, (4, 16, 1, 217, 6, ALL)),
    Case(300, 50, 8, (2, 8, 1, 150, 2, DMA | W_RUNS)),
    Case(300, 8, 16, (2, 16, 1, 150, 2, DMA | W_RUNS), h_off=2),
    Case(300, 50, 32, (2, 32, 1, 150, 2, DMA | W_RUNS)),                      # P = 32: DMA and row runs on VEC 2
    Case(300, 7, 8, (1, 8, 1, 150, 2, DMA | W_RUNS)),
    Case(300, 8, 16, (1, 16, 1, 150, 2, DMA | W_RUNS), pad_h=1),
    Case(300, 9, 32, (1, 32, 1, 150, 2, DMA | W_RUNS)),
    Case(300, 8, 8, (2, 8, 1, 150, 2, DMA | W_RUNS), z_off=2),                # gZ1's base decides too
    Case(300, 8, 8, (1, 8, 1, 150, 2, DMA | W_RUNS), h_off=1, z_off=1),
    Case(300, 8, 8, (2, 8, 1, 150, 2, DMA | W_RUNS), pad_h=2, pad_z=2),       # ld % 4 == 2
]

# --- P at the reference datasets' class counts and at the edges of pm, all at nhid 200.  P < pm: scalar
# staging (zero-padded to pm), guarded W2 loads and the per-float lane sum -- on the float4 column path for
# P <= 16 (mr's 2 classes), on VEC 2 past 16 (N = 200 with 20 classes falls from VEC 4 because pm = 32).
CASES += [
    Case(1300, 200, 2, (4, 8, 1, 217, 6, 0)),                                 # mr
    Case(1300, 200, 1, (4, 8, 1, 217, 6, 0)),
    Case(1300, 200, 9, (4, 16, 1, 217, 6, 0)),
    Case(1300, 200, 20, (2, 32, 1, 217, 6, 0)),                               # 20ng
    Case(1300, 200, 23, (2, 32, 1, 217, 6, 0)),                               # ohsumed
    Case(1300, 200, 17, (2, 32, 1, 217, 6, 0)),
    Case(1300, 200, 32, (2, 32, 1, 217, 6, DMA | W_RUNS)),
    Case(300, 9, 2, (1, 8, 1, 150, 2, 0)),                                    # P < pm on VEC 1, each pm
    Case(300, 9, 9, (1, 16, 1, 150, 2, 0)),
    Case(300, 9, 17, (1, 32, 1, 150, 2, 0)),
    Case(300, 50, 9, (2, 16, 1, 150, 2, 0)),
]

# --- staging: each way of leaving the DMA (P == pm throughout; P < pm is above), and DMA without G
CASES += [
    Case(300, 200, 8, (4, 8, 1, 150, 2, W_RUNS | VEC_REDUCE), pad_gs=4),                # ldgs > P
    Case(300, 200, 8, (4, 8, 1, 150, 2, W_RUNS | VEC_REDUCE), pad_g=4),                 # ldg > P, ldgs == P
    Case(300, 200, 8, (4, 8, 1, 150, 2, ALL), pad_g=4, with_g=False),                   # ... which only counts with G
    Case(300, 200, 16, (4, 16, 1, 150, 2, ALL), with_g=False),
    Case(300, 50, 32, (2, 32, 1, 150, 2, W_RUNS), pad_gs=1),
    Case(300, 50, 32, (2, 32, 1, 150, 2, W_RUNS), pad_g=3),
    Case(300, 7, 16, (1, 16, 1, 150, 2, W_RUNS), pad_gs=2, pad_g=2),
]

# --- W2: rows apart (ldw > P) and a base one float past a 16-byte boundary leave the row runs
CASES += [
    Case(300, 200, 8, (4, 8, 1, 150, 2, DMA | VEC_REDUCE), pad_w=4),
    Case(300, 200, 8, (4, 8, 1, 150, 2, DMA | VEC_REDUCE), w_off=1),
    Case(300, 200, 16, (4, 16, 1, 150, 2, DMA | VEC_REDUCE), pad_w=1),
    Case(300, 50, 32, (2, 32, 1, 150, 2, DMA), w_off=1),
    Case(300, 7, 8, (1, 8, 1, 150, 2, DMA), pad_w=3),
    Case(300, 200, 2, (4, 8, 1, 150, 2, 0), pad_w=2, w_off=1),                # P < pm, W2 padded and offset
]

# --- slices, each with G (gb2 comes from slice 0 alone).  N = 260 on VEC 4: the second slice has one column
# unit, so 256 row lanes; N = 1030 on VEC 2: five slices, the last has three units (85 row lanes, one thread
# idle); N = 257 on VEC 1: the second slice is one column.  ldg > P: slice 0 leaves the DMA, the others keep it.
CASES += [
    Case(300, 260, 8, (4, 8, 2, 150, 2, ALL)),
    Case(300, 260, 9, (4, 16, 2, 150, 2, 0)),
    Case(300, 1030, 8, (2, 8, 5, 150, 2, DMA | W_RUNS)),
    Case(300, 1030, 20, (2, 32, 5, 150, 2, 0)),
    Case(300, 257, 8, (1, 8, 2, 150, 2, DMA | W_RUNS)),
    Case(300, 257, 23, (1, 32, 2, 150, 2, 0)),
    Case(300, 260, 16, (4, 16, 2, 150, 2, W_RUNS | VEC_REDUCE), pad_g=4),
]

# --- rows.  One row; rpb going 1 -> 2 (M = 257: the last workgroup has one row); a lane's second 8-row batch
# with a ragged end (VEC 1, N = 256: RL = 1, rpb = 10, the last workgroup has 5 rows; VEC 4, N = 256: RL = 4,
# rpb = 34, the last workgroup has 17 rows); rpb capped at 256 and 258 workgroups (the side reduce's second
# round, the last workgroup has one row).
CASES += [
    Case(1, 8, 8, (4, 8, 1, 1, 1, ALL)),
    Case(1, 7, 3, (1, 8, 1, 1, 1, 0)),
    Case(255, 200, 8, (4, 8, 1, 255, 1, ALL)),
    Case(256, 200, 8, (4, 8, 1, 256, 1, ALL)),
    Case(257, 200, 8, (4, 8, 1, 129, 2, ALL)),
    Case(257, 50, 20, (2, 32, 1, 129, 2, 0)),
    Case(2305, 256, 8, (1, 8, 1, 231, 10, DMA | W_RUNS), pad_h=1),
    Case(2305, 256, 5, (1, 8, 1, 231, 10, 0), h_off=1),
    Case(8449, 256, 8, (4, 8, 1, 249, 34, ALL)),
    Case(8449, 256, 9, (4, 16, 1, 249, 34, 0)),
    Case(4200, 50, 32, (2, 32, 1, 248, 17, DMA | W_RUNS)),                    # VEC 2: RL = 10, rpb = 17 <= 80
    Case(600, 65, 5, (1, 8, 1, 200, 3, 0)),                                   # VEC 1: RL = 3 = rpb, every lane a row
    Case(65793, 4, 8, (4, 8, 1, 258, 256, ALL)),
    Case(65793, 3, 2, (1, 8, 1, 258, 256, 0)),
]

# --- strides: H's and gZ1's rows apart, alone and together, on each column path
CASES += [
    Case(300, 200, 8, (4, 8, 1, 150, 2, ALL), pad_h=4),
    Case(300, 200, 8, (4, 8, 1, 150, 2, ALL), pad_z=4),
    Case(300, 200, 16, (4, 16, 1, 150, 2, ALL), pad_h=8, pad_z=4),
    Case(300, 50, 20, (2, 32, 1, 150, 2, 0), pad_h=2, pad_z=6),
    Case(300, 7, 8, (1, 8, 1, 150, 2, DMA | W_RUNS), pad_h=1, pad_z=2),
    Case(300, 260, 2, (4, 8, 2, 150, 2, 0), pad_h=4, pad_z=8, pad_gs=1, pad_g=2, pad_w=3, w_off=1),   # everything strided
]

# nullable outputs (gW / gb1 / G null, all three null): one case per column path, each with several slices
NULLABLE_CASES = [next(c for c in CASES if (c.N, c.P, c.pad_g) == k) for k in ((260, 8, 0), (1030, 20, 0), (257, 8, 0))]
