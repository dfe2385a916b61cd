"""The SpMM case table (test infrastructure, no GPU import).

gcnk_spmm_csr_f32 / gcnk_spmm_csr_f32_part / gcnk_spmm_proj_f32 launch from
one host function, spmm_route (csrc/spmm.hip), which gcnk_spmm_route
(include/gcnk.h) reports: the row kernel's (LPR, VEC, NP), its column windows
and their O32, whether spmm_heavy_top_kernel follows; the tile kernel's
(VEC4, NT, DIAG), its column slices and whether the slab reduce follows.  Each
Case below names the route it is meant to reach (the first 14 words of the
report).  tests/test_spmm_cases.py checks on the CPU that every case reaches
the route it names and that the table reaches every entry of INSTANTIATIONS
-- the list the comment block above spmm_route keeps --, and
tests/test_spmm_routes.py runs every case on the GPU, under all five epilogue
codes, against float64.

Operands (the smallest that still hold every row kind):
  R     48 x 2048, rectangular (no diagonal), row kernel only.  Rows 0-12 hold
        R_DEGREES nonzeros, the other 35 rows 1..8.  At ipc 4 every LPR sees
        light units, heavy units and multi-segment heavy rows; at LPR 64 / ipc 4
        a row of more than 64 segments too (a top entry), at LPR 64 / ipc 12 and
        at LPR 16, 32 / ipc 4 none (the projection's settings).
  T700, T900   test_gpu_parity._mixed_density_csr at M = 700 / 900, K = 900:
        single- and multi-chunk tile blocks beside the row kernel; M = 900 is
        square and keeps its diagonal aside (DIAG).
  BIG   R's row degrees with columns from three bands of 64 rows of B: the
        first, the ones around row 2^19 (byte offset 2^31 at ldb = 1024) and
        the last below K; K = 2^20 - 1 (O32, offsets up to just under 2^32),
        2^20 (the first K without O32) and 2^20 + 16 (offsets past 2^32).
        B is a view of one [BIG_ROWS x 1024] buffer.
A case's B and C are views into wider buffers (ldb = F + pad_b -- 1024 for
BIG --, ldc = F + pad_c); misalign names the one base pointer that is 4 bytes
past a 16-byte boundary.
"""
import functools
from typing import NamedTuple

import numpy as np

EPILOGUES = ("none", "bias", "bias_relu", "drop", "hash")   # GCNK_EPI_* 0..4
MISALIGN = ("", "b_base", "c_base", "bias_base", "ws_base")
LPRS = (1, 2, 4, 8, 16, 32, 64)
PROJ_LPRS = (16, 32, 64)
BIG_LDB = 1024
BIG_ROWS = 2**20 + 16
BIG_K = {"lo": 2**20 - 1, "edge": 2**20, "hi": 2**20 + 16}
R_DEGREES = (0, 1, 2, 5, 16, 17, 63, 64, 65, 130, 300, 1100, 2048)

NO_ROWS = (0,) * 8
NO_TILE = (0,) * 6


def rows(lpr, vec, np_=0, o32=1, windows=1, top=0):
    """out16[0:8]: launches, LPR, VEC, NP, windows, O32 first, O32 last, top kernel follows."""
    return (1, lpr, vec, np_, windows, o32, o32, top)


def tile(v4, nt, diag, slices=1, reduce=1):
    """out16[8:14]: launches, VEC4, NT, DIAG, column slices, slab reduce follows."""
    return (1, v4, nt, diag, slices, reduce)


class Case(NamedTuple):
    operand: str        # "R", "T700", "T900", "BIG_lo", "BIG_edge", "BIG_hi"
    F: int
    lanes: int          # lanes_hint (0: from F)
    ipc: int            # 0: gcnk_spmm_default_ipc
    dense: float        # dense threshold of the plan (2.0: no tile part)
    pad_b: int
    pad_c: int
    misalign: str
    P: int              # 0: no projection
    store_main: bool
    two_part: bool      # also run as gcnk_spmm_csr_f32_part 1 then 2: same bits
    tops: bool          # the plan has a top entry
    tag: str            # what the case is in the table for (REQUIRED)
    route: tuple

    @property
    def name(self):
        r = self.route
        s = self.operand
        if r[0]:
            s += f"-row{r[1]}x{r[2]}" + (f"p{r[3]}" if r[3] else "") + ("" if r[5] and r[6] else "-o64")
            s += f"-w{r[4]}" if r[4] > 1 else ""
            s += "-top" if r[7] else ""
        if r[8]:
            s += f"-tile{'v' if r[9] else 's'}{r[10]}{'d' if r[11] else ''}"
        s += f"-F{self.F}"
        if self.P:
            s += f"-P{self.P}{'' if self.store_main else '-nostore'}"
        if (self.pad_b, self.pad_c) != (4, 4) and not self.operand.startswith("BIG"):
            s += f"-b{self.pad_b}c{self.pad_c}"
        return s + (f"-{self.misalign}" if self.misalign else "")


# Every instantiation csrc/spmm.hip compiles and a launch can reach (the comment block above spmm_route)
INSTANTIATIONS = (
    [("row", lpr, vec, o32) for lpr in LPRS for vec in (4, 1) for o32 in (1, 0)]
    + [("proj", lpr, np_, o32) for lpr in PROJ_LPRS for np_ in (8, 32) for o32 in (1, 0)]
    + [("top", vec) for vec in (4, 1)]
    + [("tile", v4, nt, diag) for v4 in (1, 0) for nt in (1, 2, 4) for diag in (1, 0)]
    + [("reduce",)])
# ... and the ones it compiles that no launch reaches at the default GCNK_TILE_MAXNT = 4
UNREACHABLE = [("tile", v4, nt, diag) for v4 in (1, 0) for nt in (6, 7, 8) for diag in (1, 0)]


def instantiations_of(route):
    """The kernels a reported route (out16) launches, as entries of INSTANTIATIONS."""
    r = tuple(route)
    got = set()
    if r[0]:
        for o32 in {r[5], r[6]} if r[4] > 1 else {r[5]}:
            got.add(("proj", r[1], r[3], o32) if r[3] else ("row", r[1], r[2], o32))
        if r[7]:
            got.add(("top", r[2]))
    if r[8]:
        got.add(("tile", r[9], r[10], r[11]))
    if r[13]:
        got.add(("reduce",))
    return got


def _r(F, lanes, route, ipc=4, tag="R", **kw):
    d = dict(operand="R", F=F, lanes=lanes, ipc=ipc, dense=2.0, pad_b=4, pad_c=4, misalign="", P=0, store_main=True,
             two_part=False, tops=bool(route[7]), tag=tag, route=route + NO_TILE)
    d.update(kw)
    return Case(**d)


def _row_f(lpr, vec):
    """Three column tiles, the last ragged (whole at LPR 1 x VEC 4)."""
    return 8 * lpr + 4 if vec == 4 else 2 * lpr + 1


# --- row kernel, every (LPR, VEC): R at ipc 4, lanes = LPR.  At LPR 64 the plan has a top entry, so
# spmm_heavy_top_kernel<4> / <1> follow.
ROW_CASES = [_r(_row_f(lpr, vec), lpr, rows(lpr, vec, top=int(lpr == 64))) for lpr in LPRS for vec in (4, 1)]

# --- column windows (more than 64 column tiles): the second window runs on re-armed arrival counters, shifted
# B, C, bias, mask, partial slots and hash offset, at LPR 64 with the top entry
WINDOW_CASES = [
    _r(130, 1, rows(1, 1, windows=3), tag="windows"),                   # 64 + 64 + 2 tiles
    _r(264, 1, rows(1, 4, windows=2), tag="windows"),                   # 66 tiles
    _r(4101, 64, rows(64, 1, windows=2, top=1), tag="windows"),         # 65 tiles
    _r(16388, 64, rows(64, 4, windows=2, top=1), tag="windows"),        # 65 tiles
]

# --- each condition of the float4 path violated alone (F = 200, lanes from F: LPR 64; F % 4 at F = 202 on rows of
# 204 floats, so that ldb and ldc stay multiples of 4)
VEC4_BASE = _r(200, 0, rows(64, 4, top=1), tag="vec4: none violated")
VEC4_VIOLATIONS = {
    "F % 4": VEC4_BASE._replace(tag="vec4: F % 4", F=202, pad_b=2, pad_c=2, route=rows(64, 1, top=1) + NO_TILE),
    "ldb % 4": VEC4_BASE._replace(tag="vec4: ldb % 4", pad_b=5, route=rows(64, 1, top=1) + NO_TILE),
    "ldc % 4": VEC4_BASE._replace(tag="vec4: ldc % 4", pad_c=5, route=rows(64, 1, top=1) + NO_TILE),
    "B base": VEC4_BASE._replace(tag="vec4: B base", misalign="b_base", route=rows(64, 1, top=1) + NO_TILE),
    "C base": VEC4_BASE._replace(tag="vec4: C base", misalign="c_base", route=rows(64, 1, top=1) + NO_TILE),
    "bias base": VEC4_BASE._replace(tag="vec4: bias base", misalign="bias_base", route=rows(64, 1, top=1) + NO_TILE),
    "workspace base": VEC4_BASE._replace(tag="vec4: workspace base", misalign="ws_base", route=rows(64, 1, top=1) + NO_TILE),
}
VEC4_CASES = [VEC4_BASE] + list(VEC4_VIOLATIONS.values())


# --- fused projection: lanes 16, 32, 64 x P 8 (NP 8), 20 (NP 32) x F = 4 LPR (every lane busy), 4 LPR - 12
# (idle lanes in the one tile) x H stored or not.  Plans without a top entry: ipc 4 at LPR 16, 32, ipc 12 at 64.
def _proj_ipc(lpr):
    return 12 if lpr == 64 else 4


def _proj_tag(F, lpr, store):
    return f"{'every lane' if F == 4 * lpr else 'idle lanes'}, {'H stored' if store else 'H not stored'}"


PROJ_CASES = [_r(F, lpr, rows(lpr, 4, np_=8 if P <= 8 else 32), ipc=_proj_ipc(lpr), P=P, store_main=store,
                 tag=_proj_tag(F, lpr, store))
              for lpr in PROJ_LPRS for P in (8, 20) for F in (4 * lpr, 4 * lpr - 12) for store in (True, False)]


# --- gather offsets at and past 32 bits: views of one [BIG_ROWS x 1024] B.  "hi" (and "edge", the first K without
# O32): every row (LPR, VEC) and every projection (LPR, NP) at O32 = false; "lo": O32 with byte offsets up to just
# under 2^32.
def _big(which, F, lanes, route, ipc=4, **kw):
    return _r(F, lanes, route, ipc=ipc, operand="BIG_" + which, pad_b=BIG_LDB - F, tag=which, **kw)


# (its repeated columns fall unevenly on the planner's column classes: a top entry at LPR 32 / ipc 4 already)
_BIG_PROJ_IPC = {16: 4, 32: 8, 64: 12}
BIG_CASES = (
    [_big("hi", _row_f(lpr, vec), lpr, rows(lpr, vec, o32=0, top=int(lpr >= 32))) for lpr in LPRS for vec in (4, 1)]
    + [_big("hi", 4 * lpr, lpr, rows(lpr, 4, np_=8 if P <= 8 else 32, o32=0), ipc=_BIG_PROJ_IPC[lpr], P=P)
       for lpr in PROJ_LPRS for P in (8, 20)]
    + [_big("edge", _row_f(64, 4), 64, rows(64, 4, o32=0, top=1)),
       _big("edge", _row_f(2, 1), 2, rows(2, 1, o32=0)),
       _big("edge", 64, 16, rows(16, 4, np_=32, o32=0), P=20, store_main=False)]
    + [_big("lo", _row_f(64, 4), 64, rows(64, 4, top=1)),
       _big("lo", _row_f(64, 1), 64, rows(64, 1, top=1)),
       _big("lo", _row_f(2, 4), 2, rows(2, 4)),
       _big("lo", _row_f(16, 1), 16, rows(16, 1)),
       _big("lo", 256, 64, rows(64, 4, np_=8), ipc=12, P=8)])


# --- tile path: NT 2 at both VEC4 and NT 4 scalar, on both M (DIAG at M = 900), single launch and two parts.
# The operand's other rows run in the row kernel beside it (lanes from F).
def _t(M, F, row_route, tile_route):
    return Case(f"T{M}", F, 0, 0, 0.25, 4, 4, "", 0, True, True, False, "T", row_route + tile_route)


TILE_CASES = [c for M in (700, 900) for c in (
    _t(M, 18, rows(32, 1), tile(0, 2, int(M == 900))),
    _t(M, 20, rows(8, 4), tile(1, 2, int(M == 900))),
    _t(M, 50, rows(64, 1), tile(0, 4, int(M == 900))),
    # the widths of the existing tests, so that the table covers the other tile instantiations too
    _t(M, 7, rows(8, 1), tile(0, 1, int(M == 900))),
    _t(M, 8, rows(2, 4), tile(1, 1, int(M == 900))),
    _t(M, 200, rows(64, 4), tile(1, 4, int(M == 900), slices=4)),
)]

# What the table is for: (instantiation, tag) pairs, each reached by exactly one case -- so taking any case out
# orphans one (test_table_reaches_every_instantiation names it).
REQUIRED = (
    [(("row", lpr, vec, 1), "R") for lpr in LPRS for vec in (4, 1)] + [(("top", vec), "R") for vec in (4, 1)]
    + [(("row", lpr, vec, 1), "windows") for lpr in (1, 64) for vec in (4, 1)]
    + [(("row", 64, 4, 1), "vec4: none violated")] + [(("row", 64, 1, 1), "vec4: " + k) for k in VEC4_VIOLATIONS]
    + [(("proj", lpr, np_, 1), f"{lanes}, {h}") for lpr in PROJ_LPRS for np_ in (8, 32)
       for lanes in ("every lane", "idle lanes") for h in ("H stored", "H not stored")]
    + [(("tile", v4, nt, diag), "T") for v4 in (1, 0) for nt in (1, 2, 4) for diag in (1, 0)]
    + [(("row", lpr, vec, 0), "hi") for lpr in LPRS for vec in (4, 1)]
    + [(("proj", lpr, np_, 0), "hi") for lpr in PROJ_LPRS for np_ in (8, 32)]
    + [(("row", 64, 4, 0), "edge"), (("row", 2, 1, 0), "edge"), (("proj", 16, 32, 0), "edge")]
    + [(("row", 64, 4, 1), "lo"), (("row", 64, 1, 1), "lo"), (("row", 2, 4, 1), "lo"), (("row", 16, 1, 1), "lo"),
       (("proj", 64, 8, 1), "lo")])

SMALL_CASES = ROW_CASES + WINDOW_CASES + VEC4_CASES + PROJ_CASES + TILE_CASES
ALL_CASES = SMALL_CASES + BIG_CASES


# ------------------------------------------------------------------------------ operands (host CSR arrays)

def _csr(cols, seed):
    rp = np.zeros(len(cols) + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols])
    ci = np.concatenate(cols).astype(np.int64)
    v = np.random.default_rng(seed).standard_normal(len(ci)).astype(np.float32)
    return rp, ci, v


def _degrees(rng):
    return list(R_DEGREES) + [int(d) for d in rng.integers(1, 9, 35)]


@functools.lru_cache(maxsize=None)
def operand(name):
    """(rowptr, colind, val, (M, K)) of a case's operand."""
    if name == "R":
        rng = np.random.default_rng(2048)
        return _csr([np.sort(rng.choice(2048, d, replace=False)) for d in _degrees(rng)], 1) + ((48, 2048),)
    if name.startswith("BIG_"):
        K = BIG_K[name[4:]]
        rng = np.random.default_rng(20)
        band = np.concatenate([np.arange(64), 2**19 - 32 + np.arange(64), K - 64 + np.arange(64)])
        cols = []
        for d in _degrees(rng):   # (more nonzeros than band rows: columns repeat within a row)
            c = rng.choice(band, d, replace=d > len(band))
            cols.append(np.sort(np.concatenate([band, c[len(band):]]) if d > len(band) else c))
        return _csr(cols, 2) + ((48, K),)
    if name in ("T700", "T900"):
        from test_gpu_parity import _mixed_density_csr
        M = int(name[1:])
        return tuple(_mixed_density_csr(np.random.default_rng(M), M, 900)) + ((M, 900),)
    raise KeyError(name)
