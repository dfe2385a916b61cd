"""The GEMM case table (test infrastructure, no GPU import).

gcnk_gemm_f32 picks one of six kernel families and about thirty template
instantiations from (transA, transB, M, N, K, lda, ldb, alignment, split_k).
Each Case below names the route it is meant to reach, as gcnk_gemm_route
(include/gcnk.h) reports it: (family, p0, p1, flags).  tests/test_gemm_routes.py
checks on the CPU that every case reaches the route it names and that the
table reaches every entry of INSTANTIATIONS -- the list the comment block above
gemm_route in csrc/gemm.hip keeps -- and on the GPU runs every case against
float64.

A case's operands are views into wider buffers:
  A   stored [M x K] ([K x M] with transA), lda = its columns + pad_a
  B   stored [K x N] ([N x K] with transB), ldb = its columns + pad_b
  C   [M x N], ldc = N + pad_c;  R (MASK_POS) [M x N], ldr = N + PAD_R
misalign "a_base" / "b_base": A's / B's base pointer is one float past a 16-byte boundary.
Shapes are the smallest that still reach the kernel: M ragged against the
kernel's row block (16 or 64 rows), N ragged inside the family's range, K at
the bottom and the top of each instantiation's range and off the 16-deep k
block; the skinny kernel also at K % 4 in {1, 2, 3} on rows padded to a
multiple of 4 floats (its scalar K tail).
"""
from typing import NamedTuple

# include/gcnk.h GCNK_GEMM_ROUTE_* (test_gemm_routes.py checks them against _lib's)
NARROW, SKINNY, SHORTK, SMALLM, TILED_N16, TILED = 1, 2, 3, 4, 5, 6
SPLIT, PTR_FETCH = 1, 2
FAMILY_NAMES = {NARROW: "narrow", SKINNY: "skinny", SHORTK: "shortk", SMALLM: "smallm", TILED_N16: "tiled16",
                TILED: "tiled"}
EPILOGUES = ("none", "bias", "bias_null", "bias_relu", "mask_pos")   # bias_null: BIAS with a null bias (adds 0)
REQUIRED_EPILOGUES = ("none", "bias", "bias_relu", "mask_pos")
PAD_R = 5


class Case(NamedTuple):
    ta: int
    tb: int
    M: int
    N: int
    K: int
    pad_a: int
    pad_b: int
    pad_c: int
    split_k: int
    epilogue: str
    misalign: str
    route: tuple

    @property
    def lda(self):
        return (self.M if self.ta else self.K) + self.pad_a

    @property
    def ldb(self):
        return (self.K if self.tb else self.N) + self.pad_b

    @property
    def name(self):
        fam, p0, p1, fl = self.route
        return (f"{FAMILY_NAMES[fam]}{p0}.{p1}{'s' if fl & SPLIT else ''}{'p' if fl & PTR_FETCH else ''}-"
                f"{'T' if self.ta else 'N'}{'T' if self.tb else 'N'}-{self.M}x{self.N}x{self.K}-"
                f"a{self.pad_a}b{self.pad_b}c{self.pad_c}-k{self.split_k}-{self.epilogue}"
                f"{'-' + self.misalign if self.misalign else ''}")


# Every instantiation the library compiles (csrc/gemm.hip, the comment block above gemm_route)
INSTANTIATIONS = (
    [(NARROW, kch, 2, 0) for kch in (13, 16)]
    + [(SKINNY, kb, nt, 0) for kb in (1, 2, 4, 8, 16) for nt in (1, 2, 4)]
    + [(SHORTK, kch, 3, 0) for kch in range(1, 9)]
    + [(SMALLM, 2, 2, SPLIT)]
    + [(fam, ta, tb, fl) for fam in (TILED_N16, TILED) for ta in (0, 1) for tb in (0, 1) for fl in (0, SPLIT)])
# ... and the tiled kernel's pointer loads (a run-time branch of each tile): reached on both tiles
PTR_FETCH_FAMILIES = (TILED_N16, TILED)


def _pad4(k):
    """Padding that makes a row of k floats a multiple of 4 floats and longer than k."""
    return 4 - k % 4


def _nn(M, N, K, epilogue, route, pad_a=None, pad_b=4, pad_c=4, split_k=1, misalign=""):
    return Case(0, 0, M, N, K, _pad4(K) if pad_a is None else pad_a, pad_b, pad_c, split_k, epilogue, misalign, route)


CASES = []

# --- narrow: gemm_shortk_kernel<13 | 16, 2>, M >= 16384, N in (16, 32], 128 < K <= 208 < K <= 256, K % 4 == 0.
# 16384 + 65 rows: the last group of 8 row blocks has empty tail blocks.
_NARROW_M = 16384 + 65
CASES += [
    _nn(_NARROW_M, 20, 132, "none", (NARROW, 13, 2, 0)),
    _nn(_NARROW_M, 28, 148, "mask_pos", (NARROW, 13, 2, 0)),
    _nn(_NARROW_M, 32, 200, "bias_relu", (NARROW, 13, 2, 0)),
    _nn(_NARROW_M, 28, 208, "bias", (NARROW, 13, 2, 0)),
    _nn(_NARROW_M, 32, 212, "bias_relu", (NARROW, 16, 2, 0)),
    _nn(_NARROW_M, 28, 244, "bias_null", (NARROW, 16, 2, 0)),
    _nn(_NARROW_M, 20, 256, "mask_pos", (NARROW, 16, 2, 0)),
    _nn(16384, 24, 256, "bias", (NARROW, 16, 2, 0), pad_c=0),
    _nn(_NARROW_M, 32, 252, "none", (NARROW, 16, 2, 0), pad_b=0),
    _nn(16383, 20, 200, "none", (SKINNY, 4, 2, 0)),          # one row short of the narrow kernel
    _nn(_NARROW_M, 16, 200, "none", (SKINNY, 4, 1, 0)),      # one n-tile: the skinny kernel at any M
]

# --- skinny: gemm_skinny_ksplit_kernel<KB, NT>; KB by K (16-deep k blocks per wave), NT by N; lda % 4 == 0.
# Bottom and top of every (KB, NT): the bottoms have K % 4 == 1 (the scalar K tail).
_SKINNY_K = {1: (1, 64), 2: (65, 128), 4: (129, 256), 8: (257, 512), 16: (513, 1024)}
_SKINNY_N = {1: (1, 16), 2: (17, 32), 4: (33, 64)}
_i = 0
for _kb, (_klo, _khi) in _SKINNY_K.items():
    for _nt, (_nlo, _nhi) in _SKINNY_N.items():
        for _n, _k in ((_nlo, _klo), (_nhi, _khi)):
            CASES.append(_nn((77, 130, 257)[_i % 3], _n, _k, EPILOGUES[_i % 5], (SKINNY, _kb, _nt, 0)))
            _i += 1
CASES += [   # K % 4 in {2, 3}, K off the k block, N inside the n-tile ranges
    _nn(77, 17, 66, "mask_pos", (SKINNY, 2, 2, 0)),
    _nn(130, 33, 67, "bias", (SKINNY, 2, 4, 0)),
    _nn(257, 1, 258, "bias_relu", (SKINNY, 8, 1, 0)),
    _nn(77, 50, 515, "none", (SKINNY, 16, 4, 0)),
    _nn(130, 20, 1023, "mask_pos", (SKINNY, 16, 2, 0)),
    _nn(257, 40, 510, "bias", (SKINNY, 8, 4, 0)),
    _nn(130, 8, 3, "bias_relu", (SKINNY, 1, 1, 0)),
    _nn(77, 28, 202, "none", (SKINNY, 4, 2, 0), pad_b=0, pad_c=0),
]

# --- short-K: gemm_shortk_kernel<KCH, 3>, N > 64, K <= 128, K, N, lda, ldb % 4 == 0; KCH = 16-deep k chunks.
# N = 68, 100, 200 leave a partial 48-column tile; 600 rows: two groups of 8 row blocks.
for _kch in range(1, 9):
    for _j, _k in enumerate((16 * (_kch - 1) + 4, 16 * _kch)):
        _i = 2 * _kch + _j
        CASES.append(_nn((77, 130, 257, 600)[_i % 4], (68, 100, 200)[_i % 3], _k, EPILOGUES[_i % 5],
                         (SHORTK, _kch, 3, 0)))
CASES += [
    _nn(130, 96, 100, "mask_pos", (SHORTK, 7, 3, 0), pad_b=0, pad_c=0),     # whole 48-column tiles, contiguous B, C
    _nn(77, 68, 40, "none", (SHORTK, 3, 3, 0)),
]

# --- small-M: gemm_smallm_wk_kernel<2, 2> + gemm_slab_reduce4_kernel (the epilogue is the reduce kernel's)
CASES += [
    _nn(50, 200, 1000, "none", (SMALLM, 2, 2, SPLIT), split_k=4),
    _nn(64, 36, 515, "bias", (SMALLM, 2, 2, SPLIT), split_k=3),
    _nn(1, 4, 512, "bias_relu", (SMALLM, 2, 2, SPLIT), split_k=2),
    _nn(17, 116, 4099, "mask_pos", (SMALLM, 2, 2, SPLIT), split_k=17),
    _nn(63, 332, 777, "bias_null", (SMALLM, 2, 2, SPLIT), split_k=8),
    _nn(50, 200, 1000, "bias", (TILED, 0, 0, SPLIT), split_k=3),            # fewer slabs than the kernel's 4
    _nn(65, 200, 1000, "none", (TILED, 0, 0, SPLIT), split_k=4),            # one row too many
]

# --- tiled, N <= 16 (128 x 16 tile) and N > 16 (64 x 64 tile): the four transposes, whole and split.
# (NN reaches them past the fast kernels' ranges: K > 1024, K % 4 != 0 with N > 64, rows not padded to 4 floats.)
CASES += [
    _nn(130, 8, 1040, "none", (TILED_N16, 0, 0, 0)),
    _nn(77, 16, 97, "bias", (TILED_N16, 0, 0, 0), pad_a=0),
    _nn(257, 8, 200, "mask_pos", (TILED_N16, 0, 0, SPLIT), split_k=4),
    Case(1, 0, 77, 8, 130, 3, 4, 4, 1, "bias_relu", "", (TILED_N16, 1, 0, 0)),
    Case(1, 0, 200, 8, 2000, 4, 0, 4, 8, "bias", "", (TILED_N16, 1, 0, SPLIT)),
    Case(0, 1, 130, 16, 50, 2, 6, 4, 1, "mask_pos", "", (TILED_N16, 0, 1, 0)),
    Case(0, 1, 257, 7, 300, 4, 4, 1, 3, "none", "", (TILED_N16, 0, 1, SPLIT)),
    Case(1, 1, 77, 5, 33, 3, 7, 3, 1, "bias", "", (TILED_N16, 1, 1, 0)),
    Case(1, 1, 130, 12, 260, 2, 4, 4, 2, "bias_relu", "", (TILED_N16, 1, 1, SPLIT)),
    Case(1, 0, 130, 16, 77, 0, 0, 0, 1, "none", "", (TILED_N16, 1, 0, 0)),
    Case(0, 1, 77, 1, 100, 4, 4, 3, 4, "bias_null", "", (TILED_N16, 0, 1, SPLIT)),

    _nn(257, 100, 97, "none", (TILED, 0, 0, 0)),
    _nn(130, 40, 1100, "bias", (TILED, 0, 0, 0)),
    _nn(77, 100, 300, "bias_relu", (TILED, 0, 0, SPLIT), split_k=3),
    _nn(77, 100, 100, "none", (TILED, 0, 0, SPLIT), split_k=8),              # 7 slabs of 16: fewer than asked for
    _nn(33, 70, 10, "bias", (TILED, 0, 0, 0), split_k=4),                    # one slab whatever was asked for
    Case(1, 0, 200, 52, 612, 4, 0, 4, 1, "none", "", (TILED, 1, 0, 0)),      # gW2 = H1^T gS2 of the unfused backward
    Case(1, 0, 200, 52, 2000, 3, 5, 4, 8, "mask_pos", "", (TILED, 1, 0, SPLIT)),
    Case(0, 1, 612, 200, 52, 0, 0, 0, 1, "mask_pos", "", (TILED, 0, 1, 0)),  # gZ1 = gS2 W2^T, MASK_POS, strided R
    Case(0, 1, 257, 50, 33, 3, 3, 6, 1, "bias_null", "", (TILED, 0, 1, 0)),
    Case(0, 1, 130, 68, 400, 4, 4, 4, 4, "bias", "", (TILED, 0, 1, SPLIT)),
    Case(1, 1, 77, 40, 130, 3, 2, 4, 1, "bias_relu", "", (TILED, 1, 1, 0)),
    Case(1, 1, 257, 33, 333, 7, 3, 5, 5, "none", "", (TILED, 1, 1, SPLIT)),
]

# --- fall-throughs: one shape per fast family, then one change at a time.  A's base pointer off a 16-byte
# boundary or rows of A not a multiple of 4 floats leave every fast kernel for the tiled one; rows of B not a
# multiple of 4 floats, or B's base pointer off a 16-byte boundary, take the short-K kernel to the tiled one and
# the narrow kernel to the skinny one (which reads B by scalars).
FALLTHROUGHS = []


def _fall(fast, *changed):
    CASES.extend((fast,) + changed)
    FALLTHROUGHS.append((fast, changed))


_f = _nn(_NARROW_M, 20, 200, "bias", (NARROW, 13, 2, 0))
_fall(_f, _f._replace(misalign="a_base", route=(TILED, 0, 0, 0)), _f._replace(pad_a=5, route=(TILED, 0, 0, 0)),
      _f._replace(pad_b=3, route=(SKINNY, 4, 2, 0)), _f._replace(misalign="b_base", route=(SKINNY, 4, 2, 0)))
_f = _nn(130, 20, 200, "bias_relu", (SKINNY, 4, 2, 0))
_fall(_f, _f._replace(misalign="a_base", route=(TILED, 0, 0, 0)), _f._replace(pad_a=5, route=(TILED, 0, 0, 0)))
_f = _nn(130, 8, 200, "mask_pos", (SKINNY, 4, 1, 0))
_fall(_f, _f._replace(misalign="a_base", route=(TILED_N16, 0, 0, 0)), _f._replace(pad_a=1, route=(TILED_N16, 0, 0, 0)))
_f = _nn(130, 100, 100, "mask_pos", (SHORTK, 7, 3, 0))
_fall(_f, _f._replace(misalign="a_base", route=(TILED, 0, 0, 0)), _f._replace(pad_a=5, route=(TILED, 0, 0, 0)),
      _f._replace(pad_b=3, route=(TILED, 0, 0, 0)), _f._replace(misalign="b_base", route=(TILED, 0, 0, 0)))
_f = _nn(50, 200, 1000, "bias_relu", (SMALLM, 2, 2, SPLIT), split_k=4)
_fall(_f, _f._replace(misalign="a_base", route=(TILED, 0, 0, SPLIT)), _f._replace(pad_a=5, route=(TILED, 0, 0, SPLIT)))

# --- operands past 32-bit byte offsets: strided views of one ~2.15 GB buffer (BIG_FLOATS), tiny products.
# A stored [4100 x 70] with lda = 131072 (transA): 4100 * 131072 * 4 B > 0x7ff00000, both tiles, whole and split.
# A [64 x 1000] with lda = 8388608: 64 * 8388608 * 4 B = 2^31, past the small-M kernel's buffer offsets too.
BIG_FLOATS = 4100 * 131072
BIG_CASES = [
    Case(1, 0, 70, 8, 4100, 131072 - 70, 4, 4, 1, "none", "", (TILED_N16, 1, 0, PTR_FETCH)),
    Case(1, 0, 70, 40, 4100, 131072 - 70, 4, 4, 8, "bias", "", (TILED, 1, 0, SPLIT | PTR_FETCH)),
    Case(0, 0, 64, 40, 1000, 8388608 - 1000, 4, 4, 4, "mask_pos", "", (TILED, 0, 0, SPLIT | PTR_FETCH)),
]

ALL_CASES = CASES + BIG_CASES
