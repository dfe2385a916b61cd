"""The case table of the factored gc1 kernel and the hand-built operands its
tests run on (test infrastructure, no GPU import).

gcnk_hubfactor_gc1_f32 launches one of 24 instantiations
hubfactor_gc1_kernel<KS, NTQ, NP> (csrc/factor.hip):
  KS  = 13 / 18 / 25 / 32 k-steps of U W1[Kc], cutting at Kc = 52, 72 and 100
  NTQ = 2 / 3 / 4 16-column tiles of F per wave, cutting at F = 128 and 192
  NP  = 1 / 2 n-tiles of P, cutting at P = 16
and stages U's rows through LDS (u_lds) where ldu % 4 == 0, U is 16-B aligned
and the rows fit beside the block's other operands in 160 KiB, else loads U's
fragments directly.  Each Case names the route it is meant to reach, as
gcnk_hubfactor_gc1_route (include/gcnk.h) reports it: (KS, NTQ, NP, u_lds).
tests/test_hubfactor_routes.py checks on the CPU that every case reaches the
route it names and that the table reaches every instantiation, both u_lds values
per KS (0 by an ldu that is no multiple of 4 and by the LDS budget) and both
sides of every cut, and on the GPU runs every case against float64.

operands(): the construction of tests/test_hubfactor_items.py for any shape;
the block records are packed by tests/hub_records.py.
"""
from typing import NamedTuple

import numpy as np

from hub_records import ROWS, pack, rec_words_for

M = 70                       # three 32-row blocks, the last with 6 real rows
COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 0]   # ..., 17, 0, 0, 1, ... down a block
LONG_POS, LONG_ITEMS = 32 + 13, 200               # the long row: middle block, followed by an empty row
NAN_BITS = np.int32(0x7FC00000)
K0 = 3

KS_VALUES, NTQ_VALUES, NP_VALUES = (13, 18, 25, 32), (2, 3, 4), (1, 2)
INSTANTIATIONS = [(ks, ntq, np_) for ks in KS_VALUES for ntq in NTQ_VALUES for np_ in NP_VALUES]
# both sides of every cut, and the ends of every range
REQUIRED_KC = (1, 4, 52, 53, 72, 73, 100, 101, 127, 128)
REQUIRED_F = (4, 128, 132, 192, 196, 256)
REQUIRED_P = (1, 16, 17, 32)


def item_counts():
    """Items per position of the block order (rows past M hold nothing)."""
    nblk = (M + ROWS - 1) // ROWS
    counts = np.array([COUNTS[(p % ROWS) % len(COUNTS)] for p in range(nblk * ROWS)])
    counts[M:] = 0                                 # rows past M hold nothing
    counts[LONG_POS] = LONG_ITEMS
    counts[LONG_POS + 1] = 0                       # an empty row right after the long one
    counts[2 * ROWS - 1] = 0                       # and one as that block's last row
    return counts


def rec_words():
    return rec_words_for(item_counts(), tail=4)   # every record keeps a tail


REC_WORDS = rec_words()


def operands(nhub, Kc, F, P, ldu):
    """Seeded operands of one launch and Z = U W1[K0:K0+Kc] + A_H S in float64
    from the same arrays, rows in output order.  The unused tail of every
    record and U's columns past Kc are NaN bits."""
    rng = np.random.default_rng(1000 * nhub + 10 * Kc + F + P)
    perm = rng.permutation(M)                      # position in block order -> output row
    assert not np.array_equal(perm, np.arange(M))
    counts = item_counts()
    hubs = [rng.integers(0, nhub, c) for c in counts]             # repeated hubs allowed
    vals = [rng.uniform(-1.0, 1.0, c).astype(np.float32) for c in counts]
    words = rec_words()
    rec = pack([list(zip(h, v)) for h, v in zip(hubs, vals)], perm, M, words, NAN_BITS)
    U = np.zeros((M, ldu), np.float32)
    U[:, :Kc] = rng.standard_normal((M, Kc)) * 0.3
    U[:, Kc:] = np.nan                             # columns past Kc are not the kernel's to read into Z
    W1 = rng.standard_normal((K0 + Kc + 5, F)).astype(np.float32)
    S = rng.standard_normal((nhub, F)).astype(np.float32)
    b1 = rng.standard_normal(F).astype(np.float32)
    W2 = rng.standard_normal((F, P)).astype(np.float32)
    # float64 from the same arrays, rows in output order
    Z = np.zeros((M, F))
    UW = U[:, :Kc].astype(np.float64) @ W1[K0:K0 + Kc].astype(np.float64)
    for pos in range(M):
        z = UW[pos].copy()
        for hcol, val in zip(hubs[pos], vals[pos]):
            z += np.float64(val) * S[hcol].astype(np.float64)
        Z[perm[pos]] = z
    return dict(rec=rec, rec_words=words, ldu=ldu, U=U, W1=W1, S=S, b1=b1, W2=W2, Z=Z)


class Case(NamedTuple):
    Kc: int
    F: int
    P: int
    nhub: int
    ldu: int
    route: tuple        # (KS, NTQ, NP, u_lds)

    @property
    def name(self):
        ks, ntq, np_, u_lds = self.route
        return f"ks{ks}q{ntq}p{np_}{'u' if u_lds else ''}-{self.Kc}x{self.F}x{self.P}-h{self.nhub}-ld{self.ldu}"


CASES = []

# --- every instantiation, U staged in LDS (ldu a multiple of 4: Kc rounded up, or wider).  Kc, F and P walk
# the required values; Kc = 1, 53, 73, 101 and 127 are no multiple of 4 (the row's last 16-B piece reaches
# past Kc into U's NaN columns; W1's rows past Kc are the kernel's zero fill).
CASES += [
    Case(1, 4, 1, 7, 4, (13, 2, 1, 1)),
    Case(4, 128, 17, 7, 4, (13, 2, 2, 1)),
    Case(52, 132, 16, 7, 52, (13, 3, 1, 1)),
    Case(1, 192, 32, 7, 8, (13, 3, 2, 1)),
    Case(4, 196, 1, 7, 8, (13, 4, 1, 1)),
    Case(52, 256, 17, 7, 56, (13, 4, 2, 1)),
    Case(53, 4, 16, 7, 56, (18, 2, 1, 1)),
    Case(72, 128, 32, 7, 72, (18, 2, 2, 1)),
    Case(53, 132, 1, 7, 60, (18, 3, 1, 1)),
    Case(72, 192, 17, 7, 76, (18, 3, 2, 1)),
    Case(53, 196, 16, 7, 56, (18, 4, 1, 1)),
    Case(72, 256, 32, 7, 72, (18, 4, 2, 1)),
    Case(73, 4, 1, 7, 76, (25, 2, 1, 1)),
    Case(100, 128, 17, 7, 100, (25, 2, 2, 1)),
    Case(73, 132, 16, 7, 76, (25, 3, 1, 1)),
    Case(100, 192, 32, 7, 104, (25, 3, 2, 1)),
    Case(73, 196, 1, 7, 80, (25, 4, 1, 1)),
    Case(100, 256, 17, 7, 100, (25, 4, 2, 1)),     # the dense 100-d X at the widest hidden layer
    Case(101, 4, 16, 7, 104, (32, 2, 1, 1)),
    Case(127, 128, 32, 7, 128, (32, 2, 2, 1)),
    Case(128, 132, 1, 7, 128, (32, 3, 1, 1)),
    Case(101, 192, 17, 7, 104, (32, 3, 2, 1)),
    Case(127, 196, 16, 7, 128, (32, 4, 1, 1)),
    Case(128, 64, 32, 7, 132, (32, 2, 2, 1)),      # Kc = 128 at the F the end-to-end test uses
]

# --- U loaded directly because ldu is no multiple of 4, every KS (odd and 2 mod 4)
CASES += [
    Case(52, 196, 16, 7, 53, (13, 4, 1, 0)),
    Case(72, 132, 17, 7, 74, (18, 3, 2, 0)),
    Case(100, 4, 1, 7, 101, (25, 2, 1, 0)),
    Case(127, 192, 32, 7, 127, (32, 3, 2, 0)),
    Case(1, 128, 16, 7, 1, (13, 2, 1, 0)),
]

# --- U loaded directly because its staged rows would take the block past 160 KiB (ldu a multiple of 4), every
# KS: S_T's nhub x F floats fill the budget.  Kc = 128, F = 256 leaves it with 7 hubs already; the other hub
# counts are the largest the entry point still accepts (one more hub is refused for LDS: asserted on the CPU).
BUDGET_CASES = [
    Case(52, 256, 16, 97, 52, (13, 4, 1, 0)),
    Case(72, 256, 17, 71, 72, (18, 4, 2, 0)),
    Case(100, 256, 32, 43, 100, (25, 4, 2, 0)),
    Case(73, 192, 16, 99, 76, (25, 3, 1, 0)),
    Case(128, 256, 17, 7, 128, (32, 4, 2, 0)),
    Case(128, 256, 1, 21, 128, (32, 4, 1, 0)),
]
LAST_HUB_CASES = [c for c in BUDGET_CASES if c.nhub != 7]
CASES += BUDGET_CASES
CASES += [
    Case(101, 196, 32, 7, 104, (32, 4, 2, 1)),     # KS 32, NTQ 4, NP 2 with U staged: what is left of 160 KiB
]

# --- refused for LDS: W1's 128 rows of 256 floats beside 40 hubs' S_T rows
LDS_REFUSED = (128, 256, 8, 40, 128)   # Kc, F, P, nhub, ldu
