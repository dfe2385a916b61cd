"""The hub-factor block record, packed by hand for the tests (test infrastructure, no GPU import).

Layout (csrc/hub_block.h): per 32-row block of the block order, rec_words int32 words --
33 block-relative item offsets, 3 pad words, 32 output row ids with -1 past M, then the rows'
items in order, two words each: {hub index, fp32 value bits}.  rec_words is the common stride,
a multiple of 4.  tests/test_hub_records.py pins the constants to factor.py's and this packer
to oracle/factor_host.py's records.
"""
import numpy as np

ROWS, REC_ROW, REC_HEAD = 32, 36, 68


def rec_words_for(counts, tail=0):
    """The shortest stride for `counts` items per position (a multiple of ROWS positions), plus `tail` spare words."""
    per_block = np.asarray(counts).reshape(-1, ROWS).sum(1)
    return (REC_HEAD + 2 * int(per_block.max()) + 3) // 4 * 4 + tail


def pack(items_per_position, perm, M, rec_words, fill=0):
    """The [nblk x rec_words] int32 records of M rows: position p of the block order holds
    output row perm[p] and the items items_per_position[p], a sequence of (hub, value) pairs
    (positions past M, or past the sequence's end, hold nothing).  Items that do not fit in
    rec_words are dropped from the block's end, as the device writer drops them; the offsets
    still count them.  Every word after a block's items is `fill`."""
    nblk = (M + ROWS - 1) // ROWS
    rec = np.full((nblk, rec_words), fill, np.int32)
    for b in range(nblk):
        rows = [list(items_per_position[p]) if p < min(M, len(items_per_position)) else []
                for p in range(b * ROWS, (b + 1) * ROWS)]
        rec[b, :ROWS + 1] = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        rec[b, ROWS + 1:REC_ROW] = 0
        real = min(ROWS, M - b * ROWS)
        rec[b, REC_ROW:REC_ROW + real] = perm[b * ROWS:b * ROWS + real]
        rec[b, REC_ROW + real:REC_HEAD] = -1
        flat = [it for r in rows for it in r][:(rec_words - REC_HEAD) // 2]
        rec[b, REC_HEAD:REC_HEAD + 2 * len(flat):2] = [h for h, _ in flat]
        rec[b, REC_HEAD + 1:REC_HEAD + 2 * len(flat):2] = np.array([v for _, v in flat], np.float32).view(np.int32)
    return rec
