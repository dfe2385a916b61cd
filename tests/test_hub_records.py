"""tests/hub_records.py against the other statements of the hub-factor block record (CPU only):
its constants equal factor.py's and oracle/factor_host.py's, and pack() reproduces the oracle's
records word for word on small doc-topic graphs -- M = 64 (two full blocks) and M = 70 with 5 hubs
(three blocks, the last with 6 real rows; a row with no hub item; a hub row holding every hub column).
A graph of one row has no hub, so the oracle builds no factor for M = 1: that record is checked
against the layout word by word."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hub_records as hr  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import factor  # noqa: E402
from graph_convolutional_networks_for_text_classification_amd.sparse import from_arrays  # noqa: E402
from oracle import factor_host  # noqa: E402

HUBS = {64: [3, 20, 41, 50, 63], 70: [3, 20, 41, 64, 69]}
FULL = 41                      # the hub row that holds every hub column


def test_constants_are_the_packages_and_the_oracles():
    assert (hr.ROWS, hr.REC_ROW, hr.REC_HEAD) == (factor.ROWS_PER_BLOCK, factor.REC_ROW, factor.REC_HEAD)
    assert (hr.ROWS, hr.REC_ROW, hr.REC_HEAD) == (factor_host.ROWS_PER_BLOCK, factor_host.REC_ROW,
                                                  factor_host.REC_HEAD)
    assert hr.REC_ROW >= hr.ROWS + 1 and hr.REC_ROW % 4 == 0 and hr.REC_HEAD == hr.REC_ROW + hr.ROWS


def _graph(M):
    """Rows [(column, value)] of an A-hat-like matrix: hub rows of 64 or more columns, a light row its
    diagonal and 0, 1 or 2 hub columns; and an X whose light rows use columns 2 .. 5."""
    rng = np.random.default_rng(M)
    hubs = HUBS[M]
    lights = [r for r in range(M) if r not in hubs]
    rows = []
    for r in range(M):
        if r in hubs:
            keep = hubs if r == FULL or M == 64 else [r]      # (M = 64: a hub row is every column)
            cols = sorted(set(keep) | set(rng.choice(lights, size=64 - len(keep), replace=False).tolist()))
        else:
            cols = sorted({r} | set(rng.choice(hubs, size=r % 3, replace=False).tolist()))
        rows.append([(c, np.float32(rng.uniform(0.1, 1.0))) for c in cols])
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    colind = np.array([c for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], np.float32)
    A = from_arrays(rowptr, colind, val, (M, M), "cpu")
    xc = np.tile(np.arange(2, 6, dtype=np.int32), M)
    X = from_arrays(np.arange(0, 4 * M + 1, 4, dtype=np.int32), xc, rng.standard_normal(4 * M).astype(np.float32),
                    (M, 9), "cpu")
    return rows, A, types.SimpleNamespace(csr=X, dense=None, shape=(M, 9))


@pytest.mark.parametrize("M", [64, 70])
def test_pack_reproduces_the_oracles_records(M):
    rows, A, xop = _graph(M)
    f = factor_host.build(A, xop)
    assert f is not None and f.hubs.tolist() == HUBS[M] and f.nblk == (M + hr.ROWS - 1) // hr.ROWS
    hub_index = {h: j for j, h in enumerate(HUBS[M])}
    items = [[(hub_index[c], v) for c, v in rows[r] if c in hub_index] for r in f.perm]
    counts = [len(it) for it in items]
    assert 0 in counts and counts[f.perm.tolist().index(FULL)] == 5      # a row with no hub item, the long list
    assert f.rec_words == hr.rec_words_for(counts + [0] * (hr.ROWS * f.nblk - M))
    rec = hr.pack(items, f.perm, M, f.rec_words)
    assert rec.dtype == f.rec.dtype == np.int32 and np.array_equal(rec, f.rec)
    real = (f.rec[:, hr.REC_ROW:hr.REC_HEAD] >= 0).sum(1).tolist()
    assert real == ([hr.ROWS, hr.ROWS] if M == 64 else [hr.ROWS, hr.ROWS, 6])


def test_pack_one_row():
    """M = 1: one block with one real row.  (The oracle refuses the graph: a single row is no hub.)"""
    A = from_arrays(np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1, np.float32), (1, 1), "cpu")
    assert factor_host.build(A, types.SimpleNamespace(csr=A, dense=None, shape=(1, 1))) is None
    words = hr.REC_HEAD + 8
    rec = hr.pack([[(2, np.float32(0.5)), (0, np.float32(-1.0))]], np.array([0]), 1, words, fill=-7)
    assert rec.shape == (1, words) and rec.dtype == np.int32
    want = np.full(words, -7, np.int32)
    want[0], want[1:hr.ROWS + 1], want[hr.ROWS + 1:hr.REC_ROW] = 0, 2, 0      # offsets (every later row: empty) | pad
    want[hr.REC_ROW], want[hr.REC_ROW + 1:hr.REC_HEAD] = 0, -1                # row ids
    want[hr.REC_HEAD:hr.REC_HEAD + 4] = [2, np.float32(0.5).view(np.int32), 0, np.float32(-1.0).view(np.int32)]
    assert np.array_equal(rec[0], want)
    # the shortest record: no item, head only
    assert np.array_equal(hr.pack([[]], np.array([0]), 1, hr.REC_HEAD)[0, :hr.REC_ROW], np.zeros(hr.REC_ROW, np.int32))
