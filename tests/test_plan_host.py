"""CPU checks of the SpMM plan builder (gcnk_spmm_plan_build_host: the same
host code the device build runs, writing into host memory): the row-unit +
tile plan's layout and its size query.  The kernels themselves are checked
on the GPU (tests/test_gpu_parity.py); the row-unit control logic by the
Python model in tests/path_model.py.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib
from graph_convolutional_networks_for_text_classification_amd.sparse import PLAN_MAGIC, PlanHeader
from oracle import csr_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def build_host_plan(rp, ci, v, shape, groups=1, ipc=12, dense=0.25):
    lib = _lib.load()
    M, K = shape
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    v = np.ascontiguousarray(v, np.float32)
    nnz = len(ci)
    nbytes = lib.gcnk_spmm_plan_bytes_host(rp.ctypes.data, ci.ctypes.data, M, K, nnz, ipc, groups, dense)
    assert nbytes > 0, lib.gcnk_last_error()
    buf = np.zeros(nbytes // 4, np.int32)
    rc = lib.gcnk_spmm_plan_build_host(rp.ctypes.data, ci.ctypes.data, v.ctypes.data, M, K, nnz, ipc, groups, dense,
                                       buf.ctypes.data, nbytes)
    assert rc == 0, lib.gcnk_last_error()
    return buf


def _doc_topic(rng, below, H, above, hub_deg, light_deg, hub_hub=0.2, empty_frac=0.05, no_diag_frac=0.05):
    """Square doc-topic-like operand: `below` light rows, H contiguous hub rows,
    `above` light rows; light rows = own diagonal + a few hub columns, hub rows =
    light columns + some hub columns (+ diagonal)."""
    M = below + H + above
    h0 = below
    hubs = np.arange(h0, h0 + H)
    light = np.concatenate([np.arange(below), np.arange(h0 + H, M)])
    rows, cols = [], []
    for r in light:
        if rng.random() < empty_frac:
            continue
        d = int(rng.integers(0, light_deg + 1))
        c = list(rng.choice(hubs, min(d, H), replace=False))
        if rng.random() >= no_diag_frac:
            c.append(r)
        rows += [r] * len(c)
        cols += c
    for r in hubs:
        c = list(rng.choice(light, min(len(light), hub_deg), replace=False))
        c += [x for x in hubs if rng.random() < hub_hub]
        rows += [r] * len(c)
        cols += c
    rows, cols = np.array(rows), np.array(cols)
    return csr_ref.coo_to_csr(rows, cols, rng.standard_normal(rows.size).astype(np.float32), (M, M))


def test_row_plan_layout():
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 2000, 20000)
    cols = rng.integers(0, 2000, 20000)
    rp, ci, v = csr_ref.coo_to_csr(rows, cols, rng.standard_normal(20000).astype(np.float32), (2000, 2000))
    plan = build_host_plan(rp, ci, v, (2000, 2000))
    hdr = PlanHeader(plan)
    assert hdr.magic == PLAN_MAGIC and hdr.M == 2000 and hdr.nnz == len(ci)
    rp, ci, v = _doc_topic(rng, 600, 12, 288, 500, 6)
    # items are packed {col, value bits} right after the header in CSR order
    plan = build_host_plan(rp, ci, v, (900, 900))
    assert PlanHeader(plan).magic == PLAN_MAGIC
    items = plan[16:16 + 2 * len(ci)].reshape(-1, 2)
    assert np.array_equal(items[:, 0], ci)
    assert np.array_equal(items[:, 1].view(np.float32), v.astype(np.float32))


def test_plan_rejects_bad_csr():
    lib = _lib.load()
    rp = np.array([0, 2, 1], np.int32)
    ci = np.array([0, 1], np.int32)
    n = lib.gcnk_spmm_plan_bytes_host(rp.ctypes.data, ci.ctypes.data, 2, 2, 2, 8, 1, 0.25)
    assert n == _lib.EARG and b"rowptr" in lib.gcnk_last_error()
    rp = np.array([0, 1, 2], np.int32)
    ci = np.array([0, 5], np.int32)
    n = lib.gcnk_spmm_plan_bytes_host(rp.ctypes.data, ci.ctypes.data, 2, 2, 2, 8, 1, 0.25)
    assert n == _lib.EARG and b"out of range" in lib.gcnk_last_error()


@pytest.mark.parametrize("kind", ["random", "mixed", "doc_topic"])
def test_plan_bytes_is_exactly_the_built_image(kind):
    """gcnk_spmm_plan_bytes_host sizes a row-unit plan from its header alone
    (no light-row sort, no image): the build must write exactly that many
    bytes -- none past them, the last one included."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(__file__))
    from test_gpu_parity import _mixed_density_csr, _random_csr
    lib = _lib.load()
    rng = np.random.default_rng(17)
    if kind == "mixed":
        rp, ci, v = _mixed_density_csr(rng, 900, 900)
        M = K = 900
    elif kind == "doc_topic":
        rp, ci, v = _doc_topic(rng, 2000, 30, 900, 400, 5)
        M = K = 2930
    else:
        M, K = 3001, 2003
        rp, ci, v = _random_csr(M, K, 20000, rng, heavy_rows=(5, 1700), heavy_deg=2500, empty_frac=0.2)
    rp, ci, v = (np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (v, np.float32)))
    nbytes = lib.gcnk_spmm_plan_bytes_host(rp.ctypes.data, ci.ctypes.data, M, K, len(ci), 12, 1, 0.25)
    assert nbytes > 0 and nbytes % 4 == 0
    buf = np.full(nbytes // 4 + 64, -7, np.int32)
    rc = lib.gcnk_spmm_plan_build_host(rp.ctypes.data, ci.ctypes.data, v.ctypes.data, M, K, len(ci), 12, 1, 0.25,
                                       buf.ctypes.data, buf.nbytes)
    assert rc == 0, lib.gcnk_last_error()
    assert PlanHeader(buf).magic == PLAN_MAGIC
    assert np.all(buf[nbytes // 4:] == -7), "the build wrote past the size plan_bytes reported"
    # no plan word is -7 (ids >= -1, counts >= 0, float bits of -7 would be a NaN),
    # so a sentinel left in the last reported word means the size was too large
    assert buf[nbytes // 4 - 1] != -7, "plan_bytes reported more than the build wrote"


# ---------------------------------------------------------------------------
# Plan images pinned by digest.  The inputs come from integer arithmetic (and
# the R8 golden graph), never from a random-number library's stream.

def _csr_of(rows):
    """CSR of per-row column lists (order kept; values k -> ((7919 k) % 1009 - 504) / 64, exact in fp32)."""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate(rows).astype(np.int32) if rp[-1] else np.zeros(0, np.int32)
    k = np.arange(len(ci), dtype=np.int64)
    return rp, ci, (((k * 7919) % 1009 - 504) / 64.0).astype(np.float32)


def _boundary_rows():
    """4096 x 4096, no tile block.  Row 0: 2048 nonzeros spread evenly over the 8
    column classes (8 runs of 256: 64 segments of 32 at groups 1, ipc 8); row 1:
    one more in the last class (65 segments: a top entry); rows 2-13: degrees at
    and one past every light-row limit of the crossed (groups, ipc); row 14:
    unsorted columns whose classes alternate (one run, dealt round-robin); row
    15 empty; the rest light rows of a diagonal and two more columns."""
    N = 4096
    ev = np.arange(0, N, 2)
    rows = [ev, np.append(ev, N - 1)]
    for i, d in enumerate((8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 64, 65)):
        rows.append(np.sort(((i + 2) * 37 + 61 * np.arange(d)) % N))
    j = np.arange(300)
    rows.append((j % 2) * 2048 + j)
    rows.append(np.zeros(0, np.int64))
    for r in range(16, N):
        rows.append(np.unique([r, (r * 7) % N, (r * 13 + 5) % N]))
    return _csr_of(rows) + (N, N)


def _tile_blocks():
    """512 x 512.  Three 64-row blocks dense enough for the tile path: 50
    contiguous columns (one chunk), 200 columns (four chunks: a reduce entry), 40
    even columns (one chunk with a column list), each row with its diagonal kept
    aside; then diagonal-only rows and all-empty rows."""
    rows = [np.unique(np.append(np.arange(256, 306), r)) for r in range(64)]
    rows += [np.unique(np.append(np.arange(128, 328), r)) for r in range(64, 128)]
    rows += [np.unique(np.append(2 * np.arange(40), r)) for r in range(128, 192)]
    rows += [np.array([r]) for r in range(192, 400)]
    rows += [np.zeros(0, np.int64)] * 112
    return _csr_of(rows) + (512, 512)


def _rect_long_row():
    """5 x 140000, rectangular.  Row 0 holds every column: 8 runs of 17500, 4376
    segments of 32 at groups 1, ipc 8 -- past 64 * 64, so the segment length
    doubles; an empty row, a 3-nonzero row, 70 unsorted columns, one nonzero."""
    K = 140000
    j = np.arange(70)
    rows = [np.arange(K), np.zeros(0, np.int64), np.array([5, 70000, 139999]), (j % 2) * 70000 + (69 - j) * 3,
            np.array([0])]
    return _csr_of(rows) + (5, K)


def _digest_cases():
    with np.load(os.path.join(GOLDEN, "r8_graph.npz")) as z:
        n = int(max(z["adj_row"].max(), z["adj_col"].max())) + 1
        rp, ci, v = csr_ref.coo_to_csr(z["adj_row"], z["adj_col"], z["adj_val"], (n, n))
    yield ("r8_adj", rp.astype(np.int32), ci.astype(np.int32), v.astype(np.float32), n, n)
    yield ("boundary_rows",) + _boundary_rows()
    yield ("tile_blocks",) + _tile_blocks()
    yield ("rect_long_row",) + _rect_long_row()
    yield ("no_rows", np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 7)
    yield ("no_nonzeros", np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 3)


def plan_digests(lib):
    """{case: sha256 of the plan image} and {case: header} over the matrices x
    groups x ipc x dense_threshold, checking the size query on the way."""
    digests, headers = {}, {}
    for name, rp, ci, v, M, K in _digest_cases():
        rp, ci, v = (np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (v, np.float32)))
        for groups in (1, 2, 8, 32, 64):
            for ipc in (8, 12, 32):
                for dense in (0.25, 2.0):
                    nbytes = lib.gcnk_spmm_plan_bytes_host(rp.ctypes.data, ci.ctypes.data, M, K, len(ci), ipc, groups,
                                                           dense)
                    assert nbytes >= 64 and nbytes % 4 == 0, lib.gcnk_last_error()
                    buf = np.full(nbytes // 4 + 16, -7, np.int32)
                    rc = lib.gcnk_spmm_plan_build_host(rp.ctypes.data, ci.ctypes.data, v.ctypes.data, M, K, len(ci),
                                                       ipc, groups, dense, buf.ctypes.data, buf.nbytes)
                    assert rc == 0, lib.gcnk_last_error()
                    key = f"{name}/groups{groups}/ipc{ipc}/dense{dense}"
                    # plan_bytes is exactly the image: nothing written past it, its last word written
                    assert np.all(buf[nbytes // 4:] == -7) and buf[nbytes // 4 - 1] != -7, key
                    digests[key] = hashlib.sha256(buf[:nbytes // 4].tobytes()).hexdigest()
                    headers[key] = PlanHeader(buf[:16].copy())
    return digests, headers


def test_plan_images_match_recorded_digests():
    """The planner's output is a byte contract: every plan image equals, by
    SHA-256, the one recorded in golden/plan_digests.json (recorded from the
    library as it was before the planner moved out of spmm.hip)."""
    digests, headers = plan_digests(_lib.load())
    # the matrices reach the branches they are meant to
    h = headers["tile_blocks/groups1/ipc12/dense0.25"]
    assert h.ntile == 6 and h.nsingle == 2 and h.nred == 1 and h.ntblk == 3 and h.has_diag
    assert headers["tile_blocks/groups1/ipc12/dense2.0"].ntile == 0
    h = headers["boundary_rows/groups1/ipc8/dense0.25"]
    assert h.ntile == 0 and h.has_tops and h.segp > 0 and h.nheavy > 0 and not h.has_diag
    assert not headers["boundary_rows/groups1/ipc32/dense0.25"].has_tops
    h = headers["boundary_rows/groups8/ipc8/dense0.25"]
    assert h.segp == 0 and h.nhunits > 0, "padded heavy items only for whole-wavefront groups"
    h = headers["rect_long_row/groups1/ipc8/dense0.25"]
    assert h.has_tops and h.segp == 64, "past 64 * 64 segments of 32 the segment length doubles"
    assert headers["r8_adj/groups1/ipc12/dense0.25"].nheavy > 0
    h = headers["no_rows/groups1/ipc8/dense0.25"]
    assert h.M == 0 and h.nunits == 0
    assert headers["no_nonzeros/groups64/ipc32/dense2.0"].nnz == 0
    with open(os.path.join(GOLDEN, "plan_digests.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(digests)
    wrong = [k for k in want if want[k] != digests[k]]
    assert not wrong, f"{len(wrong)} plan images changed, e.g. {wrong[:3]}"



def test_power_law_hub_keeps_short_segments_two_levels():
    """on an R-MAT graph whose hub rows hold ~10^4
    nonzeros the plan keeps every heavy segment at the base length (ipc x the
    workgroup's lane groups; it used to double it past 64 segments) and gives
    such a row a top heavy entry (.w = -2) over groups of <= 64 segments, each
    group's .w the top's slot for its sum; no heavy entry
    has more than 64 slots, slots never overlap, and the units cover every
    nonzero of the heavy rows exactly once."""
    from graph_convolutional_networks_for_text_classification_amd import datasets
    rp, ci, v = (t.numpy() for t in datasets.rmat_csr(16, 1_300_000, seed=2))
    n = len(rp) - 1
    ipc, groups = 12, 1                      # whole-wavefront groups (F > 128): 4-wave segments
    plan = build_host_plan(rp, ci, v, (n, n), groups=groups, ipc=ipc, dense=2.0)
    hdr = PlanHeader(plan)
    nnz, nunits, nh, nheavy = hdr.nnz, hdr.nunits, hdr.nhunits, hdr.nheavy
    units = plan[16 + 2 * nnz:16 + 2 * nnz + 4 * nunits].reshape(-1, 4)
    heavy = plan[16 + 2 * nnz + 4 * nunits:16 + 2 * nnz + 4 * nunits + 4 * nheavy].reshape(-1, 4)
    seg = ipc * 4
    deg = np.diff(rp)
    hub = int(np.argmax(deg))
    assert deg[hub] > 64 * seg
    hu = units[:nh][units[:nh, 0] == hub]
    assert len(hu) > 64 and (hu[:, 2] - hu[:, 1]).max() <= seg
    assert (heavy[:, 2] <= 64).all() and (heavy[:, 2] >= 1).all()
    assert hdr.has_tops, "the plan flags its two-level rows"
    tops = heavy[(heavy[:, 0] == hub) & (heavy[:, 3] == -2)]
    assert len(tops) == 1 and tops[0, 2] > 1
    groups_of_hub = heavy[(heavy[:, 0] == hub) & (heavy[:, 3] >= 0)]
    assert len(groups_of_hub) == tops[0, 2]
    assert groups_of_hub[:, 3].tolist() == list(range(tops[0, 1], tops[0, 1] + tops[0, 2]))
    assert groups_of_hub[:, 2].sum() == len(hu)
    slots = np.concatenate([np.arange(h[1], h[1] + h[2]) for h in heavy])
    assert len(np.unique(slots)) == len(slots) == hdr.nslots
    for r in np.unique(units[:nh, 0][units[:nh, 0] >= 0])[:200]:
        u = units[:nh][units[:nh, 0] == r]
        got = np.sort(np.concatenate([np.arange(a, b) for a, b in u[:, 1:3]]))
        assert np.array_equal(got, np.arange(rp[r], rp[r + 1]))
