"""The SpMM case table (tests/spmm_cases.py) against the route report, on the CPU.

gcnk_spmm_route -- the host function the launches of gcnk_spmm_csr_f32,
gcnk_spmm_csr_f32_part and gcnk_spmm_proj_f32 switch on -- says what each case
launches, from a plan header built on the host (gcnk_spmm_plan_build_host):
each case must reach the route it names on a plan that still holds the row
kinds it is there for, and the table every reachable instantiation the library
compiles (so a moved threshold or a planner change cannot orphan one
unnoticed); the seven conditions of the float4 path, the column-window count,
the O32 edge and the refusals.  tests/test_spmm_routes.py runs the same cases
on the GPU.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmm_cases as sc  # noqa: E402

import gcn_amd  # noqa: E402,F401
from graph_convolutional_networks_for_text_classification_amd import _lib  # noqa: E402
from graph_convolutional_networks_for_text_classification_amd.sparse import PlanHeader  # noqa: E402

from test_plan_host import build_host_plan  # noqa: E402

ALIGN_BIT = {"b_base": _lib.SPMM_ALIGNED_B, "c_base": _lib.SPMM_ALIGNED_C, "bias_base": _lib.SPMM_ALIGNED_BIAS,
             "ws_base": _lib.SPMM_ALIGNED_WORKSPACE}


def groups_of(c):
    return int(_lib.load().gcnk_spmm_groups(c.F, c.lanes))


def ipc_of(c):
    rp, ci, _, (M, _K) = sc.operand(c.operand)
    return c.ipc or int(_lib.load().gcnk_spmm_default_ipc(M, len(ci), c.F, c.lanes))


@functools.lru_cache(maxsize=None)
def _host_header(operand, ipc, groups, dense):
    rp, ci, v, shape = sc.operand(operand)
    return build_host_plan(rp, ci, v, shape, groups=groups, ipc=ipc, dense=dense)[:16].copy()


def _header(c):
    return _host_header(c.operand, ipc_of(c), groups_of(c), c.dense)


def _query(hdr, F, ldb, ldc, aligned=_lib.SPMM_ALIGNED_ALL, lanes=0, P=0, part=0):
    out = (ctypes.c_int32 * 16)(*([-1] * 16))
    rc = _lib.load().gcnk_spmm_route(hdr.ctypes.data if hdr is not None else None, F, ldb, ldc, aligned, lanes, P,
                                     part, out)
    return rc, tuple(out)


def _route(c, part=0):
    aligned = _lib.SPMM_ALIGNED_ALL & ~ALIGN_BIT.get(c.misalign, 0)
    rc, out = _query(_header(c), c.F, c.F + c.pad_b, c.F + c.pad_c, aligned, c.lanes, c.P, part)
    assert rc == _lib.OK, _lib.load().gcnk_last_error()
    assert out[14:] == (0, 0)
    return out[:14]


def test_route_refuses_bad_arguments():
    lib = _lib.load()
    c = sc.VEC4_BASE
    hdr = _header(c)
    good = dict(hdr=hdr, F=c.F, ldb=c.F, ldc=c.F)
    assert _query(**good)[0] == _lib.OK
    assert lib.gcnk_spmm_route(hdr.ctypes.data, c.F, c.F, c.F, 15, 0, 0, 0, None) == _lib.EARG
    assert b"gcnk_spmm_route" in lib.gcnk_last_error()
    for bad in (dict(hdr=None), dict(hdr=np.zeros(16, np.int32)), dict(F=-1), dict(ldb=c.F - 1), dict(ldc=c.F - 1),
                dict(part=3), dict(part=-1), dict(P=-1)):
        rc, out = _query(**{**good, **bad})
        assert rc == _lib.EARG and out == (0,) * 16, bad
    # nothing to do, nothing launched: F = 0, and an operand of no rows
    assert _query(**{**good, "F": 0, "ldb": 0, "ldc": 0}) == (_lib.OK, (0,) * 16)
    empty = build_host_plan(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), (0, 7))[:16].copy()
    assert _query(empty, 8, 8, 8) == (_lib.OK, (0,) * 16)


@pytest.mark.parametrize("case", sc.ALL_CASES, ids=lambda c: c.name)
def test_case_reaches_the_route_it_names(case):
    c = case
    assert _route(c) == c.route
    assert c.misalign in sc.MISALIGN and c.F + c.pad_b >= c.F and (c.P == 0 or not c.two_part)
    h = PlanHeader(_header(c))
    M = sc.operand(c.operand)[3][0]
    assert h.groups == 64 // c.route[1] and h.has_tops == c.tops
    # the plan still holds the row kinds the case is there for
    assert h.nunits - h.nhunits >= (M if c.dense > 1 else 1), "light units"
    if c.operand.startswith("T"):
        assert 0 < h.nsingle < h.ntile and h.nred > 0 and h.has_diag == (M == 900)
        # the two-part launch: the single-chunk tile blocks, then everything else
        one, two = _route(c, 1), _route(c, 2)
        assert one == sc.NO_ROWS + c.route[8:13] + (0,) and two == c.route
    else:
        assert h.ntile == 0 and not h.has_diag
        assert h.nhunits > 0 and h.nheavy >= 2 and h.nslots >= 2 * h.nheavy, "heavy units, two multi-segment heavy rows"
        assert (h.segp > 0) == (c.route[1] == 64), "padded heavy items: whole-wavefront groups only"


def _reached():
    got = {}
    for c in sc.ALL_CASES:
        for inst in sc.instantiations_of(_route(c)):
            got.setdefault((inst, c.tag), []).append(c.name)
    return got


def test_table_reaches_every_instantiation():
    """The instantiation list of csrc/spmm.hip (the comment block above
    spmm_route), mirrored by spmm_cases.INSTANTIATIONS: a case for each entry
    and nothing reached that the list does not know.  REQUIRED pairs each
    instantiation with what a case runs it for; every pair has exactly one
    case, so taking any case out of the table orphans a pair."""
    got = _reached()
    insts = {k[0] for k in got}
    missing = [i for i in sc.INSTANTIATIONS if i not in insts]
    assert not missing, f"no case reaches {missing}"
    unknown = sorted(insts - set(sc.INSTANTIATIONS))
    assert not unknown, f"routes outside the instantiation list: {unknown}"
    assert not insts & set(sc.UNREACHABLE)
    orphans = [k for k in sc.REQUIRED if k not in got]
    assert not orphans, f"no case reaches {orphans}"
    assert {k[0] for k in sc.REQUIRED} | {("reduce",)} == set(sc.INSTANTIATIONS)
    for c in sc.ALL_CASES:   # every case is the only one of a pair
        mine = [k for k, names in got.items() if names == [c.name] and k in sc.REQUIRED]
        assert mine, f"{c.name} reaches nothing the table needs it for"
    # the list itself: 7 LPR x 2 VEC x 2 O32, 3 LPR x 2 NP x 2 O32, 2 top kernels, 2 VEC4 x 3 NT x 2 DIAG, the reduce
    assert len(set(sc.INSTANTIATIONS)) == len(sc.INSTANTIATIONS) == 28 + 12 + 2 + 12 + 1
    assert len(set(sc.REQUIRED)) == len(sc.REQUIRED)


def test_each_vec4_condition_alone_takes_the_scalar_kernel():
    base = sc.VEC4_BASE
    assert _route(base)[2] == 4 and base.misalign == "" and (base.F % 4, base.pad_b % 4, base.pad_c % 4) == (0, 0, 0)
    seen = set()
    for what, c in sc.VEC4_VIOLATIONS.items():
        # the seven conditions of spmm_route's vec4, each by itself
        violated = {"F % 4": c.F % 4 != 0, "ldb % 4": (c.F + c.pad_b) % 4 != 0, "ldc % 4": (c.F + c.pad_c) % 4 != 0,
                    "B base": c.misalign == "b_base", "C base": c.misalign == "c_base",
                    "bias base": c.misalign == "bias_base", "workspace base": c.misalign == "ws_base"}
        assert [k for k, v in violated.items() if v] == [what]     # violated alone
        diff = {f for f in c._fields if getattr(c, f) != getattr(base, f)} - {"route", "tag"}
        assert diff == ({"F", "pad_b", "pad_c"} if what == "F % 4" else
                        {"misalign"} if what.endswith("base") else {"pad_" + what[2]}), (what, diff)
        assert _route(c)[:4] == (1, 64, 1, 0), what
        seen.add(what)
    assert len(seen) == 7
    # the mask's four bits, one by one
    hdr = _header(base)
    for bit in (1, 2, 4, 8):
        assert _query(hdr, base.F, base.F, base.F, _lib.SPMM_ALIGNED_ALL & ~bit)[1][2] == 1
    # F % 4 alone, and F % 4 == 0 with nothing else violated, at every LPR and on the tile path
    for lanes in sc.LPRS:
        h = _host_header("R", 4, 64 // lanes, 2.0)
        assert _query(h, 4 * lanes + 2, 4 * lanes + 4, 4 * lanes + 8, lanes=lanes)[1][1:3] == (lanes, 1)
        assert _query(h, 4 * lanes, 4 * lanes + 4, 4 * lanes + 8, lanes=lanes)[1][1:3] == (lanes, 4)
    t = sc.TILE_CASES[0]
    for F, v4 in ((18, 0), (20, 1)):
        c = t._replace(F=F, pad_b=20 - F + 4, pad_c=20 - F + 8)
        out = _query(_header(c), F, F + c.pad_b, F + c.pad_c)[1]
        assert (F + c.pad_b) % 4 == 0 and (F + c.pad_c) % 4 == 0 and out[8:10] == (1, v4) and out[2] == (4 if v4 else 1)


def test_column_window_count():
    """ceil(ceil(F / (LPR VEC)) / 64) launches: 64 tiles, 65 tiles, three windows, and a sweep."""
    for lanes, vec, F, want in ((1, 1, 64, 1), (1, 1, 65, 2), (1, 1, 130, 3), (64, 4, 16384, 1), (64, 4, 16388, 2),
                                (64, 1, 4096, 1), (64, 1, 4097, 2), (1, 4, 256, 1), (1, 4, 260, 2), (8, 4, 4100, 3)):
        hdr = _host_header("R", 4, 64 // lanes, 2.0)
        ld = F + (4 if vec == 4 else 1)
        rc, out = _query(hdr, F, ld, ld, lanes=lanes)
        assert rc == _lib.OK and out[1:3] == (lanes, vec) and out[4] == want, (lanes, vec, F, out)
    for lanes in sc.LPRS:
        hdr = _host_header("R", 4, 64 // lanes, 2.0)
        for F in range(1, 70 * lanes * 4, 37):
            out = _query(hdr, F, F, F, lanes=lanes)[1]
            tiles = -(-F // (lanes * out[2]))
            assert out[2] == (4 if F % 4 == 0 else 1) and out[4] == -(-tiles // 64), (lanes, F)


def test_o32_flips_exactly_at_4_gib():
    """O32 iff K ldb 4 + Fw 4 < 2^32 (Fw: the window's columns)."""
    K = sc.BIG_K["lo"]
    hdr = _host_header("BIG_lo", 4, 1, 2.0)
    assert PlanHeader(hdr).K == K
    for F, ldb, want in ((1023, 1024, 1), (1024, 1024, 0), (1020, 1024, 1), (4, 1025, 0)):
        assert (K * ldb * 4 + F * 4 < 2**32) == bool(want)
        out = _query(hdr, F, ldb, F, lanes=64)[1]
        assert out[4:7] == (1, want, want), (F, ldb, out)
    for which in ("edge", "hi"):
        out = _query(_host_header("BIG_" + which, 4, 1, 2.0), 4, sc.BIG_LDB, 4, lanes=64)[1]
        assert out[5:7] == (0, 0)
    # the band where the windows differ: the first window (64 columns) reaches 2^32, the last (1 column) does not
    one = build_host_plan(np.array([0, 1], np.int32), np.array([63], np.int32), np.ones(1, np.float32), (1, 64),
                          groups=64, ipc=4, dense=2.0)[:16].copy()
    ldb = 2**24 - 1
    assert 64 * ldb * 4 + 64 * 4 == 2**32
    out = _query(one, 65, ldb, 65, lanes=1)[1]
    assert out[:7] == (1, 1, 1, 0, 2, 0, 1) and sc.instantiations_of(out) == {("row", 1, 1, 0), ("row", 1, 1, 1)}


def test_refusals_are_reported_as_the_launch_reports_them():
    lib = _lib.load()
    r64 = _host_header("R", 12, 1, 2.0)            # lanes 64, no top entry
    assert _query(r64, 200, 200, 200, lanes=64, P=8) == (_lib.OK, sc.rows(64, 4, np_=8) + sc.NO_TILE + (0, 0))
    t = _host_header("T700", ipc_of(sc.TILE_CASES[0]._replace(F=200, lanes=64)), 1, 0.25)
    assert PlanHeader(t).ntile > 0
    for what, q in (("tile chunks", dict(hdr=t, F=200, lanes=64, P=8)),
                    ("a top entry", dict(hdr=_host_header("R", 4, 1, 2.0), F=200, lanes=64, P=8)),
                    ("P = 33", dict(hdr=r64, F=200, lanes=64, P=33)),
                    ("F > 4 LPR", dict(hdr=_host_header("R", 4, 4, 2.0), F=68, lanes=16, P=8)),
                    ("F > 4 LPR at 64 lanes", dict(hdr=r64, F=260, lanes=64, P=8)),
                    ("LPR < 16", dict(hdr=_host_header("R", 4, 8, 2.0), F=32, lanes=8, P=8)),
                    ("not float4", dict(hdr=r64, F=200, lanes=64, P=8, aligned=_lib.SPMM_ALIGNED_ALL & ~1))):
        rc, out = _query(ldb=q["F"], ldc=q["F"], **q)
        assert rc == _lib.EUNSUP and out == (0,) * 16, what
        assert b"gcnk_spmm_proj_f32" in lib.gcnk_last_error(), what
    # a plan built for another group count
    rc, out = _query(_host_header("R", 4, 4, 2.0), 64, 64, 64, lanes=32)
    assert rc == _lib.EARG and out == (0,) * 16 and b"lane groups" in lib.gcnk_last_error()
    assert PlanHeader(_host_header("R", 4, 1, 2.0)).has_tops and not PlanHeader(r64).has_tops
