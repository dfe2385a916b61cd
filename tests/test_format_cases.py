"""The sparse-format and metrics case tables (tests/format_cases.py), on the CPU.

Before tests/test_format_kernels.py holds the kernels to the references bit for bit, the references
are held to what they restate -- ATen's coalesce, scipy's normalisation (oracle/gcn_ref.py) and the
reference's own outputs (tests/golden), torch.max, the reference's macro_f1 -- and the cases to what
they are in the table for: a case that pins a summation order gives other bits in another order, a
key-width case has keys of the stated width, an edge case sits on its edge.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import format_cases as fc  # noqa: E402

from oracle import csr_ref, gcn_ref  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------ COO -> CSR

@pytest.mark.parametrize("name", [n for n, c in fc.coo_cases().items() if c["max_run"] <= 2])
def test_coo_reference_equals_aten_coalesce(name):
    """Runs of at most 2 (a + b = b + a): ATen's CPU coalesce defines every bit."""
    c = fc.coo_cases()[name]
    M, K = c["shape"]
    rp, ci, v = fc.coo_to_csr_f32(c["rows"], c["cols"], c["vals"], c["shape"])
    t = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([c["rows"], c["cols"]])), torch.from_numpy(c["vals"]),
                                (M, K)).coalesce()
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(t.indices()[0].numpy(), minlength=M))]))
    assert np.array_equal(ci, t.indices()[1].numpy())
    assert np.array_equal(_bits(v), _bits(t.values().numpy()))


@pytest.mark.parametrize("name", list(fc.coo_cases()) + ["after-bad"])
def test_coo_reference_pattern_equals_oracle(name):
    c = fc.coo_valid_case() if name == "after-bad" else fc.coo_cases()[name]
    rp, ci, v = fc.coo_to_csr_f32(c["rows"], c["cols"], c["vals"], c["shape"])
    rp64, ci64, v64 = csr_ref.coo_to_csr(c["rows"], c["cols"], c["vals"], c["shape"])
    assert np.array_equal(rp, rp64) and np.array_equal(ci, ci64)
    assert len(rp) == c["shape"][0] + 1 and rp[-1] == len(ci) == len(v)
    if len(v):   # and the values are the float64 sums to within the runs' fp32 rounding
        mag = csr_ref.coo_to_csr(c["rows"], c["cols"], np.abs(c["vals"]), c["shape"])[2]
        assert np.all(np.abs(v - v64) <= c["max_run"] * 2.0**-24 * mag)


def test_coo_cases_are_what_the_table_says():
    cases = fc.coo_cases()
    w = cases["wide"]
    M, K = w["shape"]
    assert (M * K).bit_length() == 33 and fc.max_key_bits(w) == 33
    keys = w["rows"] * K + w["cols"]
    assert (keys >= 2**32).sum() > 100 and len(np.unique(keys & 0xFFFFFFFF)) <= len(np.unique(keys))
    assert {(0, 0), (0, K - 1), (M - 1, 0), (M - 1, K - 1)} <= set(zip(w["rows"].tolist(), w["cols"].tolist()))
    assert len(keys) - len(np.unique(keys)) == 1000
    # a sort by the low 32 bits alone gives another order
    assert not np.array_equal(np.argsort(keys, kind="stable"), np.argsort(keys & 0xFFFFFFFF, kind="stable"))
    for name, mk, bits in (("pow2-256x256", 2**16, 16), ("pow2-1x65537", 2**16 + 1, 17)):
        c = cases[name]
        M, K = c["shape"]
        assert M * K == mk and fc.max_key_bits(c) == bits
        assert (c["rows"] * K + c["cols"]).max() == M * K - 1, "the largest key is used"
    assert cases["vec-K1"]["shape"][1] == 1 and cases["vec-M1"]["shape"][0] == 1
    assert len(cases["vec-nnz1"]["vals"]) == 1 and len(cases["vec-nnz0"]["vals"]) == 0
    assert np.array_equal(fc.coo_to_csr_f32([], [], [], (10, 4))[0], np.zeros(11, np.int64))
    # one_run: its 300 entries cover sorted positions 100..399, across the 256-thread boundary
    c = cases["one_run"]
    order = np.lexsort((c["cols"], c["rows"]))
    at = [k for k, i in enumerate(order) if (c["rows"][i], c["cols"][i]) == fc.ONE_RUN_AT]
    assert at == list(range(fc.ONE_RUN_BEFORE, fc.ONE_RUN_BEFORE + fc.ONE_RUN_LEN)) and at[0] < 256 < at[-1]
    assert set(np.abs(c["vals"][order[at]]).tolist()) == {1e8, 1.0}
    # runs: every length 1..7
    c = cases["runs"]
    _, counts = np.unique(c["rows"] * c["shape"][1] + c["cols"], return_counts=True)
    assert set(counts.tolist()) == set(range(1, 8)) and c["shape"] == (400, 300)
    # empty_rows: 70 leading, 300 in the middle, 70 trailing
    c = cases["empty_rows"]
    deg = np.diff(fc.coo_to_csr_f32(c["rows"], c["cols"], c["vals"], c["shape"])[0])
    assert not deg[:70].any() and not deg[-70:].any() and not deg[150:450].any()
    assert deg[70:150].all() and deg[450:530].all()
    for name, c in cases.items():
        _, counts = np.unique(c["rows"] * c["shape"][1] + c["cols"], return_counts=True)
        assert (counts.max() if len(counts) else 0) == c["max_run"], name
    # the bad entries are outside the shape, one each, among valid ones
    M, K = fc.BAD_SHAPE
    for which in fc.BAD_ENTRIES:
        c = fc.coo_bad_case(which)
        out = (c["rows"] < 0) | (c["rows"] >= M) | (c["cols"] < 0) | (c["cols"] >= K)
        assert out.sum() == 1 and 0 < np.flatnonzero(out)[0] < len(out) - 1, which


@pytest.mark.parametrize("name", ["one_run", "runs", "mixed"])
def test_order_cases_have_teeth(name):
    """The fp32 sum in input order differs in bits from the reversed-order sum and from the float64 sum
    rounded once, in at least one run: a kernel that sums in another order or precision fails the case."""
    if name == "mixed":
        sums = fc.dense_run_sums(fc.dense_cases()[name])
    else:
        c = fc.coo_cases()[name]
        sums = fc.run_sums(c["rows"], c["cols"], c["vals"])
    assert sums
    assert any(_bits(f) != _bits(r) for f, r, _ in sums), "reversed order gives the same bits"
    assert any(_bits(f) != _bits(d) for f, _, d in sums), "float64 rounded once gives the same bits"


# ------------------------------------------------------------------------------ transpose

def test_transpose_cases_are_what_the_table_says():
    cases = fc.transpose_cases()
    for name, c in cases.items():
        rp, ci = c["rowptr"], c["colind"]
        rows = np.repeat(np.arange(c["shape"][0]), np.diff(rp))
        canonical = bool(np.all((np.diff(ci) > 0) | (np.diff(rows) > 0))) if len(ci) > 1 else True
        assert canonical == c["canonical"], name
    u = cases["unsorted_dups"]
    rows = np.repeat(np.arange(300), np.diff(u["rowptr"]))
    keys, counts = np.unique(rows * 200 + u["colind"], return_counts=True)
    assert 0.05 < (counts > 1).mean() < 0.2 and counts.max() >= 3
    dup = np.flatnonzero(counts > 1)[0]
    assert len(set(u["val"][rows * 200 + u["colind"] == keys[dup]].tolist())) > 1, "repeated entries differ in value"
    assert any(np.any(np.diff(u["colind"][u["rowptr"][r]:u["rowptr"][r + 1]]) < 0) for r in range(300))
    for K, bits in ((1024, 10), (1025, 11)):
        c = cases[f"pow2-K{K}"]
        assert c["shape"][1] == K and int(c["colind"].max()) == K - 1 and int(c["colind"].max()).bit_length() == bits
    assert [len(cases[f"edge-nnz{n}"]["colind"]) for n in (0, 1, 256, 257)] == [0, 1, 256, 257]
    e = cases["empties-lead-trail"]
    deg = np.diff(e["rowptr"])
    assert not deg[:100].any() and not deg[200:].any() and deg[100] and deg[199]
    assert np.count_nonzero(np.diff(cases["empties-one-row"]["rowptr"])) == 1
    w = cases["wideK"]
    assert w["shape"] == (1, 2**20) and len(w["colind"]) == 1000 and w["colind"].max() == 2**20 - 1
    b = set(_bits(cases["bits"]["val"]).tolist())
    assert {0x80000000, 0x7F800000, 0xFF800000} <= b and np.isnan(cases["bits"]["val"]).sum() == 2


def test_transpose_reference_is_stable():
    """oracle.csr_ref.csr_transpose keeps ascending source rows, and CSR order among equal (row, col)."""
    c = fc.transpose_cases()["unsorted_dups"]
    rp, ci, v = fc.csr_transpose(c["rowptr"], c["colind"], c["val"], c["shape"])
    rows = np.repeat(np.arange(c["shape"][0]), np.diff(c["rowptr"]))
    src = {}
    for k in range(len(ci)):   # entry k of the transpose must be the next unused source entry of its (row, col)
        col = int(np.searchsorted(rp, k, side="right") - 1)
        key = (int(ci[k]), col)
        cand = np.flatnonzero((rows == key[0]) & (c["colind"] == key[1]))
        j = cand[src.get(key, 0)]
        src[key] = src.get(key, 0) + 1
        assert _bits(v[k]) == _bits(c["val"][j])
        assert k == rp[col] or ci[k] >= ci[k - 1]


# ------------------------------------------------------------------------------ normalise

@pytest.mark.parametrize("name", ["weighted", "n257", "n1-empty", "n1-loop", "zero_sum"])
def test_normalize_reference_equals_scipy(name):
    pytest.importorskip("scipy")
    c = fc.normalize_cases()[name]
    rp, ci, v = fc.sym_normalize_f64(c["rows"], c["cols"], c["vals"], c["n"])
    r, cc, vv = gcn_ref.normalize_adj_coo(c["rows"], c["cols"], c["vals"], c["n"])
    assert np.array_equal(np.repeat(np.arange(c["n"]), np.diff(rp)), r) and np.array_equal(ci, cc)
    assert np.array_equal(_bits(v), _bits(vv))


def test_normalize_reference_reproduces_the_goldens(golden_meta):
    for case in golden_meta["tiny_cases"]:
        rp, ci, v = fc.sym_normalize_f64(case["A_rows"], case["A_cols"], case["A_vals"], case["n"])
        rows = np.repeat(np.arange(case["n"]), np.diff(rp))
        got = {(int(r), int(c)): int(_bits(x)[0]) for r, c, x in zip(rows, ci, v)}
        want = {(int(r), int(c)): int(_bits(np.float32(x))[0]) for r, c, x in
                zip(case["adj_rows"], case["adj_cols"], case["adj_vals"])}
        assert got == want, case["name"]


def test_normalize_cases_are_what_the_table_says():
    cases = fc.normalize_cases()
    for name, c in cases.items():
        pairs = set(zip(c["rows"].tolist(), c["cols"].tolist()))
        assert len(pairs) == len(c["rows"]), name
        w = dict(zip(zip(c["rows"].tolist(), c["cols"].tolist()), c["vals"].tolist()))
        assert all(w[(j, i)] == x for (i, j), x in w.items()), name + ": symmetric"
        assert all(x != -1.0 for (i, j), x in w.items() if i == j), name
    c = cases["weighted"]
    n = c["n"]
    assert n == 700 and np.any(c["vals"] != np.round(c["vals"])) and c["vals"].min() > 0.01 and c["vals"].max() < 3
    nb = [set() for _ in range(n)]
    for i, j in zip(c["rows"].tolist(), c["cols"].tolist()):
        nb[i].add(j)
    assert sum(r in nb[r] for r in range(n)) == 50
    assert all(not nb[r] for r in fc.W_ISOLATED)
    for r in fc.W_ABOVE:
        assert len(nb[r] - {r}) >= 40 and min(nb[r] - {r}) > r
    for r in fc.W_BELOW:
        assert len(nb[r] - {r}) >= 40 and max(nb[r] - {r}) < r
    assert fc.W_ABOVE[0] in nb[fc.W_ABOVE[0]] and fc.W_ABOVE[1] not in nb[fc.W_ABOVE[1]]
    assert fc.W_BELOW[0] in nb[fc.W_BELOW[0]] and fc.W_BELOW[1] not in nb[fc.W_BELOW[1]]
    assert len(nb[0]) >= 40 and len(nb[n - 1]) >= 40 and 0 not in nb[0] and n - 1 not in nb[n - 1]
    mid = [r for r in range(n) if r in nb[r] and len(nb[r]) > 3 and min(nb[r]) < r < max(nb[r])]
    assert mid, "an explicit diagonal in the middle of a row"
    assert cases["n257"]["n"] == 257 and 256 in cases["n257"]["rows"]
    # zero_sum: d = 0 exactly at its nodes, whose rows and columns are zeros of both signs
    c = cases["zero_sum"]
    rp, ci, v, rowsum, d = fc.sym_normalize_detail(c["rows"], c["cols"], c["vals"], c["n"])
    assert all(rowsum[z] == 0 and d[z] == 0 for z in fc.ZERO_SUM_NODES) and np.count_nonzero(d == 0) == 4
    rows = np.repeat(np.arange(c["n"]), np.diff(rp))
    touched = np.isin(rows, fc.ZERO_SUM_NODES) | np.isin(ci, fc.ZERO_SUM_NODES)
    assert np.all(v[touched] == 0) and np.all(v[~touched] != 0) and np.all(rowsum[d != 0] > 0)
    assert np.signbit(v[touched]).any() and not np.signbit(v[touched]).all()
    # neg_sum: NaN exactly in the row and column of its node
    c = cases["neg_sum"]
    rp, ci, v, rowsum, d = fc.sym_normalize_detail(c["rows"], c["cols"], c["vals"], c["n"])
    assert rowsum[fc.NEG_SUM_NODE] < 0 and np.count_nonzero(rowsum <= 0) == 1
    rows = np.repeat(np.arange(c["n"]), np.diff(rp))
    assert np.array_equal(np.isnan(v), (rows == fc.NEG_SUM_NODE) | (ci == fc.NEG_SUM_NODE))


# ------------------------------------------------------------------------------ CSR -> dense

def test_dense_cases_are_what_the_table_says():
    cases = fc.dense_cases()
    assert {c["shape"][1] for n, c in cases.items() if n.startswith("lanes")} == {1, 63, 64, 65, 150}
    assert {c["shape"][0] for n, c in cases.items() if n.startswith("rows4")} == {1, 3, 4, 5}
    assert {c["ld"] - c["shape"][1] for c in cases.values()} == {0, 3}
    c = cases["lengths"]
    deg = np.diff(c["rowptr"]).tolist()
    assert deg[:5] == [0, 1, 64, 65, c["shape"][1]] and deg[5:] == [64, 64, 65, 65, 66, 66]
    for r in range(5, 11):   # sorted up to their last pair
        cols = c["colind"][c["rowptr"][r]:c["rowptr"][r + 1]]
        assert np.all(np.diff(cols[:-1]) > 0) and cols[-1] <= cols[-2]
    c = cases["mixed"]
    kinds = []
    for r in range(c["shape"][0]):
        cols = c["colind"][c["rowptr"][r]:c["rowptr"][r + 1]]
        kinds.append("inc" if np.all(np.diff(cols) > 0) else "dup" if len(set(cols.tolist())) < len(cols) else "desc")
    assert kinds == ["inc", "desc", "dup"] * 4
    for c in cases.values():
        assert not np.any(c["val"] == 0)
        M, K = c["shape"]
        want = fc.csr_to_dense_f32(c["rowptr"], c["colind"], c["val"], M, K)
        acc = np.zeros((M, K))
        np.add.at(acc, (np.repeat(np.arange(M), np.diff(c["rowptr"])), c["colind"]), c["val"].astype(np.float64))
        mag = np.zeros((M, K))
        np.add.at(mag, (np.repeat(np.arange(M), np.diff(c["rowptr"])), c["colind"]), np.abs(c["val"]).astype(np.float64))
        assert np.all(np.abs(want - acc) <= 8 * 2.0**-24 * mag)


# ------------------------------------------------------------------------------ class_stats

@pytest.mark.parametrize("nclass,n", fc.CLASS_SIZES)
def test_class_reference_equals_torch(nclass, n):
    c = fc.class_case(nclass, n)
    x = torch.from_numpy(c["wide"][:, :nclass].copy())
    assert np.array_equal(c["pred"], torch.max(x, 1)[1].numpy())
    # in-range targets: the reference's per-class sums (oracle/gcn_ref.macro_f1's expressions) and its means
    targ = torch.from_numpy(np.where((c["targets"] >= 0) & (c["targets"] < nclass), c["targets"], c["pred"]))
    got = fc.class_counts(c["wide"], c["ld"], targ.numpy(), None, nclass)
    pred = torch.from_numpy(c["pred"])
    tp = np.array([((pred == i) & (targ == i)).sum().item() for i in range(nclass)])
    fp = np.array([((pred == i) & (targ != i)).sum().item() for i in range(nclass)])
    fn = np.array([((pred != i) & (targ == i)).sum().item() for i in range(nclass)])
    assert np.array_equal(got, np.concatenate([tp, fp, fn, [tp.sum()]]))
    with np.errstate(divide="ignore", invalid="ignore"):
        p = tp / (tp + fp)
        p[np.isnan(p)] = 0
        r = tp / (tp + fn)
        r[np.isnan(r)] = 0
        want = (2 * (p.mean() * r.mean()) / (p.mean() + r.mean()), p.mean(), r.mean())
    assert gcn_ref.macro_f1(x, targ, nclass) == pytest.approx(want, rel=0, abs=0, nan_ok=True)
    assert gcn_ref.accuracy(x, targ) == got[-1] / n
    # out-of-range targets: a false positive of the predicted class, no false negative, never correct
    full = fc.class_want(nclass, n, "none")
    nbad = sum(len(a) for a in c["bad"].values())
    assert full[:nclass].sum() + full[nclass:2 * nclass].sum() == n and full[:nclass].sum() == full[-1]
    assert full[nclass:2 * nclass].sum() - full[2 * nclass:3 * nclass].sum() == nbad
    assert not fc.class_want(nclass, n, "empty").any()
    assert fc.class_want(nclass, n, "repeats")[:2 * nclass].sum() == len(c["idx"]["repeats"])
    assert np.array_equal(fc.class_want(nclass, n, "perm"), full)


def test_class_cases_are_what_the_table_says():
    assert {n for _c, n in fc.CLASS_SIZES} == {1, 255, 256, 257, 1000}
    assert {c for c, _n in fc.CLASS_SIZES} == {1, 2, 8, 255, 1024} and (1024, 257) in fc.CLASS_SIZES
    c = fc.class_case(8, 1000)
    x = c["wide"][:, :8]
    kind = {k: np.flatnonzero(c["kinds"] == i) for i, k in enumerate(fc.LOGIT_KINDS)}
    assert all(len(v) > 100 for v in kind.values())
    assert all((x[i] == x[i].max()).sum() == 2 for i in kind["ties"])
    assert all(np.all(x[i] == 0) and np.signbit(x[i, 0]) and not np.signbit(x[i, 1]) for i in kind["signed zeros"])
    assert all(np.isnan(x[i, 0]) and c["pred"][i] == 0 for i in kind["nan first"])
    assert all(np.isnan(x[i]).sum() == 1 and np.nanmax(x[i]) == 50.0 and np.nanargmax(x[i]) < c["pred"][i]
               for i in kind["nan after larger"])
    assert all(np.isnan(x[i]).sum() == 2 and c["pred"][i] == np.flatnonzero(np.isnan(x[i]))[0] for i in kind["two nans"])
    assert all(np.isposinf(x[i]).sum() == 1 for i in kind["+inf"])
    assert all(np.all(np.isneginf(x[i])) and c["pred"][i] == 0 for i in kind["all -inf"])
    pad = c["wide"][:, 8:]
    assert pad.shape[1] == fc.CLASS_PAD and np.all(np.isnan(pad) | np.isposinf(pad)) and np.isnan(pad).any()
    t = c["targets"]
    assert (t == -1).any() and (t == 8).any() and (t == 2**33).any() and (t == 2**33 + c["pred"]).any()
    # reading the padding as classes (ld used as nclass) or truncating the targets changes the counts
    assert not np.array_equal(fc.class_counts(c["wide"], c["ld"], t, None, 8)[:8],
                              fc.class_counts(c["wide"], c["ld"], t & 0xFFFFFFFF, None, 8)[:8])
    assert len(set(c["idx"]["repeats"].tolist())) < len(c["idx"]["repeats"])
    assert sorted(c["idx"]["perm"].tolist()) == list(range(1000)) and len(c["idx"]["empty"]) == 0

