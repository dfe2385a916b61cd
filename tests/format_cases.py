"""The sparse-format and metrics case tables (test infrastructure: numpy only, no GPU import,
no import of the product package).

The kernels every model passes through before any SpMM or GEMM runs:
  csrc/csr.hip        gcnk_coo_to_csr, gcnk_csr_transpose, gcnk_csr_to_dense
  csrc/normalize.hip  gcnk_sym_normalize
  csrc/metrics.hip    gcnk_class_stats
Each has a plain reference here -- a direct loop or sort that restates the operation, with the
kernel's rounding: fp32 sums in the stated order, float64 with one rounding for the normalisation
-- and a table of the smallest shapes at which it can still go wrong.  tests/test_format_cases.py
checks on the CPU that the references are right (against ATen, scipy, torch.max and the goldens)
and that the cases have teeth (a case meant to pin a summation order really gives other bits in
another order); tests/test_format_kernels.py runs every case on the GPU and compares exactly.

References
  coo_to_csr_f32     stable sort by (row, col), each run summed in fp32 in input order
  csr_transpose      oracle.csr_ref.csr_transpose (a stable lexsort by column, then source row)
  sym_normalize_f64  D^-1/2 (A + I) D^-1/2 in float64: row sums in column order, d = rowsum^-0.5
                     with inf -> 0, value (d[r] a) d[c], one rounding to fp32
  csr_to_dense_f32   per row, each column's entries summed in CSR order in fp32, from +0
  class_counts       per row: argmax = first maximal value, NaN maximal, the first NaN wins;
                     TP | FP of the predicted class | FN of an in-range target | correct
"""
import functools

import numpy as np

from oracle.csr_ref import csr_transpose  # noqa: F401  (the transpose reference, re-exported)


# ------------------------------------------------------------------------------ references

def coo_to_csr_f32(rows, cols, vals, shape):
    """(rowptr int64[M+1], colind int64, val float32) of a COO in any order with duplicates."""
    M, _K = shape
    rows = np.asarray(rows, np.int64)
    cols = np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float32)
    order = np.lexsort((cols, rows))   # stable: equal (row, col) keep their input order
    counts = np.zeros(M + 1, np.int64)
    colind, val = [], []
    prev = None
    for i in order:
        rc = (int(rows[i]), int(cols[i]))
        if rc == prev:
            val[-1] = np.float32(val[-1] + vals[i])
        else:
            colind.append(rc[1])
            val.append(vals[i])
            counts[rc[0] + 1] += 1
            prev = rc
    return np.cumsum(counts), np.array(colind, np.int64), np.array(val, np.float32)


def run_sums(rows, cols, vals):
    """Per run of equal (row, col), of length 2 or more: (fp32 sum in input order, fp32 sum in
    reversed order, float64 sum rounded once) -- what a case that pins the order must tell apart."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float32)
    runs = {}
    for i in range(len(vals)):
        runs.setdefault((int(rows[i]), int(cols[i])), []).append(vals[i])
    out = []
    for vs in runs.values():
        if len(vs) < 2:
            continue
        fwd, rev = np.float32(0), np.float32(0)
        for v in vs:
            fwd = np.float32(fwd + v)
        for v in vs[::-1]:
            rev = np.float32(rev + v)
        out.append((fwd, rev, np.float32(np.sum(np.asarray(vs, np.float64)))))
    return out


def sym_normalize_f64(rows, cols, vals, n):
    """CSR (rowptr, colind, val float32) of D^-1/2 (A + I) D^-1/2 for a duplicate-free COO A."""
    return sym_normalize_detail(rows, cols, vals, n)[:3]


def sym_normalize_detail(rows, cols, vals, n):
    """sym_normalize_f64's result, then rowsum(A + I) and d, both float64 (for a failure's report)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float32)
    order = np.lexsort((cols, rows))
    per_row = [[] for _ in range(n)]
    for i in order:
        per_row[int(rows[i])].append((int(cols[i]), float(vals[i])))   # float(): fp32 -> float64, exact
    rowsum = np.zeros(n, np.float64)
    for r in range(n):
        ent = per_row[r]
        at = [k for k, (c, _a) in enumerate(ent) if c == r]
        if at:
            ent[at[0]] = (r, ent[at[0]][1] + 1.0)
        else:
            ent.insert(sum(1 for c, _a in ent if c < r), (r, 1.0))
        s = 0.0
        for _c, a in ent:   # in column order
            s += a
        rowsum[r] = s
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.power(rowsum, -0.5)
    d[np.isinf(d)] = 0.0
    rowptr = np.zeros(n + 1, np.int64)
    colind, val = [], []
    with np.errstate(invalid="ignore"):
        for r in range(n):
            rowptr[r + 1] = rowptr[r] + len(per_row[r])
            for c, a in per_row[r]:
                colind.append(c)
                val.append(np.float32((d[r] * np.float64(a)) * d[c]))
    return rowptr, np.array(colind, np.int64), np.array(val, np.float32), rowsum, d


def csr_to_dense_f32(rowptr, colind, val, M, K):
    out = np.zeros((M, K), np.float32)
    for r in range(M):
        for k in range(int(rowptr[r]), int(rowptr[r + 1])):
            out[r, colind[k]] = np.float32(out[r, colind[k]] + np.float32(val[k]))
    return out


def first_argmax(p):
    """Index of the first maximal value of a row; NaN counts as maximal, the first NaN wins."""
    nan = np.flatnonzero(np.isnan(p))
    return int(nan[0]) if nan.size else int(np.flatnonzero(p == p.max())[0])


def class_counts(logits, ld, targets, idx, nclass):
    """int64[3 * nclass + 1] = TP | FP | FN | correct over the rows `idx` (all when None) of the
    flat fp32 buffer `logits`, row i at logits[i * ld : i * ld + nclass]."""
    flat = np.asarray(logits, np.float32).reshape(-1)
    targets = np.asarray(targets, np.int64)
    scored = range(len(targets)) if idx is None else [int(i) for i in np.asarray(idx, np.int64)]
    tp, fp, fn = (np.zeros(nclass, np.int64) for _ in range(3))
    for i in scored:
        best = first_argmax(flat[i * ld:i * ld + nclass])
        t = int(targets[i])
        if best == t:
            tp[best] += 1
        else:
            fp[best] += 1
            if 0 <= t < nclass:
                fn[t] += 1
    return np.concatenate([tp, fp, fn, [tp.sum()]])


# ------------------------------------------------------------------------------ COO -> CSR

def _mixed(rng, n):
    """fp32 values of mixed magnitude: sums of them depend on the order."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)).astype(np.float32)


def _coo(name, rows, cols, vals, shape, max_run):
    return dict(name=name, rows=np.asarray(rows, np.int64), cols=np.asarray(cols, np.int64),
                vals=np.asarray(vals, np.float32), shape=shape, max_run=max_run)


def _unique_pairs(rng, M, K, n, taken=()):
    seen = set(taken)
    out = []
    while len(out) < n:
        p = (int(rng.integers(0, M)), int(rng.integers(0, K)))
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def _shuffled(rng, pairs, vals, name, shape, max_run):
    perm = rng.permutation(len(pairs))
    p = np.asarray(pairs, np.int64).reshape(-1, 2)[perm]
    return _coo(name, p[:, 0], p[:, 1], np.asarray(vals, np.float32)[perm], shape, max_run)


WIDE = (100000, 70000)   # M * K = 7e9: keys of 33 bits
ONE_RUN_AT, ONE_RUN_LEN, ONE_RUN_BEFORE = (3, 2), 300, 100


@functools.lru_cache(maxsize=None)
def coo_cases():
    """name -> case.  max_run: the longest run of equal (row, col); at 2 or less the fp32 sum does
    not depend on the order (a + b = b + a), so ATen's coalesce is a second reference."""
    cases = []
    # wide: keys above 2^32 (a key cut to 32 bits merges or reorders entries), the four corners, 1000
    # duplicated pairs
    rng = np.random.default_rng(100)
    M, K = WIDE
    corners = [(0, 0), (0, K - 1), (M - 1, 0), (M - 1, K - 1)]
    pairs = corners + _unique_pairs(rng, M, K, 3000, corners)
    pairs = pairs + pairs[4:1004]
    cases.append(_shuffled(rng, pairs, _mixed(rng, len(pairs)), "wide", WIDE, 2))
    # pow2: M * K = 2^16 exactly and 2^16 + 1, each with an entry at the largest key (one radix bit too
    # few leaves that entry unsorted)
    for name, (M, K) in (("pow2-256x256", (256, 256)), ("pow2-1x65537", (1, 65537))):
        rng = np.random.default_rng(M)
        pairs = [(M - 1, K - 1), (0, 0)] + _unique_pairs(rng, M, K, 600, [(M - 1, K - 1), (0, 0)])
        pairs = pairs + pairs[:100]
        cases.append(_shuffled(rng, pairs, _mixed(rng, len(pairs)), name, (M, K), 2))
    # vectors: one column, one row, one entry, no entry
    rng = np.random.default_rng(101)
    r = np.concatenate([rng.permutation(50)[:30], np.arange(10)])
    cases.append(_coo("vec-K1", r, np.zeros(40, np.int64), _mixed(rng, 40), (50, 1), 2))
    c = np.concatenate([rng.permutation(50)[:30], np.arange(10)])
    cases.append(_coo("vec-M1", np.zeros(40, np.int64), c, _mixed(rng, 40), (1, 50), 2))
    cases.append(_coo("vec-nnz1", [3], [4], [2.5], (5, 7), 1))
    cases.append(_coo("vec-nnz0", [], [], [], (10, 4), 0))
    # one_run: 300 entries at one (r, c), 1e8, 1 and -1e8 mixed; with 100 entries sorted before it the run
    # covers sorted positions 100..399, across the 256-thread block boundary
    rng = np.random.default_rng(102)
    before = [(r, c) for r in range(3) for c in range(40)][:ONE_RUN_BEFORE]
    after = [(4, c) for c in range(30)]
    pairs = before + [ONE_RUN_AT] * ONE_RUN_LEN + after
    run = np.float32([1e8] * 6 + [-1e8] * 6 + [1.0] * (ONE_RUN_LEN - 12))   # (the 1s count only while the 1e8s cancel)
    vals = np.concatenate([_mixed(rng, len(before)), run, _mixed(rng, len(after))])
    cases.append(_shuffled(rng, pairs, vals, "one_run", (5, 40), ONE_RUN_LEN))
    # runs: lengths 1..7 in shuffled input order, mixed magnitudes
    rng = np.random.default_rng(103)
    base = _unique_pairs(rng, 400, 300, 700)
    pairs = [p for k, p in enumerate(base) for _ in range(1 + k % 7)]
    cases.append(_shuffled(rng, pairs, _mixed(rng, len(pairs)), "runs", (400, 300), 7))
    # empty_rows: 70 leading, 300 in the middle, 70 trailing
    rng = np.random.default_rng(104)
    live = np.concatenate([np.arange(70, 150), np.arange(450, 530)])
    pairs = [(int(r), int(c)) for r in live for c in rng.permutation(40)[:rng.integers(1, 6)]]
    pairs = pairs + pairs[:50]
    cases.append(_shuffled(rng, pairs, _mixed(rng, len(pairs)), "empty_rows", (600, 40), 2))
    return {c["name"]: c for c in cases}


BAD_SHAPE = (30, 20)
BAD_ENTRIES = {"row=M": (30, 3), "col=K": (3, 20), "row=-1": (-1, 3), "col=-1": (3, -1), "row=2^40": (2**40, 3)}


@functools.lru_cache(maxsize=None)
def coo_bad_case(which):
    """A valid COO with the one bad entry `which` in the middle of it (the poison flag's patterns)."""
    rng = np.random.default_rng(105)
    M, K = BAD_SHAPE
    pairs = _unique_pairs(rng, M, K, 300)
    pairs.insert(150, BAD_ENTRIES[which])
    p = np.asarray(pairs, np.int64)
    return _coo("bad-" + which, p[:, 0], p[:, 1], _mixed(rng, len(pairs)), BAD_SHAPE, 1)


def coo_valid_case():
    """The conversion run right after a refused one, on the same stream."""
    rng = np.random.default_rng(106)
    pairs = _unique_pairs(rng, *BAD_SHAPE, 200)
    pairs = pairs + pairs[:40]
    return _shuffled(rng, pairs, _mixed(rng, len(pairs)), "after-bad", BAD_SHAPE, 2)


def max_key_bits(case):
    M, K = case["shape"]
    return max(int(r) * K + int(c) for r, c in zip(case["rows"], case["cols"])).bit_length()


# ------------------------------------------------------------------------------ transpose

def _csr_case(name, cols_per_row, vals, shape, canonical):
    rp = np.zeros(len(cols_per_row) + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols_per_row])
    ci = np.concatenate([np.asarray(c, np.int64) for c in cols_per_row]) if rp[-1] else np.zeros(0, np.int64)
    assert len(cols_per_row) == shape[0] and len(vals) == rp[-1] and (not len(ci) or ci.max() < shape[1])
    return dict(name=name, rowptr=rp, colind=ci, val=np.asarray(vals, np.float32), shape=shape,
                canonical=canonical)


def _sorted_rows(rng, M, K, degs, must=()):
    rows = [np.sort(rng.choice(K, int(d), replace=False)) for d in degs]
    for r, c in must:
        rows[r] = np.union1d(rows[r], [c])
    return rows


@functools.lru_cache(maxsize=None)
def transpose_cases():
    """name -> case.  canonical: sorted, duplicate-free columns in every row (then the transpose of the
    transpose is the matrix itself)."""
    cases = []
    # unsorted_dups: shuffled columns in each row, about 10% of the (r, c) repeated with other values --
    # entries keep ascending source-row order, equal entries CSR order (an unstable sort swaps their values)
    rng = np.random.default_rng(200)
    M, K = 300, 200
    rows = []
    for r in range(M):
        c = rng.choice(K, int(rng.integers(0, 25)), replace=False)
        c = np.concatenate([c, c[rng.random(len(c)) < 0.1], c[rng.random(len(c)) < 0.02]])
        rows.append(rng.permutation(c))
    n = sum(len(c) for c in rows)
    cases.append(_csr_case("unsorted_dups", rows, _mixed(rng, n), (M, K), False))
    # pow2: the radix sort's bit count at K a power of two (last column 1023: 10 bits) and one past it
    # (last column 1024: 11 bits)
    for K in (1024, 1025):
        rng = np.random.default_rng(K)
        rows = _sorted_rows(rng, 50, K, rng.integers(0, 40, 50), must=[(7, K - 1), (31, K - 1), (31, 0)])
        n = sum(len(c) for c in rows)
        cases.append(_csr_case(f"pow2-K{K}", rows, _mixed(rng, n), (50, K), True))
    # edges
    rng = np.random.default_rng(201)
    rows = [[0] * int(k) for k in rng.integers(0, 3, 20)]
    cases.append(_csr_case("edge-K1", rows, _mixed(rng, sum(len(c) for c in rows)), (20, 1), False))
    cases.append(_csr_case("edge-M1", [rng.permutation(30)[:17]], _mixed(rng, 17), (1, 30), False))
    cases.append(_csr_case("edge-nnz1", [[], [], [5], []], [1.5], (4, 9), True))
    for nnz in (256, 257):   # the 256-thread block boundary of iota / gather
        rows = _sorted_rows(rng, 7, 64, [32] * 7) + [np.arange(nnz - 7 * 32)]
        cases.append(_csr_case(f"edge-nnz{nnz}", rows, _mixed(rng, nnz), (8, 64), True))
    cases.append(_csr_case("edge-nnz0", [[] for _ in range(6)], [], (6, 9), True))
    # empties: gather_kernel's binary search over runs of equal row pointers
    rng = np.random.default_rng(202)
    rows = [[]] * 100 + _sorted_rows(rng, 100, 60, rng.integers(0, 9, 100)) + [[]] * 100
    rows[100] = np.union1d(rows[100], [0])     # the first and last live rows are populated
    rows[199] = np.union1d(rows[199], [59])
    n = sum(len(c) for c in rows)
    cases.append(_csr_case("empties-lead-trail", rows, _mixed(rng, n), (300, 60), True))
    rows = [[]] * 100 + [np.arange(60)] + [[]] * 100
    cases.append(_csr_case("empties-one-row", rows, _mixed(rng, 60), (201, 60), True))
    # wideK: one row, 2^20 columns (20 radix bits), first and last column used
    rng = np.random.default_rng(203)
    K = 2**20
    c = np.union1d(rng.choice(K, 998, replace=False), [0, K - 1])
    cases.append(_csr_case("wideK", [c], _mixed(rng, len(c)), (1, K), True))
    # bits: the values travel as bit patterns
    rng = np.random.default_rng(204)
    rows = _sorted_rows(rng, 20, 30, rng.integers(1, 10, 20))
    n = sum(len(c) for c in rows)
    v = _mixed(rng, n)
    v[:8] = np.float32([-0.0, np.inf, -np.inf, np.nan, 0.0, -0.0, np.nan, 1e-45])
    cases.append(_csr_case("bits", rows, rng.permutation(v), (20, 30), True))
    return {c["name"]: c for c in cases}


# ------------------------------------------------------------------------------ normalise

def _sym(name, n, edges, diag=()):
    """A symmetric A as COO (both directions of every edge, then the diagonals), shuffled."""
    e = [(i, j, w) for i, j, w in edges] + [(j, i, w) for i, j, w in edges] + [(i, i, w) for i, w in diag]
    assert len({(i, j) for i, j, _w in e}) == len(e), "duplicate-free"
    rng = np.random.default_rng(n + len(e))
    e = [e[k] for k in rng.permutation(len(e))]
    return dict(name=name, n=n, rows=np.array([x[0] for x in e], np.int64), cols=np.array([x[1] for x in e], np.int64),
                vals=np.array([x[2] for x in e], np.float32))


def _random_edges(rng, nodes, m, w=lambda rng: np.float32(rng.uniform(0.01, 3.0))):
    seen, out = set(), []
    while len(out) < m:
        i, j = (int(x) for x in rng.choice(nodes, 2, replace=False))
        if (min(i, j), max(i, j)) not in seen:
            seen.add((min(i, j), max(i, j)))
            out.append((min(i, j), max(i, j), w(rng)))
    return out


W_N = 700
W_ISOLATED = (5, 333, 698)
W_ABOVE, W_BELOW = (300, 302), (301, 303)   # neighbours all above / all below; the first of each has a diagonal
W_ENDS = (0, W_N - 1)


@functools.lru_cache(maxsize=None)
def normalize_cases():
    """name -> symmetric, duplicate-free COO A.  No diagonal weight is exactly -1: scipy's A + eye prunes
    the cancelled entry where the kernel keeps a stored zero -- a known structural difference, in an
    input no real graph has."""
    cases = []
    # weighted: non-integer fp32 weights; the inserted or incremented diagonal first (rows 0, 300, 302),
    # last (rows 699, 301, 303) and in the middle of long rows; isolated nodes (a row of the diagonal only)
    rng = np.random.default_rng(300)
    special = set(W_ISOLATED + W_ABOVE + W_BELOW + W_ENDS)
    plain = np.array([i for i in range(W_N) if i not in special])
    edges = _random_edges(rng, plain, 2000)
    w = lambda: np.float32(rng.uniform(0.01, 3.0))   # noqa: E731
    for r in W_ENDS:
        edges += [(min(r, int(j)), max(r, int(j)), w()) for j in rng.choice(plain, 40, replace=False)]
    for r in W_ABOVE:
        edges += [(r, int(j), w()) for j in rng.choice(plain[plain > r], 40, replace=False)]
    for r in W_BELOW:
        edges += [(int(j), r, w()) for j in rng.choice(plain[plain < r], 40, replace=False)]
    diag = [(int(i), w()) for i in rng.choice(plain, 48, replace=False)] + [(W_ABOVE[0], w()), (W_BELOW[0], w())]
    cases.append(_sym("weighted", W_N, edges, diag))
    # n across the 256-thread boundary; n = 1 with no entry and with a self loop
    rng = np.random.default_rng(301)
    edges = _random_edges(rng, np.arange(257), 600) + [(0, 256, np.float32(0.75))]
    edges = list({(i, j): (i, j, x) for i, j, x in edges}.values())
    cases.append(_sym("n257", 257, edges, [(255, np.float32(0.3)), (256, np.float32(1.7))]))
    cases.append(_sym("n1-empty", 1, [], []))
    cases.append(_sym("n1-loop", 1, [], [(0, np.float32(0.5))]))
    # zero_sum: nodes whose two neighbours weigh -0.5, so rowsum(A + I) = 0, d = 0 and their rows and
    # columns are +-0 (compare the sign of zero).  Their neighbours keep positive sums.
    rng = np.random.default_rng(302)
    n = 60
    zeros = (0, 17, 40, 59)
    plain = np.array([i for i in range(n) if i not in zeros])
    edges = _random_edges(rng, plain, 150)
    for k, z in enumerate(zeros):
        a, b = plain[3 * k], plain[-1 - 3 * k]
        edges += [(min(z, int(j)), max(z, int(j)), np.float32(-0.5)) for j in (a, b)]
        edges += [(min(int(j), int(plain[20 + k])), max(int(j), int(plain[20 + k])), np.float32(2.5)) for j in (a, b)]
    edges = list({(i, j): (i, j, x) for i, j, x in edges}.values())
    cases.append(_sym("zero_sum", n, edges, [(int(plain[5]), np.float32(0.25))]))
    # neg_sum: one row sum below zero: d is NaN there (compare where the NaNs are, every other value by bits)
    rng = np.random.default_rng(303)
    n = 40
    edges = [e for e in _random_edges(rng, np.arange(n), 90) if 11 not in e[:2]]
    edges += [(3, 11, np.float32(-2.0)), (11, 30, np.float32(-1.5)), (11, 12, np.float32(0.5))]
    edges += [(3, 4, np.float32(5.0)), (30, 31, np.float32(5.0))]   # (its neighbours' sums stay positive)
    edges = list({(i, j): (i, j, x) for i, j, x in edges}.values())
    cases.append(_sym("neg_sum", n, edges, []))
    return {c["name"]: c for c in cases}


ZERO_SUM_NODES = (0, 17, 40, 59)
NEG_SUM_NODE = 11


# ------------------------------------------------------------------------------ CSR -> dense

def _dense_case(name, cols_per_row, K, ld, rng):
    n = sum(len(c) for c in cols_per_row)
    v = _mixed(rng, n)
    v[v == 0] = 1.0   # (a stored -0 of a sorted row is copied, where the sum from +0 gives +0: left out)
    c = _csr_case(name, cols_per_row, v, (len(cols_per_row), K), False)
    c["ld"] = ld
    return c


def _row_kinds(rng, K, deg):
    """A strictly increasing row (the store path), a descending unique one, one with repeated columns."""
    deg = min(deg, K)
    inc = np.sort(rng.choice(K, deg, replace=False))
    dup = rng.choice(inc, deg + 3, replace=True) if deg else inc
    return [inc, inc[::-1].copy(), dup]


@functools.lru_cache(maxsize=None)
def dense_cases():
    """name -> CSR with `ld`.  One wavefront per row, four rows per workgroup, lane l owns columns l,
    l + 64, ...; the path (zero-fill then one store per entry, or a sum per column) is chosen per row."""
    cases = []
    for K in (1, 63, 64, 65, 150):    # lanes: the 64-lane stride
        rng = np.random.default_rng(400 + K)
        rows = _row_kinds(rng, K, 40) + [np.arange(K), []] + _row_kinds(rng, K, 5)
        cases.append(_dense_case(f"lanes-K{K}", rows, K, K + 3, rng))
    for M in (1, 3, 4, 5):            # rows4: the 4-rows-per-workgroup boundary
        rng = np.random.default_rng(410 + M)
        rows = [_row_kinds(rng, 70, 9)[r % 3] for r in range(M)]
        cases.append(_dense_case(f"rows4-M{M}", rows, 70, 73, rng))
    # lengths: 0, 1, 64, 65 and K entries, sorted; then rows of 64, 65 and 66 whose only disorder is their last
    # pair (the pair the order check's lane 63, and lane 0's second step, look at)
    rng = np.random.default_rng(420)
    K = 130
    rows = [np.sort(rng.choice(K, d, replace=False)) for d in (0, 1, 64, 65, K)]
    for d in (64, 65, 66):
        c = np.sort(rng.choice(K, d, replace=False))
        c[-2:] = c[-2:][::-1]
        rows.append(c)
        c = np.sort(rng.choice(K, d, replace=False))
        c[-1] = c[-2]
        rows.append(c)
    cases.append(_dense_case("lengths", rows, K, K + 3, rng))
    # mixed: the three kinds in alternation, duplicates of mixed magnitude
    rng = np.random.default_rng(421)
    rows = [k for _ in range(4) for k in _row_kinds(rng, 100, 30)]
    mixed = _dense_case("mixed", rows, 100, 103, rng)
    cases.append(mixed)
    cases.append(dict(mixed, name="mixed-ldK", ld=100))
    cases.append(dict(cases[2], name="lanes-K64-ldK", ld=64))
    return {c["name"]: c for c in cases}


def dense_run_sums(case):
    """run_sums over the (row, column) runs of a CSR case."""
    rows = np.repeat(np.arange(case["shape"][0]), np.diff(case["rowptr"]))
    return run_sums(rows, case["colind"], case["val"])


# ------------------------------------------------------------------------------ class_stats

CLASS_SIZES = [(c, n) for c in (1, 2, 8, 255) for n in (1, 255, 256, 257, 1000)] + [(1024, 257)]
CLASS_PAD = 5            # ld = nclass + 5; the padding holds NaN and +inf
LOGIT_KINDS = ("random", "ties", "signed zeros", "nan first", "nan after larger", "two nans", "+inf", "all -inf")
BAD_TARGETS = ("-1", "nclass", "2^33", "2^33 + prediction")


@functools.lru_cache(maxsize=None)
def class_case(nclass, n):
    """wide fp32 [n x (nclass + 5)] whose first nclass columns are the logits; int64 targets; the row sets."""
    rng = np.random.default_rng(1000 * nclass + n)
    ld = nclass + CLASS_PAD
    wide = rng.standard_normal((n, ld)).astype(np.float32)
    x = wide[:, :nclass]
    kinds = (np.arange(n) + nclass) % len(LOGIT_KINDS)
    for i in range(n):
        a, b = sorted(int(c) for c in rng.choice(nclass, 2, replace=nclass < 2))
        kind = LOGIT_KINDS[kinds[i]]
        if kind == "ties":
            x[i, a] = x[i, b] = x[i].max() + 1
        elif kind == "signed zeros":
            x[i] = 0.0
            x[i, ::2] = -0.0
        elif kind == "nan first":
            x[i, 0] = np.nan
        elif kind == "nan after larger":
            x[i, a] = 50.0
            x[i, b] = np.nan
        elif kind == "two nans":
            x[i, a] = x[i, b] = np.nan
        elif kind == "+inf":
            x[i, b] = np.inf
        elif kind == "all -inf":
            x[i] = -np.inf
    wide[:, nclass:] = np.float32([np.nan, np.inf, np.inf, np.nan, np.inf])
    pred = np.array([first_argmax(x[i]) for i in range(n)], np.int64)
    targ = rng.integers(0, nclass, n).astype(np.int64)
    hit = rng.random(n) < 0.5
    targ[hit] = pred[hit]
    bad = {}
    for k, name in enumerate(BAD_TARGETS):   # (n = 1 keeps its in-range target: rows 3, 10, 17, 24 and on)
        at = np.arange(3 + 7 * k, n, 29)
        targ[at] = {"-1": -1, "nclass": nclass, "2^33": 2**33, "2^33 + prediction": 2**33 + pred[at]}[name]
        bad[name] = at
    idx = {"none": None, "perm": rng.permutation(n).astype(np.int64),
           "repeats": rng.integers(0, n, max(n // 2, 3)).astype(np.int64), "empty": np.zeros(0, np.int64)}
    return dict(nclass=nclass, n=n, ld=ld, wide=wide, targets=targ, pred=pred, idx=idx, kinds=kinds, bad=bad)


@functools.lru_cache(maxsize=None)
def class_want(nclass, n, idx_kind):
    c = class_case(nclass, n)
    return class_counts(c["wide"], c["ld"], c["targets"], c["idx"][idx_kind], nclass)
