"""Seeded case tables for the multi-column solvers -- a helper of
tests/test_columns_fuzz_cpu.py, tests/test_gpu_columns_fuzz.py and
tests/test_gpu_columns_group_fuzz.py, not a test.

cases("one"): 48 drawn one-rank cases and the pinned shapes; cases("group"): 32
drawn rank groups. A case is a plain dict of draws (no arrays): the matrix
family and its parameters, the scaling, max_iter in 1..60, the column counts of
its two calls (nrhs_a, then nrhs in 1..9 on the same Matrix), ld - n in 0..5,
the columns, whether a tolerance is placed, the preconditioner kind, the
Chebyshev degree in 0..4 and whether the bounds are passed or left to the
library. Everything else is derived from it, on the CPU, and cached per case:

  matrix(case)     the oracle.CSR (global, for a group) with b = A 1;
  form(A)          (has_a, a_width, nslices) as build_a_image decides them: an
                   A image when every row is ascending and no 512-row slice has
                   more than 32 distinct offsets, one width when padding every
                   slice to the widest costs under 4 %, else per-slice (0);
  columns(case, A) B, X0 of shape (max(nrhs_a, nrhs), n);
  precond(case, A) the caller's m, or None for Jacobi, and the m the
                   restatements take;
  libs(case, A)    the libraries the case is run with: batch alone on a fully
                   diagonal matrix (there the preconditioned recurrences end in
                   rounding noise after one iteration and their niters depends
                   on the dot's order); else batch, pcg, srcg, poly, poly32, and
                   mixed unless the scaling is p10 (it iterates unpreconditioned
                   and does not converge there);
  tolerance(case)  0.0, or a value between two consecutive residuals of column
                   0 that is at least 1 % away from every residual of every
                   column of every library's restatement (so no loop test can
                   flip on rounding);
  reference(...)   the committed restatement of a library, with a choice of the
                   dot's order.

A case whose references disagree with themselves under the two dot orders
(tests/test_columns_fuzz_cpu.py) is replaced by bumping its entry in REDRAW,
which reseeds that case alone.

Pinned shapes (27-pt unless marked), what each is there for:
  32x32x32 (64 slices: exactly one dot group), 32x32x33 (66: a second group of
  two), 21x21x73 (63); 17x9x10, 20x16x8, 16x14x16, 16x16x18 (3, 5, 7, 9 slices:
  around the 8 XCDs); 40x40x1 (9 wide, 4 slices), 2x2x300 (15 wide, 3 slices),
  1x1x700 (3 wide, 2 slices), 1x24x24 and 24x1x30 7-pt (5 wide, 2 slices): the
  kW = 0 kernels with a uniform abase; 3x3x100 (27 wide, its offsets -13..13 all
  consecutive: "triples" that are not x-neighbours).
"""
import numpy as np

import columns_cases as cc
import oracle
import test_gpu_mixed as tm
import test_gpu_pcg as tp
import test_gpu_pcg_group as tpg
import test_gpu_poly as tpoly
import test_gpu_poly32 as tpoly32
import test_gpu_srcg as tsr
from test_gpu_poly32_group import rank_dot

SEED = 20261021
DRAWN = {"one": 48, "group": 32}
SLICE = 512
A_MAX = 32  # (kAMax)
ONE_LIBS = ("batch", "pcg", "srcg", "poly", "poly32", "mixed")
GROUP_LIBS = ("batch", "pcg", "poly", "poly32")
PRECONDITIONED = ("pcg", "srcg", "poly", "poly32")

# case name -> redraw number (a case that failed the reference-alone condition
# of tests/test_columns_fuzz_cpu.py; beside it the first draw's library and
# column that missed it, its niters under the two dot orders and its spreads
# on rtrans and on x). Nearly all are the unpreconditioned recurrence on a
# scaled matrix it does not converge on, or a recurrence on a "perturbed"
# stencil that is no longer diagonally dominant: there the trajectory itself
# amplifies the last bit of a dot.
REDRAW = {
    "o2": 1,  # batch column 2: niters 33 / 33, rtrans 1.2e-10, x 1.9e-06
    "o4": 2,  # mixed column 0: niters 57 / 57, rtrans 1.6e-09, x 4.2e-17
    "o7": 1,  # mixed column 0: niters 34 / 34, rtrans 2.7e-08, x 4.4e-16
    "o10": 1,  # batch column 0: niters 35 / 35, rtrans 7.5e-01, x 3.4e-03
    "o11": 5,  # srcg column 1: niters 24 / 24, rtrans 8.0e-13, x 1.1e-10
    "o12": 1,  # batch column 0: niters 51 / 51, rtrans 1.7e-08, x 4.4e-12
    "o13": 1,  # batch column 0: niters 40 / 40, rtrans 3.2e-14, x 1.3e-09
    "o14": 1,  # batch column 1: niters 48 / 48, rtrans 8.8e-02, x 3.3e-03
    "o17": 3,  # pcg column 0: niters 59 / 59, rtrans 2.4e-07, x 3.0e-08
    "o18": 3,  # batch column 0: niters 46 / 46, rtrans 7.5e-01, x 3.8e-06
    "o21": 2,  # batch column 0: niters 59 / 59, rtrans 6.8e+00, x 2.1e-22
    "o23": 2,  # batch column 0: niters 49 / 49, rtrans 7.4e-02, x 8.1e-05
    "o25": 1,  # batch column 5: niters 18 / 18, rtrans 3.0e-11, x 2.3e-10
    "o26": 2,  # batch column 0: niters 29 / 29, rtrans 1.7e-13, x 2.6e-08
    "o29": 1,  # batch column 0: niters 37 / 37, rtrans 2.9e-06, x 5.7e-06
    "o35": 1,  # pcg column 0: niters 56 / 56, rtrans 2.6e-09, x 3.9e-09
    "o39": 2,  # batch column 2: niters 26 / 26, rtrans 3.4e-10, x 2.2e-06
    "o41": 1,  # mixed column 0: niters 37 / 37, rtrans 3.3e-09, x 2.6e-23
    "o46": 2,  # batch column 0: niters 40 / 40, rtrans 2.9e-01, x 2.1e-03
    "o47": 2,  # batch column 1: niters 48 / 48, rtrans 6.1e-03, x 2.1e-03
    "g3": 1,  # batch column 0: niters 36 / 36, rtrans 2.5e-14, x 2.7e-09
    "g7": 1,  # batch column 0: niters 42 / 42, rtrans 3.7e-01, x 1.9e-02
    "g8": 1,  # batch column 1: niters 53 / 53, rtrans 5.5e-01, x 6.3e-03
    "g9": 1,  # batch column 0: niters 48 / 48, rtrans 2.4e-03, x 1.4e-03
    "g10": 3,  # batch column 0: niters 28 / 28, rtrans 9.2e-15, x 1.1e-08
    "g15": 1,  # pcg column 0: niters 52 / 52, rtrans 1.7e-06, x 1.5e-09
    "g23": 1,  # pcg column 2: niters 59 / 59, rtrans 2.2e-08, x 8.9e-09
    "g25": 1,  # batch column 0: niters 31 / 31, rtrans 2.0e-14, x 4.1e-10
}

# (name, dims, 7-pt, max_iter, nrhs_a, nrhs, scaling): the larger ones run few iterations to stay quick
PINNED = [
    ("32x32x32", (32, 32, 32), False, 7, 2, 5, "none"),
    ("32x32x33", (32, 32, 33), False, 6, 9, 6, "none"),
    ("21x21x73", (21, 21, 73), False, 8, 3, 7, "p2"),
    ("40x40x1", (40, 40, 1), False, 40, 6, 9, "none"),
    ("2x2x300", (2, 2, 300), False, 35, 8, 5, "p10"),
    ("3x3x100", (3, 3, 100), False, 30, 4, 8, "none"),
    ("1x1x700", (1, 1, 700), False, 25, 7, 6, "perturbed"),
    ("1x24x24_7pt", (1, 24, 24), True, 45, 5, 7, "none"),
    ("24x1x30_7pt", (24, 1, 30), True, 33, 9, 3, "none"),
    ("17x9x10", (17, 9, 10), False, 22, 1, 9, "perturbed"),
    ("20x16x8", (20, 16, 8), False, 18, 5, 6, "none"),
    ("16x14x16", (16, 14, 16), False, 15, 6, 7, "p10"),
    ("16x16x18", (16, 16, 18), False, 12, 8, 8, "none"),
]


# ---------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------
def _rng(kind, name):
    return np.random.default_rng([SEED, {"one": 1, "group": 2}[kind], REDRAW.get(name, 0)] + [ord(ch) for ch in name])


def _draw_columns(rng, ncol):
    """Per column (b, scale, x0): b "gen" (the generated A 1) or "rand"; scale
    1, 2^-20 or 2^10; x0 "zero", "rand" (about a third) or "exact" (at most one
    column, never column 0: it ends in the prologue)."""
    cols = []
    for c in range(ncol):
        b = ("gen", "rand")[int(rng.integers(2))]
        scale = (0, 0, -20, 10)[int(rng.integers(4))]
        x0 = "rand" if rng.integers(3) == 0 else "zero"
        cols.append([b, scale, x0])
    if ncol > 1 and rng.integers(3) == 0:
        cols[int(rng.integers(1, ncol))] = ["gen", 0, "exact"]
    return [tuple(c) for c in cols]


def _draw_common(rng, case, max_iter=None, nrhs_a=None, nrhs=None):
    case["max_iter"] = int(rng.integers(1, 61)) if max_iter is None else max_iter
    a, b = (int(v) for v in rng.integers(1, 10, size=2))
    case["nrhs_a"] = a if nrhs_a is None else nrhs_a
    case["nrhs"] = b if nrhs is None else nrhs
    case["pad"] = int(rng.integers(0, 6))
    case["cols"] = _draw_columns(rng, max(case["nrhs_a"], case["nrhs"]))
    case["col_seed"] = int(rng.integers(1 << 30))
    case["early"] = bool(rng.integers(3) == 0)
    case["tol_pick"] = float(rng.uniform())
    case["precond"] = ("jacobi", "caller", "pow2")[int(rng.integers(3))]
    case["pow2"] = int(rng.integers(-4, 5))
    case["degree"] = int(rng.integers(0, 5))
    case["bounds"] = bool(rng.integers(2))
    return case


def _one_cases():
    out = []
    for i in range(DRAWN["one"]):
        name = f"o{i}"
        rng = _rng("one", name)
        case = {"kind": "one", "name": name}
        # the family and the band go round with the index, so that every form stays in the table whatever is redrawn
        fam = i % 4
        if fam < 2:
            case["family"] = "stencil"
            case["s7"] = bool(rng.integers(2))
            nx, ny = (int(v) for v in rng.integers(1, 25, size=2))
            case["dims"] = (nx, ny, int(rng.integers(1, 41)))
            case["scaling"] = ("none", "p2", "p10", "perturbed")[int(rng.integers(4))]
        else:
            case["family"] = "csr"
            case["sorted"] = fam == 3
            case["n"] = int(rng.integers(2, 6001))
            case["per_row"] = int(rng.integers(1, 14))
            case["band"] = (0, 1, 7, 300, 2000)[(i // 4 + fam) % 5]
            case["dyadic"] = bool(rng.integers(2))
            case["scaling"] = ("none", "p2", "p10")[int(rng.integers(3))]
        case["seed"] = int(rng.integers(1 << 30))
        out.append(_draw_common(rng, case))
    for name, dims, s7, max_iter, nrhs_a, nrhs, scaling in PINNED:
        rng = _rng("one", name)
        case = {"kind": "one", "name": name, "family": "stencil", "s7": s7, "dims": dims, "scaling": scaling,
                "seed": int(rng.integers(1 << 30))}
        out.append(_draw_common(rng, case, max_iter, nrhs_a, nrhs))
    return out


def _group_cases():
    out = []
    for i in range(DRAWN["group"]):
        name = f"g{i}"
        rng = _rng("group", name)
        case = {"kind": "group", "name": name, "P": int(rng.integers(2, 6))}
        if rng.integers(2):
            case["family"] = "stencil"
            case["s7"] = bool(rng.integers(2))
            nx, ny = (int(v) for v in rng.integers(1, 17, size=2))
            case["dims"] = (nx, ny, int(rng.integers(1, 9)))  # per member
            case["scaling"] = "none"
        else:
            # slabs of unequal sizes: one below a slice, the others anywhere (so mostly not on a slice boundary);
            # the band no wider than the smallest slab (the z-slab plan: neighbours only)
            case["family"] = "csr"
            case["sorted"] = bool(rng.integers(2))
            slabs = [int(v) for v in rng.integers(60, 1500, size=case["P"])]
            slabs[int(rng.integers(case["P"]))] = int(rng.integers(40, SLICE))
            case["slabs"] = slabs
            case["per_row"] = int(rng.integers(1, 10))
            case["band"] = (1, 7, 40)[int(rng.integers(3))]
            case["scaling"] = ("none", "p2", "p10")[int(rng.integers(3))]
        case["seed"] = int(rng.integers(1 << 30))
        # (32 draws do not reach every column count twice by themselves: it goes round with the index)
        out.append(_draw_common(rng, case, nrhs=1 + (4 * i + 2) % 9))
    return out


_tables = {}


def cases(kind):
    if kind not in _tables:
        _tables[kind] = _one_cases() if kind == "one" else _group_cases()
    return _tables[kind]


def by_name(name):
    for kind in ("one", "group"):
        for c in cases(kind):
            if c["name"] == name:
                return c
    raise KeyError(name)


# ---------------------------------------------------------------------------
# what a case derives, cached per case name
# ---------------------------------------------------------------------------
_cache = {}


def _cached(case, key, make):
    k = (case["name"], key)
    if k not in _cache:
        _cache[k] = make()
    return _cache[k]


def sort_rows(A):
    """The same matrix with every row's entries in ascending column order."""
    rows = tp.rows_of(A)
    order = np.lexsort((A.cols, rows))
    return tm.finish(A.row_ptr, A.cols[order], A.vals[order])


def _scale(A, scaling):
    return A if scaling == "none" else tp.scaled(A, tp.scale_of(scaling, A.nrow))


def matrix(case):
    def make():
        rng = np.random.default_rng(case["seed"])
        if case["family"] == "stencil":
            nx, ny, nz = case["dims"]
            nz *= case.get("P", 1)
            if case["scaling"] == "perturbed":
                return tm.perturbed(nx, ny, nz, case["s7"], case["seed"])
            return _scale(oracle.generate(nx, ny, nz, use_7pt=case["s7"]), case["scaling"])
        if case["kind"] == "one":
            A = tm.random_spd(rng, case["n"], case["per_row"], case["band"], case["dyadic"])
        else:
            A = tpg.random_spd(rng, sum(case["slabs"]), case["per_row"], case["band"])
        if case["sorted"]:
            A = sort_rows(A)
        return _scale(A, case["scaling"])
    return _cached(case, "A", make)


def generated(case):
    """Built by generate_matrix / group_generate on the device (else from the CSR)."""
    return case["family"] == "stencil" and case["scaling"] == "none"


def counts(case):
    """A group's rows per member."""
    if case["family"] == "stencil":
        nx, ny, nz = case["dims"]
        return [nx * ny * nz] * case["P"]
    return list(case["slabs"])


def rows_of_members(case):
    out, s = [], 0
    for n in counts(case):
        out.append(slice(s, s + n))
        s += n
    return out


def form(A, lo=0, hi=None):
    """(has_a, a_width or None, nslices) of rows [lo, hi) as a matrix of their
    own (a group member: offsets are local column - local row, the same
    differences)."""
    hi = A.nrow if hi is None else hi
    n = hi - lo
    S = (n + SLICE - 1) // SLICE
    e0, e1 = int(A.row_ptr[lo]), int(A.row_ptr[hi])
    rows = tp.rows_of(A)[e0:e1] - lo
    colv = A.cols[e0:e1].astype(np.int64) - lo
    same = rows[1:] == rows[:-1]
    ascending = bool(np.all(colv[1:][same] > colv[:-1][same]))
    off = colv - rows
    base = int(off.min()) if len(off) else 0
    span = (int(off.max()) - base + 1) if len(off) else 1
    pairs = np.unique((rows // SLICE) * span + (off - base))
    cnt = np.bincount(pairs // span, minlength=S)
    if not ascending or cnt.max() > A_MAX:
        return 0, None, S
    wmax = int(cnt.max())
    return 1, (wmax if wmax * S <= 1.04 * cnt.sum() else 0), S


def exact32(A, lo=0, hi=None):
    e0, e1 = int(A.row_ptr[lo]), int(A.row_ptr[A.nrow if hi is None else hi])
    v = A.vals[e0:e1]
    return bool(np.all(v.astype(np.float32).astype(np.float64) == v))


def fully_diagonal(A):
    return A.nnz == A.nrow


def libs(case, A):
    if case["kind"] == "group":
        return ("batch",) if fully_diagonal(A) else GROUP_LIBS
    if fully_diagonal(A):
        return ("batch",)
    return ("batch",) + PRECONDITIONED + (("mixed",) if case["scaling"] != "p10" else ())


def columns(case, A):
    def make():
        n = A.nrow
        rng = np.random.default_rng(case["col_seed"])
        ncol = len(case["cols"])
        B, X0 = np.zeros((ncol, n)), np.zeros((ncol, n))
        for c, (b, scale, x0) in enumerate(case["cols"]):
            B[c] = (A.b if b == "gen" else rng.uniform(-1.0, 1.0, n)) * 2.0 ** scale
            if x0 == "rand":
                X0[c] = rng.uniform(-1.0, 1.0, n)
            elif x0 == "exact":
                X0[c] = A.xexact
        return B, X0
    return _cached(case, "cols", make)


def precond(case, A):
    """(what the caller passes: None for Jacobi or the vector m, the m of the restatements)."""
    def make():
        d = tp.csr_diagonal(A)
        if case["precond"] == "jacobi":
            return None, 1.0 / d
        if case["precond"] == "pow2":
            m = np.full(A.nrow, 2.0 ** case["pow2"])
        else:
            m = 10.0 ** np.random.default_rng(case["col_seed"] + 1).uniform(-1.0, 1.0, A.nrow) / d
        return m, m
    return _cached(case, "m", make)


def bounds(case, A):
    """(lmin, lmax) of the polynomial: numpy_bound's, lmin = lmax / 30."""
    def make():
        lmax = tpoly.numpy_bound(A, precond(case, A)[1])[0]
        return lmax / 30.0, lmax
    return _cached(case, "bounds", make)


def passed_bounds(case, A):
    """What the library is given: the explicit values in half the cases."""
    return bounds(case, A) if case["bounds"] else (None, None)


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
def _dot_of(dot):
    return {"seq": oracle.ddot, "np": np.dot}.get(dot, dot) if isinstance(dot, str) else dot


def reference(lib, A, b, x0, m, degree, max_iter, tol, dot="seq", lmin=None, lmax=None):
    """(x, niters, normr, trace[, (sweep iters, sweep residuals)]) of one column
    by the committed restatement of lib. dot: "seq" (oracle.ddot, a sequential
    sum), "np" (np.dot) or a callable (test_gpu_poly32_group.rank_dot). batch
    in the sequential order is oracle.hpccg itself; in another order it is
    test_gpu_pcg.restated with m = 1, which is the same recurrence
    (tests/test_columns_fuzz_cpu.py pins them bitwise equal in the sequential
    order). mixed on a float-exact matrix is the plain recurrence (one sweep)."""
    d = _dot_of(dot)
    b, x0 = np.ascontiguousarray(b), np.ascontiguousarray(x0)
    if lib == "batch" or (lib == "mixed" and exact32(A)):
        if dot == "seq":
            out = cc.expect_plain(A, b, x0, max_iter, tol)
        else:
            out = tp.restated(A, b, np.ones(A.nrow), max_iter, tol, x0=x0, dot=d)
        if lib == "mixed":
            out = tuple(out) + ((np.array([out[1]], np.int32), None),)
        return out
    if lib == "mixed":
        return cc.expect_refined(A, b, x0, max_iter, tol, dot=d)
    if lib == "pcg":
        return tp.restated(A, b, m, max_iter, tol, x0=x0, dot=d)
    if lib == "srcg":
        return tsr.restated_sr(A, b, m, max_iter, tol, x0=x0, dot=lambda x, y: np.float64(d(x, y)))
    if lmax is None:
        lmax = tpoly.numpy_bound(A, m)[0]
        lmin = lmax / 30.0
    if lib == "poly":
        return tpoly.restated(A, b, m, degree, lmin, lmax, max_iter, tol, x0=x0, dot=d)
    if lib == "poly32":
        return tpoly32.restated32(A, tpoly32.fl32(A), b, m, degree, lmin, lmax, max_iter, tol, x0=x0, dot=d)
    raise KeyError(lib)


def second_dot(case):
    """The other summation order of a case: np.dot, or the group's (the members' sequential sums added in rank order)."""
    return "np" if case["kind"] == "one" else rank_dot(rows_of_members(case))


def case_reference(case, lib, tol, dot="seq"):
    """The reference of every column of a case under one library: a list of reference() results."""
    def make():
        A = matrix(case)
        B, X0 = columns(case, A)
        m = precond(case, A)[1]
        lmin, lmax = bounds(case, A) if lib in ("poly", "poly32") else (None, None)
        return [reference(lib, A, B[c], X0[c], m, case["degree"], case["max_iter"], tol, dot, lmin, lmax)
                for c in range(B.shape[0])]
    key = dot if isinstance(dot, str) else "second"
    return _cached(case, ("ref", lib, float(tol), key), make)


def _residuals(case, lib, tol):
    """Every residual a loop test of lib compares with the tolerance, over the columns."""
    out = []
    for r in case_reference(case, lib, tol):
        out.append(np.asarray(r[3], np.float64))
        if lib == "mixed" and r[4][1] is not None:
            out.append(np.asarray(r[4][1], np.float64))
    return np.concatenate(out) if out else np.zeros(0)


def tolerance(case):
    """0.0, or between two consecutive residuals of column 0 (of the first
    library: batch's restatement) above the rounding regime, as
    test_gpu_fuzz.py places it, and at least 1 % away from every residual of
    every column of every library the case runs. The candidates are the gaps of
    column 0's trace, tried from the drawn one onwards; a case with no
    admissible gap runs at 0.0."""
    def make():
        if not case["early"]:
            return 0.0
        A = matrix(case)
        run = libs(case, A)
        tr = np.asarray(case_reference(case, run[0], 0.0)[0][3], np.float64)
        above = int(np.sum(tr >= 1e-9 * tr[0]))
        if above < 3:
            return 0.0
        start = int(case["tol_pick"] * (above - 1))
        for step in range(above - 1):
            j = (start + step) % (above - 1)
            hi, lo = tr[j], tr[j + 1]
            if not (hi > 0 and lo > 1e-8 * hi and lo < 0.9 * hi):
                continue
            tol = float(np.sqrt(lo * hi))
            ok = True
            for lib in run:
                # (mixed's later sweeps depend on the tolerance itself: its reference is run under it)
                res = _residuals(case, lib, tol if lib == "mixed" else 0.0)
                res = res[np.isfinite(res)]
                if np.any(np.abs(res - tol) < 0.01 * tol):
                    ok = False
                    break
            if ok:
                return tol
        return 0.0
    return _cached(case, "tol", make)


def check_end(got, ref, max_iter):
    """Termination after conftest.check_final's rule. Above the noise floor --
    where every non-degenerate column of the tables ends, under a tolerance
    too -- that is its last clause: niters equal and normr within 1e-4
    relative. A reference that ends in rounding noise goes through check_final
    itself."""
    from conftest import CONVERGED_REL, check_final
    r0 = ref[3][0]
    if ref[2] > CONVERGED_REL * r0:
        assert got[1] == ref[1], (got[1], ref[1])
        assert abs(got[2] - ref[2]) <= 1e-4 * ref[2], (got[2], ref[2])
    else:
        check_final(got[1], got[2], got[3], ref[1], ref[2], ref[3], max_iter)
