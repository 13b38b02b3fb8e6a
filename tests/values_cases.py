"""Seeded case tables of matrices with distinct values for the single solve --
a helper of tests/test_values_cpu.py, tests/test_gpu_values.py and
tests/test_gpu_values_group.py, not a test.

The generated stencil holds -1.0 at every off-diagonal: a kernel that reads an
entry's value from another slot of the row (a ring slot off by one, a shifted
pair window, the neighbouring unit's values) still computes the right product
there. The matrices here give every stored entry its own value, so such a
kernel moves the result.

cases("one"): 48 drawn one-rank cases and the pinned shapes; cases("group"): 32
drawn rank groups. A case is a plain dict of draws (no arrays); everything else
is derived from it on the CPU and cached per case:

  matrix(case)       the oracle.CSR (global, for a group);
  columns(case, A)   b (A 1 or uniform random) and x0 (zero, or uniform random
                     in about two thirds of the cases: with x0 = 0 the prologue
                     SpMV multiplies zeros and sees no value);
  tolerance(case)    0.0, or between two consecutive residuals of the oracle,
                     placed by tests/test_gpu_fuzz.py's rule;
  reference(case)    oracle.hpccg on the CSR; reference(case, second=True) the
                     same recurrence (test_gpu_pcg.restated with m = 1) under
                     the other dot order: np.dot, or for a group the members'
                     sequential sums added in rank order;
  swapped(case, A)   A with the values of the first and last off-diagonal
                     entries of one drawn row exchanged.

Matrix families:
  dominant  the structure of oracle.generate(nx, ny, nz, use_7pt), every
            off-diagonal multiplied by a factor in [0.5, 1) and every diagonal
            by one in [1, 1.5): each row and each column stays strictly
            diagonally dominant (>= 27 against < 26), so p.Ap > 0 whether the
            values are symmetric or not. sym: one factor per unordered index
            pair, else one per stored entry (a kernel that reads a_ji for a_ij
            is invisible on a symmetric matrix; for a few dozen iterations CG
            on the other is plain arithmetic the oracle performs identically).
            dyadic: the factors are multiples of 2^-10, so every value is exact
            in fp32.
  csr       test_gpu_mixed.random_spd, bands 1 and 7, n in 2..6000 (half of
            them a few rows past a slice boundary, where the last slice holds
            fewer offsets than the others: the per-slice widths); rows sorted
            (columns_fuzz.sort_rows: SELL-512-A at an odd uniform width or at
            per-slice widths) or, in a third of them, as drawn (no A image: the
            SELL-512 kernel alone).

A case that misses a condition of tests/test_values_cpu.py is replaced by
bumping its entry in REDRAW, which reseeds that case alone.

Pinned shapes (27-pt unless marked): 16x16x16 (8 slices, width 27, fits the
persistent launch), 12x10x16 7-pt (width 7, the triple plan), 32x32x33 (66
slices: a second dot group), 17x9x10 and 20x16x8 (3 and 5 slices), 3x3x100
(27 wide, consecutive offsets), 40x40x1 (9 wide), 1x1x700 (3 wide), 24x1x30
7-pt (5 wide).
"""
import numpy as np

import columns_fuzz as cf
import oracle
import test_gpu_mixed as tm
import test_gpu_pcg as tp
from test_gpu_fuzz import OPTIONS as ONE_OPTIONS
from test_gpu_group_fuzz import OPTIONS as GROUP_OPTIONS
from test_gpu_pcg_group import csr_parts  # noqa: F401 (the GPU tests cut the global matrix with it)
from test_gpu_poly32_group import rank_dot

SEED = 20261023
DRAWN = {"one": 48, "group": 32}
SLICE = cf.SLICE

# case name -> redraw number; beside it the condition the draw before missed
# and its figure (tests/test_values_cpu.py).
REDRAW = {
    "v0": 1,  # the exchange: rtrans 0.0, x 0.0 (max_iter 1 from x0 = 0: no product with a value)
    "v18": 1,  # the exchange: rtrans 4.0e-08, x 0.0 (max_iter 1: the initial residual alone, 1224 rows)
}

# (name, dims, 7-pt)
PINNED = [
    ("16x16x16", (16, 16, 16), False),
    ("12x10x16_7pt", (12, 10, 16), True),
    ("32x32x33", (32, 32, 33), False),
    ("17x9x10", (17, 9, 10), False),
    ("20x16x8", (20, 16, 8), False),
    ("3x3x100", (3, 3, 100), False),
    ("40x40x1", (40, 40, 1), False),
    ("1x1x700", (1, 1, 700), False),
    ("24x1x30_7pt", (24, 1, 30), True),
]
PINNED_MAX_ITER = 25


# ---------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------
def _rng(kind, name):
    return np.random.default_rng([SEED, {"one": 1, "group": 2}[kind], REDRAW.get(name, 0)] + [ord(ch) for ch in name])


def _draw_common(rng, case, options):
    case["seed"] = int(rng.integers(1 << 30))
    case["b"] = ("gen", "rand")[int(rng.integers(2))]
    case["x0"] = "zero" if rng.integers(3) == 0 else "rand"
    case["col_seed"] = int(rng.integers(1 << 30))
    case["max_iter"] = int(rng.integers(1, 41))
    case["early"] = bool(rng.integers(3) == 0)
    case["opts"] = {k: int(rng.choice(v)) for k, v in options.items()}
    case["swap_seed"] = int(rng.integers(1 << 30))
    return case


def _one_cases():
    out = []
    for i in range(DRAWN["one"]):
        name = f"v{i}"
        rng = _rng("one", name)
        case = {"kind": "one", "name": name}
        # the family goes round with the index, so that every form stays in the table whatever is redrawn
        if i % 2 == 0:
            case["family"] = "dominant"
            case["s7"] = bool(rng.integers(2))
            nx, ny = (int(v) for v in rng.integers(1, 25, size=2))
            case["dims"] = (nx, ny, int(rng.integers(1, 41)))
            case["sym"] = bool((i // 2) % 2)
            case["dyadic"] = bool((i // 4) % 2)
        else:
            case["family"] = "csr"
            case["sorted"] = (i // 2) % 3 != 2
            case["band"] = (1, 7)[(i // 6) % 2]
            if rng.integers(2):
                case["n"] = int(rng.integers(2, 6001))
            else:
                case["n"] = SLICE * int(rng.integers(1, 6)) + int(rng.integers(1, 13))
            case["per_row"] = int(rng.integers(1, 14))
            case["dyadic"] = bool(rng.integers(2))
        _draw_common(rng, case, ONE_OPTIONS)
        case["opts"]["resident_update"] = int(rng.choice((0, 1, -1)))
        case["opts"]["nt"] = int(rng.choice((-1, 0, 1)))
        out.append(case)
    for j, (name, dims, s7) in enumerate(PINNED):
        rng = _rng("one", name)
        case = {"kind": "one", "name": name, "family": "dominant", "s7": s7, "dims": dims,
                "sym": bool(j % 2), "dyadic": bool((j // 2) % 2)}
        _draw_common(rng, case, ONE_OPTIONS)
        case["opts"]["resident_update"] = int(rng.choice((0, 1, -1)))
        case["opts"]["nt"] = int(rng.choice((-1, 0, 1)))
        # the pinned shapes run the cross too: its iteration count, and its random x0
        case["max_iter"], case["x0"], case["early"] = PINNED_MAX_ITER, "rand", False
        out.append(case)
    return out


def _group_cases():
    out = []
    for i in range(DRAWN["group"]):
        name = f"w{i}"
        rng = _rng("group", name)
        P = int(rng.integers(2, 6))
        nx, ny = (int(v) for v in rng.integers(1, 17, size=2))
        case = {"kind": "group", "name": name, "family": "dominant", "P": P, "s7": bool(rng.integers(2)),
                "nxy": (nx, ny), "planes": [int(v) for v in rng.integers(1, 9, size=P)],
                "sym": bool(i % 2), "dyadic": bool((i // 2) % 2)}
        if i % 8 == 7:  # (a few groups of equal slabs stay in the table: the plan group_generate's members get)
            case["planes"] = [case["planes"][0]] * P
        case["dims"] = (nx, ny, sum(case["planes"]))
        out.append(_draw_common(rng, case, GROUP_OPTIONS))
        case["early"] = False  # (the group sweep places no tolerance)
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


def dominant(nx, ny, nz, s7, sym, dyadic, seed):
    """The stencil's structure with distinct values (the module's docstring)."""
    G = oracle.generate(nx, ny, nz, use_7pt=s7)
    n = G.nrow
    rows = tp.rows_of(G)
    c = G.cols.astype(np.int64)
    rng = np.random.default_rng(seed)
    if sym:
        _, inv = np.unique(np.minimum(rows, c) * n + np.maximum(rows, c), return_inverse=True)
        f = rng.uniform(0.5, 1.0, int(inv.max()) + 1)[inv]
    else:
        f = rng.uniform(0.5, 1.0, len(c))
    diag = rows == c
    f = np.where(diag, f + 0.5, f)  # ([1, 1.5) on the diagonal)
    if dyadic:
        f = np.floor(f * 1024.0) / 1024.0
    return tm.finish(G.row_ptr, G.cols, G.vals * f)


def matrix(case):
    def make():
        if case["family"] == "dominant":
            return dominant(*case["dims"], case["s7"], case["sym"], case["dyadic"], case["seed"])
        A = tm.random_spd(np.random.default_rng(case["seed"]), case["n"], case["per_row"], case["band"],
                          case["dyadic"])
        return cf.sort_rows(A) if case["sorted"] else A
    return _cached(case, "A", make)


def counts(case):
    """A group's rows per member."""
    nx, ny = case["nxy"]
    return [nx * ny * p for p in case["planes"]]


def rows_of_members(case):
    out, s = [], 0
    for n in counts(case):
        out.append(slice(s, s + n))
        s += n
    return out


def columns(case, A):
    """(b, x0)."""
    def make():
        rng = np.random.default_rng(case["col_seed"])
        b = A.b.copy() if case["b"] == "gen" else rng.uniform(-1.0, 1.0, A.nrow)
        x0 = rng.uniform(-1.0, 1.0, A.nrow) if case["x0"] == "rand" else np.zeros(A.nrow)
        return b, x0
    return _cached(case, "cols", make)


def solve(A, b, x0, max_iter, tol=0.0, dot=None):
    """{niters, normr, x, trace} of the reference recurrence: oracle.hpccg, or
    under another dot order the same recurrence spelled by
    test_gpu_pcg.restated with m = 1 (tests/test_columns_fuzz_cpu.py pins the
    two bitwise equal in the sequential order)."""
    if dot is None:
        return oracle.hpccg(A, b=b, x=x0, max_iter=max_iter, tolerance=tol)
    x, it, normr, trace = tp.restated(A, b, np.ones(A.nrow), max_iter, tol, x0=x0, dot=dot)
    return {"niters": it, "normr": normr, "x": x, "trace": trace}


def tolerance(case):
    """tests/test_gpu_fuzz.py's rule: between two consecutive oracle residuals above the rounding-noise regime."""
    def make():
        if not case["early"]:
            return 0.0
        A = matrix(case)
        b, x0 = columns(case, A)
        ref = solve(A, b, x0, case["max_iter"])
        if ref["niters"] < 3:
            return 0.0
        tr = ref["trace"]
        above = int(np.sum(tr >= 1e-9 * tr[0]))
        j = max(0, min(len(tr) - 2, above // 2))
        lo, hi = tr[j + 1], tr[j]
        if hi > 0 and lo > 1e-8 * hi and lo < 0.9 * hi:
            return float(np.sqrt(lo * hi))
        return 0.0
    return _cached(case, "tol", make)


def second_dot(case):
    return np.dot if case["kind"] == "one" else rank_dot(rows_of_members(case))


def reference(case, second=False):
    def make():
        A = matrix(case)
        b, x0 = columns(case, A)
        return solve(A, b, x0, case["max_iter"], tolerance(case), second_dot(case) if second else None)
    return _cached(case, ("ref", second), make)


def swap_first_and_last(A, row):
    """A's values with those of the first and last off-diagonal entries of a row exchanged."""
    lo, hi = int(A.row_ptr[row]), int(A.row_ptr[row + 1])
    off = [e for e in range(lo, hi) if A.cols[e] != row]
    vals = A.vals.copy()
    if len(off) >= 2:
        vals[off[0]], vals[off[-1]] = A.vals[off[-1]], A.vals[off[0]]
    return vals


def swap_row(case, A):
    """The drawn row, among those with at least two off-diagonal entries (None: there is none)."""
    rows = np.nonzero(np.diff(A.row_ptr) >= 3)[0]
    if not len(rows):
        return None
    return int(rows[np.random.default_rng(case["swap_seed"]).integers(len(rows))])


def swapped(case, A):
    row = swap_row(case, A)
    vals = A.vals if row is None else swap_first_and_last(A, row)
    return oracle.CSR(A.row_ptr, A.cols, vals, A.x, A.b, A.xexact)


def form(case):
    """columns_fuzz.form of a one-rank case: (has_a, a_width or None, nslices)."""
    return _cached(case, "form", lambda: cf.form(matrix(case)))


def trace_spread(tr_a, tr_b):
    """Largest relative difference on rtrans over the part conftest.check_trace checks (against tr_a)."""
    from conftest import RTRANS_CUTOFF
    r0 = tr_a[0] ** 2
    worst = 0.0
    for k in range(min(len(tr_a), len(tr_b))):
        rr = tr_a[k] ** 2
        if rr < RTRANS_CUTOFF * r0:
            break
        worst = max(worst, abs(tr_b[k] ** 2 - rr) / rr if rr > 0 else abs(tr_b[k] ** 2 - rr))
    return worst


def x_spread(x_a, x_b):
    return float(np.max(np.abs(x_a - x_b))) / max(1.0, float(np.max(np.abs(x_a))))
