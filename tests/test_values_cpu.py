"""What tests/test_gpu_values.py and tests/test_gpu_values_group.py rely on,
pinned without a GPU (the tables of tests/values_cases.py):

  * the tables are deterministic: 48 drawn and 9 pinned one-rank cases, 32
    groups whose members' plane counts are drawn independently;
  * reference spread: for every case the recurrence run with the sequential
    dot (oracle.hpccg) and with a second order (np.dot; for a group the
    members' sequential sums added in rank order) gives equal niters, rtrans
    traces within a tenth of the GPU test's bar on the part check_trace checks
    and x within 1e-10 max(1, max|x|); a placed tolerance is at least 1 % away
    from every residual. So a GPU solve that differs from the oracle by the
    dot's association alone has nine tenths of the bar left;
  * the tables see what the generated stencil cannot: exchanging the values of
    the first and last off-diagonal entries of one drawn row moves the
    oracle's trace at some checked point by at least 10 times the GPU bar, or
    x by at least 10 times 1e-9 -- while the same exchange leaves
    oracle.generate's values bitwise unchanged;
  * coverage: every image form, both symmetries and both exactnesses occur.

Worst spread over the tables (test_worst_spread_is_reported's output: relative
on rtrans against the bar 1e-9, 1e-8 for a group; on x relative to
max(1, max|x|) against 1e-10; the case beside it):
  one  : rtrans 8.4e-13 (32x32x33), x 1.4e-12 (v35)
  group: rtrans 2.2e-14 (w27), x 8.9e-16 (w27)
Two of the 89 first draws were replaced (values_cases.REDRAW), both for the
exchange: a max_iter of 1 forms the initial residual alone, from x0 = 0 with
no value in it, and on 1224 rows from a random x0 too little of one (4.0e-8).
None missed the spread.
"""
import numpy as np
import pytest

import oracle
import values_cases as vc
from conftest import RTRANS_RTOL_1GPU, RTRANS_RTOL_MULTI

ALL = vc.cases("one") + vc.cases("group")
_worst = {}


def gpu_bar(case):
    return RTRANS_RTOL_1GPU if case["kind"] == "one" else RTRANS_RTOL_MULTI


def spread(case):
    """(niters of the two orders, trace spread, x spread, distance of the tolerance from the nearest residual)."""
    a, b = vc.reference(case), vc.reference(case, second=True)
    tol = vc.tolerance(case)
    near = np.inf
    if tol > 0.0:
        near = min(float(np.min(np.abs(np.asarray(r["trace"]) - tol))) / tol for r in (a, b))
    return (a["niters"], b["niters"]), vc.trace_spread(a["trace"], b["trace"]), vc.x_spread(a["x"], b["x"]), near


def moved(case):
    """(trace, x) movement of the oracle under the exchange of one row's first and last off-diagonal values."""
    A = vc.matrix(case)
    b, x0 = vc.columns(case, A)
    ref = vc.reference(case)
    got = vc.solve(vc.swapped(case, A), b, x0, case["max_iter"], vc.tolerance(case))
    return vc.trace_spread(ref["trace"], got["trace"]), vc.x_spread(ref["x"], got["x"])


def test_the_tables_are_deterministic():
    assert len(vc.cases("one")) == 48 + len(vc.PINNED) and len(vc.PINNED) == 9
    assert len(vc.cases("group")) == 32
    assert vc._one_cases() == vc.cases("one") and vc._group_cases() == vc.cases("group")
    assert len({c["name"] for c in ALL}) == len(ALL)
    for c in ALL:
        assert 1 <= c["max_iter"] <= 40
        A = vc.matrix(c)
        if c["kind"] == "one" and c["name"] not in dict((p[0], 0) for p in vc.PINNED):
            assert A.nrow <= 24 * 24 * 40
        if c["kind"] == "group":
            assert 2 <= c["P"] <= 5 and all(1 <= p <= 8 for p in c["planes"]) and max(c["nxy"]) <= 16
            assert sum(vc.counts(c)) == A.nrow


@pytest.mark.parametrize("case", [c for c in ALL if c["family"] == "dominant"], ids=lambda c: c["name"])
def test_dominant_rows_and_columns(case):
    """Every row and every column strictly diagonally dominant: >= 27 on the
    diagonal against < 26 beside it; dyadic values exact in fp32."""
    A = vc.matrix(case)
    rows, c = vc.tp.rows_of(A), A.cols.astype(np.int64)
    diag = rows == c
    assert np.all(A.vals[diag] >= 27.0) and np.all(A.vals[diag] < 40.5) and diag.sum() == A.nrow
    off = np.abs(np.where(diag, 0.0, A.vals))
    assert np.all(off[~diag] >= 0.5) and np.all(off[~diag] < 1.0)
    assert np.bincount(rows, off, A.nrow).max() < 26.0 and np.bincount(c, off, A.nrow).max() < 26.0
    G = oracle.generate(*case["dims"], use_7pt=case["s7"])
    assert np.array_equal(G.row_ptr, A.row_ptr) and np.array_equal(G.cols, A.cols)
    assert vc.cf.exact32(A) == case["dyadic"] or A.nnz < 8
    # symmetric values exactly where drawn so
    n = A.nrow
    key, tkey = rows * n + c, c * n + rows
    order, torder = np.argsort(key), np.argsort(tkey)
    assert np.array_equal(key[order], tkey[torder])  # (the structure is symmetric)
    same = bool(np.array_equal(A.vals[order], A.vals[torder]))
    assert same == case["sym"] or A.nnz == A.nrow


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_reference_spread(case):
    its, ts, xs, near = spread(case)
    w = _worst.setdefault(case["kind"], [0.0, "", 0.0, ""])
    if ts > w[0]:
        w[0], w[1] = ts, case["name"]
    if xs > w[2]:
        w[2], w[3] = xs, case["name"]
    assert its[0] == its[1], its
    assert ts <= 0.1 * gpu_bar(case), ts
    assert xs <= 1e-10, xs
    assert near >= 0.01, near


def test_worst_spread_is_reported():
    print()
    for kind, w in sorted(_worst.items()):
        print(f"{kind:5s}: rtrans {w[0]:.1e} ({w[1]}), x {w[2]:.1e} ({w[3]})")


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_an_exchange_of_two_values_of_one_row_is_seen(case):
    ts, xs = moved(case)
    assert ts >= 10.0 * gpu_bar(case) or xs >= 10.0 * 1e-9, (ts, xs)


@pytest.mark.parametrize("dims,s7", [((16, 16, 16), False), ((12, 10, 16), True), ((24, 24, 40), False)])
def test_the_generated_stencil_cannot_see_that_exchange(dims, s7):
    """What tests/test_gpu_fuzz.py and tests/test_gpu_group_fuzz.py miss: on
    oracle.generate's matrix the exchange changes no value at all, in any row."""
    G = oracle.generate(*dims, use_7pt=s7)
    vals = G.vals.copy()
    for row in range(G.nrow):
        lo, hi = int(G.row_ptr[row]), int(G.row_ptr[row + 1])
        off = [e for e in range(lo, hi) if G.cols[e] != row]
        if len(off) >= 2:
            vals[off[0]], vals[off[-1]] = vals[off[-1]], vals[off[0]]
    assert vals.tobytes() == G.vals.tobytes()
    row = G.nrow // 2
    assert vc.swap_first_and_last(G, row).tobytes() == G.vals.tobytes()
    # the same rows of a distinct-valued matrix do change
    A = vc.dominant(*dims, s7, True, False, 5)
    assert vc.swap_first_and_last(A, row).tobytes() != A.vals.tobytes()


def test_the_tables_cover_what_the_gpu_tests_are_for():
    one = vc.cases("one")
    forms = {c["name"]: vc.form(c) for c in one}
    for name, want in (("16x16x16", (1, 27, 8)), ("12x10x16_7pt", (1, 7, 4)), ("32x32x33", (1, 27, 66)),
                       ("17x9x10", (1, 27, 3)), ("20x16x8", (1, 27, 5)), ("3x3x100", (1, 27, 2)),
                       ("40x40x1", (1, 9, 4)), ("1x1x700", (1, 3, 2)), ("24x1x30_7pt", (1, 5, 2))):
        assert forms[name] == want, (name, forms[name])
    kinds = {"27": 0, "7": 0, "other": 0, "per-slice": 0, "none": 0}
    for has_a, width, _ in forms.values():
        kinds["none" if not has_a else {27: "27", 7: "7", 0: "per-slice"}.get(width, "other")] += 1
    assert all(v >= 4 for v in kinds.values()), kinds
    for c in one:
        if c["family"] == "csr":
            assert forms[c["name"]][0] == int(c["sorted"]) or vc.matrix(c).nnz == vc.matrix(c).nrow, c["name"]
    for key in ("sym", "dyadic"):
        vals = [c[key] for c in one if c["family"] == "dominant"]
        assert vals.count(True) >= 8 and vals.count(False) >= 8, (key, vals.count(True), vals.count(False))
    assert {c["b"] for c in one} == {"gen", "rand"}
    x0 = [c["x0"] for c in one]
    assert x0.count("zero") >= 8 and x0.count("rand") >= 2 * x0.count("zero") - 8
    assert sum(1 for c in one if vc.tolerance(c) > 0.0) >= 6
    for key, values in list(vc.ONE_OPTIONS.items()) + [("resident_update", (0, 1, -1)), ("nt", (-1, 0, 1))]:
        assert {c["opts"][key] for c in one} == set(values), key
    # the groups: unequal slabs, one-plane members, both stencils
    groups = vc.cases("group")
    assert sum(1 for c in groups if len(set(c["planes"])) > 1) >= 16
    assert sum(1 for c in groups if len(set(c["planes"])) == 1) >= 3
    assert sum(1 for c in groups if min(c["planes"]) == 1) >= 4
    assert {c["s7"] for c in groups} == {False, True} and {c["P"] for c in groups} == {2, 3, 4, 5}
    for key in ("sym", "dyadic"):
        vals = [c[key] for c in groups]
        assert vals.count(True) >= 8 and vals.count(False) >= 8
