"""What tests/test_gpu_columns_fuzz.py and tests/test_gpu_columns_group_fuzz.py
rely on, pinned without a GPU (the tables and references of
tests/columns_fuzz.py):

  * the tables are deterministic: 48 drawn and 13 pinned one-rank cases, 32
    groups;
  * reference spread: for every case, every library it is run with and every
    column, the restatement run with the sequential dot and with a second order
    (np.dot; for a group the members' sequential sums added in rank order)
    gives equal niters, rtrans traces within a tenth of the GPU test's bar on
    the part check_trace checks, and x within 1e-10 max(1, max|x|); mixed gives
    the same per-sweep iteration counts. So a GPU solver that differs from the
    restatement by the dot's association alone has nine tenths of the bar left;
  * coverage: the slice counts, column counts, degrees, preconditioners, early
    stops, image forms and exactness the GPU tests are there for do occur;
  * the two ways reference() spells the plain recurrence are the same bits.

Worst spread over the tables (test_worst_spread_is_reported's output: relative
on rtrans against the bar 1e-9, 1e-8 for a group; on x relative to
max(1, max|x|) against 1e-10; the case beside it):
  one   batch : rtrans 1.1e-12 (32x32x33), x 8.7e-11 (o14)
  one   mixed : rtrans 1.3e-10 (o36), x 8.7e-11 (o14)
  one   pcg   : rtrans 4.4e-10 (o31), x 1.8e-11 (o31)
  one   srcg  : rtrans 1.5e-10 (o31), x 2.9e-11 (o1)
  one   poly  : rtrans 1.1e-12 (32x32x32), x 1.3e-11 (o9)
  one   poly32: rtrans 1.1e-12 (32x32x32), x 6.2e-12 (o9)
  group batch : rtrans 4.8e-12 (g17), x 1.0e-12 (g27)
  group pcg   : rtrans 1.3e-11 (g4), x 9.8e-12 (g10)
  group poly  : rtrans 4.8e-12 (g17), x 4.8e-13 (g27)
  group poly32: rtrans 4.8e-12 (g17), x 4.1e-13 (g27)
28 of the 80 first draws missed the condition and were redrawn
(columns_fuzz.REDRAW lists each with its figures): mostly the unpreconditioned
recurrence on a scaled matrix, where the trajectory amplifies the last bit of a
dot. (The pinned 24x1x30 7-pt runs unscaled for the same reason: scaled by
powers of two its batch columns disagreed by 1.1e-8 on x.)
"""
import numpy as np
import pytest

import columns_fuzz as cf
import oracle
from conftest import RTRANS_CUTOFF, RTRANS_RTOL_1GPU, RTRANS_RTOL_MULTI

ALL = cf.cases("one") + cf.cases("group")
_worst = {}


def test_the_tables_are_deterministic():
    assert len(cf.cases("one")) == 48 + len(cf.PINNED) and len(cf.PINNED) == 13
    assert len(cf.cases("group")) == 32
    assert cf._one_cases() == cf.cases("one") and cf._group_cases() == cf.cases("group")
    assert len({c["name"] for c in ALL}) == len(ALL)
    for c in ALL:
        assert 1 <= c["max_iter"] <= 60 and 1 <= c["nrhs"] <= 9 and 1 <= c["nrhs_a"] <= 9 and 0 <= c["pad"] <= 5
        assert 0 <= c["degree"] <= 4
        assert sum(1 for col in c["cols"] if col[2] == "exact") <= 1 and c["cols"][0][2] != "exact"
        assert cf.matrix(c).nrow <= 36000


def trace_spread(tr_a, tr_b):
    """Largest relative difference on rtrans over the part check_trace checks."""
    if not len(tr_a):  # (mixed with no iteration to spend: no inner trace)
        return 0.0
    r0 = tr_a[0] ** 2
    worst = 0.0
    for k in range(min(len(tr_a), len(tr_b))):
        rr = tr_a[k] ** 2
        if rr < RTRANS_CUTOFF * r0:
            break
        worst = max(worst, abs(tr_b[k] ** 2 - rr) / rr if rr > 0 else abs(tr_b[k] ** 2 - rr))
    return worst


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_reference_spread(case):
    A = cf.matrix(case)
    tol = cf.tolerance(case)
    bar = 0.1 * (RTRANS_RTOL_1GPU if case["kind"] == "one" else RTRANS_RTOL_MULTI)
    for lib in cf.libs(case, A):
        first = cf.case_reference(case, lib, tol)
        second = cf.case_reference(case, lib, tol, cf.second_dot(case))
        for c, (a, b) in enumerate(zip(first, second)):
            assert a[1] == b[1], (lib, c, a[1], b[1])
            assert len(a[3]) == len(b[3]), (lib, c)
            ts = trace_spread(a[3], b[3])
            xs = float(np.max(np.abs(a[0] - b[0]))) / max(1.0, float(np.max(np.abs(a[0]))))
            w = _worst.setdefault((case["kind"], lib), [0.0, "", 0.0, ""])
            if ts > w[0]:
                w[0], w[1] = ts, case["name"]
            if xs > w[2]:
                w[2], w[3] = xs, case["name"]
            assert ts <= bar, (lib, c, ts)
            assert xs <= 1e-10, (lib, c, xs)
            if lib == "mixed":
                assert a[4][0].tobytes() == b[4][0].tobytes(), (c, a[4][0], b[4][0])


def test_worst_spread_is_reported():
    print()
    for (kind, lib), w in sorted(_worst.items()):
        print(f"{kind:5s} {lib:6s}: rtrans {w[0]:.1e} ({w[1]}), x {w[2]:.1e} ({w[3]})")


def test_both_spellings_of_the_plain_recurrence_are_the_same_bits():
    """reference("batch") is oracle.hpccg in the sequential order and
    test_gpu_pcg.restated with m = 1 in any other: the same recurrence."""
    for name in ("o0", "o5", "17x9x10", "g3"):
        case = cf.by_name(name)
        A = cf.matrix(case)
        B, X0 = cf.columns(case, A)
        for c in range(min(3, B.shape[0])):
            a = cf.reference("batch", A, B[c], X0[c], None, 0, case["max_iter"], 0.0, "seq")
            b = cf.reference("batch", A, B[c], X0[c], None, 0, case["max_iter"], 0.0, oracle.ddot)
            assert a[1] == b[1] and np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes()
            assert a[0].tobytes() == b[0].tobytes() and np.asarray(a[3]).tobytes() == np.asarray(b[3]).tobytes()


def test_the_tables_cover_what_the_gpu_tests_are_for():
    one = cf.cases("one")
    forms = {c["name"]: cf.form(cf.matrix(c)) for c in one}
    slices = {f[2] for f in forms.values()}
    assert {1, 2, 3, 5, 7, 9, 63, 64, 66} <= slices, sorted(slices)
    for name, want in (("32x32x32", 64), ("32x32x33", 66), ("21x21x73", 63), ("17x9x10", 3), ("20x16x8", 5),
                       ("16x14x16", 7), ("16x16x18", 9)):
        assert forms[name][2] == want and forms[name][:2] == (1, 27), (name, forms[name])
    for name, width in (("40x40x1", 9), ("2x2x300", 15), ("3x3x100", 27), ("1x1x700", 3), ("1x24x24_7pt", 5),
                        ("24x1x30_7pt", 5)):
        assert forms[name][:2] == (1, width) and forms[name][2] > 1, (name, forms[name])
    # every image form on more than one slice
    multi = {f[:2] for f in forms.values() if f[2] > 1}
    assert {(1, 27), (1, 7), (1, 0), (0, None)} <= multi, sorted(multi, key=str)
    assert any(f[0] == 1 and f[1] not in (0, 7, 27) for f in multi)
    # both outcomes of an ascending CSR, recorded
    asc = {c["name"]: forms[c["name"]][0] for c in one if c["family"] == "csr" and c["sorted"]}
    assert set(asc.values()) == {0, 1}, asc
    for c in one:
        if c["family"] == "csr" and not c["sorted"] and cf.matrix(c).nnz > cf.matrix(c).nrow:
            assert forms[c["name"]][0] == 0, c["name"]
    for kind in ("one", "group"):
        table = cf.cases(kind)
        nrhs = [c["nrhs"] for c in table]
        for k in range(1, 10):
            assert nrhs.count(k) >= 2, (kind, k, nrhs.count(k))
        assert {c["degree"] for c in table} == {0, 1, 2, 3, 4}
        assert {c["precond"] for c in table} == {"jacobi", "caller", "pow2"}
        assert {c["bounds"] for c in table} == {False, True}
        # the workspace grows in some cases and is reused in others
        assert any(c["nrhs"] > c["nrhs_a"] for c in table) and any(c["nrhs"] <= c["nrhs_a"] for c in table)
        # the chunkings 4+1, 4+2, 4+4 (seven columns: one idle), 4+4 and 4+4+1 of for_chunks
        assert {5, 6, 7, 8, 9} <= set(nrhs)
        # a tolerance that ends one column early while another runs on, read from the reference
        split = 0
        for c in table:
            tol = cf.tolerance(c)
            if tol > 0.0:
                its = [r[1] for r in cf.case_reference(c, "batch", tol)]
                full = c["max_iter"] - 1
                split += any(0 < i < full for i in its) and any(i > j for i in its for j in its if 0 < j < full)
        assert split >= 3, (kind, split)
        exact = [cf.exact32(cf.matrix(c)) for c in table]
        assert exact.count(True) >= 6 and exact.count(False) >= 6, (kind, exact.count(True), exact.count(False))
    # the groups: stencils and CSR slabs, both row orders, a member below one slice, cuts off the slice boundaries
    groups = cf.cases("group")
    assert {c["family"] for c in groups} == {"stencil", "csr"}
    csr = [c for c in groups if c["family"] == "csr"]
    assert {c["sorted"] for c in csr} == {False, True}
    for c in csr:
        assert min(c["slabs"]) < cf.SLICE and c["band"] <= min(c["slabs"]) and len(set(c["slabs"])) > 1
        assert any(s % cf.SLICE for s in np.cumsum(c["slabs"])[:-1])


def test_mixed_is_given_no_p10_case_and_diagonal_matrices_go_to_batch_alone():
    seen = 0
    for c in cf.cases("one"):
        A = cf.matrix(c)
        run = cf.libs(c, A)
        if cf.fully_diagonal(A):
            assert run == ("batch",), (c["name"], run)
            continue
        assert ("mixed" in run) == (c["scaling"] != "p10")
        assert set(cf.PRECONDITIONED) <= set(run)
        seen += "mixed" in run
    assert seen >= 12
