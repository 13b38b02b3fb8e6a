"""What tests/test_gpu_columns_edge.py relies on, checked on the CPU: on every
shape and every degenerate or non-finite column of tests/columns_cases.py the
references end at niters 0 with x untouched bit for bit, or at niters 2 with
every x NaN -- so the expected values are exact and the GPU tests need no
tolerance. The plain recurrence is oracle.hpccg (pinned to the reference build
on these starts by test_oracle.py::test_degenerate_starts_match_reference), the
preconditioned one test_gpu_pcg.restated with the column's x0, the refinement
columns_cases.expect_refined.
"""
import numpy as np
import pytest

import columns_cases as cc


@pytest.mark.parametrize("shape", cc.CPU_SHAPES)
def test_references_end_at_zero_or_two_iterations(shape):
    A = cc.csr_of(shape)
    todo = cc.shape_cases(shape, A)
    names = [c[0] for c in todo]
    assert names[:5] == ["exact", "zero_rhs", "exact_negtol", "nan_b", "nan_x0"]
    assert len(names) == 5 + 2 * len(cc.inf_rows(shape))
    rng = np.random.default_rng(17)
    m_any = rng.uniform(0.25, 4.0, A.nrow)
    seen = set()
    for name, b, x0, mi, tol in todo:
        x, it, nr, tr = cc.expect_plain(A, b, x0, mi, tol)
        try:
            cc.degenerate(x, it, nr, tr, x0)
            expected = 2 if name == "exact_negtol" or name.startswith("inf_b_") else 0
            assert it == expected, (it, expected)
            for minv in (None, m_any):  # Jacobi, a caller's m
                xp, itp, nrp, trp = cc.expect_pcg(A, b, x0, mi, tol, minv)
                cc.degenerate(xp, itp, nrp, trp, x0)
                assert itp == it and np.isnan(nrp) == np.isnan(nr), (itp, it, nrp, nr)
                assert np.array_equal(xp, x, equal_nan=True)
        except AssertionError as e:
            raise AssertionError(f"{shape}/{name}: {e}") from None
        seen.add(it)
    assert seen == {0, 2}


@pytest.mark.parametrize("shape", cc.REFINED + ["p2_plain_csr513"])
def test_the_refinement_ends_at_its_first_residual_step(shape):
    """A residual that is not finite or exactly zero: no sweep, x bitwise x0
    (a -0.0 included), normr that residual."""
    A = cc.csr_of(shape)
    assert not np.array_equal(cc.fp32_image(A).vals, A.vals)  # the refinement's kind of matrix
    for name, b, x0, mi, tol in cc.shape_cases(shape, A):
        x0 = x0.copy()
        if x0[5] == 0.0:
            x0[5] = -0.0
        x, it, nr, tr, (its, res) = cc.expect_refined(A, b, x0, mi, tol)
        assert it == 0 and len(its) == 0 and len(tr) == 0 and len(res) == 1, (shape, name, it, its)
        assert nr == 0.0 or not np.isfinite(nr), (shape, name, nr)
        assert (nr == 0.0) == (name in ("exact", "zero_rhs", "exact_negtol")), (shape, name, nr)
        assert x.tobytes() == x0.tobytes(), (shape, name)


def test_the_refinement_restated_converges():
    """The restatement is the algorithm, not only its stop rule: on the finite
    column it reaches the fp64 residual in 2 to 4 sweeps (the bounds of
    test_gpu_mixed.test_refinement_reaches_the_fp64_residual)."""
    A = cc.csr_of("plain_csr513")
    tol = 1e-12 * float(np.linalg.norm(A.b))
    x, it, nr, tr, (its, res) = cc.expect_refined(A, A.b, np.zeros(A.nrow), 4000, tol)
    assert nr <= tol and 2 <= len(its) <= 4 and int(its.sum()) == it and len(res) == len(its) + 1
    assert len(tr) == it + len(its)
    assert float(np.max(np.abs(x - A.xexact))) <= 1e-9


def test_arrangements_cover_what_the_gpu_suite_promises():
    names = [c[0] for c in cc.shape_cases("16c")]
    arr = cc.arrangements(names)
    by_n = {}
    for label, cols, tol in arr:
        by_n.setdefault(len(cols), []).append(cols)
        assert (tol == -1.0) == ("exact_negtol" in cols)
    assert [c.index("nan_b") for c in by_n[4][:4]] == [0, 1, 2, 3]
    assert {c for cols in by_n[4] for c in cols if isinstance(c, str)} == set(names)
    assert [[isinstance(c, str) for c in cols] for cols in by_n[2]] == [[True, False], [False, True]]
    assert isinstance(by_n[5][0][4], str) and isinstance(by_n[5][1][0], str)
    assert sum(isinstance(c, str) for c in by_n[3][0]) == 2 and len(set(by_n[3][0])) == 3
