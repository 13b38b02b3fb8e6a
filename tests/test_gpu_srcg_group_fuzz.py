"""Seeded sweep of the group single-reduction solver (group_HPCCG_srcg) over
the 32 groups of tests/columns_fuzz.py (the groups of
tests/test_gpu_columns_group_fuzz.py: stencil groups and banded random SPD CSR
cut at unequal boundaries, both row orders, unscaled or scaled by powers of two
or of ten). One test per group:

  * every column against the one-rank restatement on the global matrix
    (columns_fuzz.case_reference(case, "srcg", tol)): termination by
    columns_fuzz.check_end, the trace by check_trace at RTRANS_RTOL_MULTI, x
    within 1e-9 max(1, max|x_ref|), with ld > n the words between the columns
    untouched, for a call with nrhs_a and then one with nrhs columns on the
    same members. The restatement differs from itself by a tenth of the bars at
    most between the sequential dot and the group's order, and every case's
    tolerance is at least 1 % away from its residuals
    (tests/test_srcg_group_cpu.py), so no case is left out;
  * one column of a group call is bitwise the same call with that column alone;
  * with max_iter <= 2 the call is group_HPCCG_pcg bit for bit.
"""
import pytest

import columns_fuzz as cf
import test_gpu_pcg_group as tpg
from test_gpu_columns_group_fuzz import Group, check_columns
from test_gpu_pcg_group import assert_same
from test_gpu_srcg_group import srcg_solve

pytestmark = pytest.mark.gpu

CASES = cf.cases("group")


def live(hp):
    return (hp.group_srcg_live_workspaces(), hp.group_pcg_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _workspaces_are_back(hp):
    base = live(hp)
    yield
    assert live(hp) == base


def test_every_group_is_run():
    assert len(CASES) == 32 and len({c["name"] for c in CASES}) == 32


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_group(hp, gpu, case):
    A = cf.matrix(case)
    B, X0 = cf.columns(case, A)
    na, nb = case["nrhs_a"], case["nrhs"]
    tol = cf.tolerance(case)
    pad = case["pad"]
    minv = cf.precond(case, A)[0]
    ref = cf.case_reference(case, "srcg", tol)
    cs = Group(hp, case)
    try:
        def solve(B, X0, max_iter=case["max_iter"], t=tol):
            return srcg_solve(hp, gpu, cs, B, X0, max_iter, t, minv=minv, pad=pad)

        check_columns("srcg", solve(B[:na], X0[:na]), ref[:na], case["max_iter"], "first call")
        last = solve(B[:nb], X0[:nb])
        check_columns("srcg", last, ref[:nb], case["max_iter"], "second call")
        alone = nb - 1 - pad % nb  # the column that is also solved by itself
        assert_same(solve(B[alone:alone + 1], X0[alone:alone + 1]), last[alone:alone + 1])
        # the first iteration is the group pcg's
        for max_iter in sorted({min(case["max_iter"], 2), 1}):
            pcg = tpg.pcg_solve(hp, gpu, cs, B[:nb], X0[:nb], max_iter, tol, minv=minv, pad=pad)
            assert_same(solve(B[:nb], X0[:nb], max_iter), pcg)
    finally:
        cs.close()
