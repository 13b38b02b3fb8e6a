"""Seeded sweep of the group multi-column solvers (group batch, pcg, poly,
poly32) over the 32 groups of tests/columns_fuzz.py: stencil groups through
group_generate (P in 2..5, nx, ny in 1..16, nz in 1..8 per member, both
stencils) and banded random SPD CSR through group_from_csr, cut at unequal
boundaries that are mostly not slice boundaries, one member below one slice,
the band no wider than the smallest slab, rows in random (SELL) or ascending
order (A image), unscaled or scaled by powers of two or of ten. One test per
group, every library on it:

  * against the one-rank restatement on the global matrix, every column:
    termination after conftest.check_final's rule (columns_fuzz.check_end), the
    trace by check_trace at RTRANS_RTOL_MULTI, x within 1e-9 max(1, max|x_ref|),
    with ld > n the words between the columns untouched, for a call with nrhs_a
    and then one with nrhs columns on the same members. The restatements differ
    from themselves by a tenth of the bar at most between the sequential dot and
    the group's order (tests/test_columns_fuzz_cpu.py);
  * poly32: the restatement with the fp32 values inside the polynomial, and
    group_poly32_info's per-member verdicts are NumPy's;
  * one column of a group call is bitwise the same call with that column alone;
  * a group batch column is bitwise group_HPCCG of that column alone, whose
    trace every member reports identically (the column libraries keep one
    trace per group, of the all-reduced scalars);
  * degree 0 of group poly is group pcg bit for bit, m = 1 of group pcg is
    group batch.
"""
import numpy as np
import pytest

import columns_fuzz as cf
import test_gpu_batch_group as tbg
import test_gpu_pcg_group as tpg
import test_gpu_poly32_group as tpoly32g
import test_gpu_poly_group as tpolyg
from conftest import RTRANS_RTOL_MULTI, check_trace
from test_gpu_pcg_group import assert_same

pytestmark = pytest.mark.gpu

CASES = cf.cases("group")


def live(hp):
    return (hp.batch_live_workspaces(), hp.group_pcg_live_workspaces(), hp.group_poly_live_workspaces(),
            hp.group_poly32_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _workspaces_are_back(hp):
    base = live(hp)
    yield
    assert live(hp) == base


class Group:
    """The members of a case with what the solve helpers of the group suites read (Ms, rows, N, split)."""

    def __init__(self, hp, case):
        self.A = A = cf.matrix(case)
        self.rows = cf.rows_of_members(case)
        self.N = A.nrow
        if cf.generated(case):
            self.Ms = hp.group_generate(*case["dims"], case["P"], use_7pt=case["s7"])
        else:
            self.Ms = tpg.members_from_csr(hp, A, cf.counts(case))
        self.P = len(self.Ms)
        assert [int(M.info()["nrow"]) for M in self.Ms] == cf.counts(case)

    def split(self, a):
        return [np.ascontiguousarray(a[:, rw]) for rw in self.rows]

    def close(self):
        for M in self.Ms:
            M.close()


def solver(hp, gpu, case, cs, lib):
    tol = cf.tolerance(case)
    pad = case["pad"]
    minv = cf.precond(case, cs.A)[0]
    lmin, lmax = cf.passed_bounds(case, cs.A)

    def solve(B, X0, degree=case["degree"], m=minv):
        if lib == "batch":
            return tbg.batch_solve(hp, gpu, cs, B, X0, case["max_iter"], tol, pad=pad)
        if lib == "pcg":
            return tpg.pcg_solve(hp, gpu, cs, B, X0, case["max_iter"], tol, minv=m, pad=pad)
        f = tpolyg.poly_solve if lib == "poly" else tpoly32g.poly32_solve
        return f(hp, gpu, cs, B, X0, case["max_iter"], tol, degree=degree, lmin=lmin, lmax=lmax, minv=m, pad=pad)
    return solve


def check_columns(lib, got, ref, max_iter, what):
    assert len(got) == len(ref)
    for c, (g, r) in enumerate(zip(got, ref)):
        where = (lib, what, c)
        x = np.concatenate(g[0])
        cf.check_end((x,) + tuple(g[1:]), r, max_iter)
        assert len(g[3]) == g[1] + 1, where
        check_trace(g[3], r[3], RTRANS_RTOL_MULTI)
        scale = max(1.0, float(np.max(np.abs(r[0]))))
        err = float(np.max(np.abs(x - r[0])))
        assert err <= 1e-9 * scale, (where, err, scale)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_group(hp, gpu, case):
    A = cf.matrix(case)
    B, X0 = cf.columns(case, A)
    na, nb = case["nrhs_a"], case["nrhs"]
    tol = cf.tolerance(case)
    run = cf.libs(case, A)
    cs = Group(hp, case)
    try:
        if case["family"] == "csr":  # the members' image forms are the ones their rows predict
            for M, rw in zip(cs.Ms, cs.rows):
                assert int(M.get_option("has_a")) == cf.form(A, rw.start, rw.stop)[0], (rw, cf.form(A, rw.start, rw.stop))
        last = {}
        alone = nb - 1 - case["pad"] % nb  # the column that is also solved by itself
        for lib in run:
            solve = solver(hp, gpu, case, cs, lib)
            ref = cf.case_reference(case, lib, tol)
            check_columns(lib, solve(B[:na], X0[:na]), ref[:na], case["max_iter"], "first call")
            last[lib] = solve(B[:nb], X0[:nb])
            check_columns(lib, last[lib], ref[:nb], case["max_iter"], "second call")
            assert_same(solve(B[alone:alone + 1], X0[alone:alone + 1]), last[lib][alone:alone + 1])
        k = min(nb, 2)
        assert_same(last["batch"][:k], tbg.single_solves(hp, gpu, cs, B[:k], X0[:k], case["max_iter"], tol))
        if "pcg" in run:
            assert_same(solver(hp, gpu, case, cs, "pcg")(B[:nb], X0[:nb], m=1.0), last["batch"])
            poly0 = last["poly"] if case["degree"] == 0 else solver(hp, gpu, case, cs, "poly")(B[:nb], X0[:nb], degree=0)
            assert_same(poly0, last["pcg"])
            info = hp.group_poly32_info(cs.Ms)
            verdicts = [int(cf.exact32(A, rw.start, rw.stop)) for rw in cs.rows]
            assert [i["exact"] for i in info] == verdicts, (info, verdicts)
            if all(verdicts):
                assert_same(last["poly32"], last["poly"])
    finally:
        cs.close()
