"""HPCCG_srpoly and group_HPCCG_srpoly at the problem sizes where a dot's
completion changes shape (tests/dot_shapes.py: g17, g65, g257 and the two
groups of tests/test_gpu_dot_shapes_group.py). The three-dot finalize
(srcg_finalize: r.r, r.u, u.w from their slice partials, with store_total on a
group member) is checked at degree 2, where the r.u slice partial comes from
the last Chebyshev step and the u.w one from the SpMM of z buffer 0, and at
degree 0, where both come from hpccg_srcg_bodies.h's step:

  * one column, then three on the same matrix (the workspace grows): column c
    of the second call is bitwise the one-column call;
  * degree 0 is (group_)HPCCG_srcg bit for bit, which the modules of the other
    libraries hold to its restatement at these sizes;
  * degree 2 under a caller's m is held to test_gpu_srpoly.restated_srpoly on
    the columns dot_shapes holds, by the helpers' check_columns at their bars
    (RTRANS_RTOL_1GPU; a group: the restatement under the group's dot order at
    RTRANS_RTOL_MULTI), and with max_iter 2 it is (group_)HPCCG_poly bit for bit.
"""
import numpy as np
import pytest

import columns_fuzz as cf
import dot_shapes as ds
import test_gpu_columns_fuzz as tcf
import test_gpu_columns_group_fuzz as tcgf
import test_gpu_pcg_group as tpg
from test_gpu_dot_shapes import build, run
from test_gpu_dot_shapes_group import Members, group_run
from test_gpu_mixed import assert_same
from test_gpu_poly32_group import rank_dot
from test_gpu_srpoly import restated_srpoly, srpoly_solve
from test_gpu_srpoly_group import srpoly_solve as group_srpoly_solve

pytestmark = pytest.mark.gpu

SHAPES = ["g17", "g65", "g257"]


def live(hp):
    return (hp.srpoly_live_workspaces(), hp.group_srpoly_live_workspaces(), hp.srcg_live_workspaces(),
            hp.group_srcg_live_workspaces(), hp.poly_live_workspaces(), hp.group_poly_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _workspaces_are_back(hp):
    base = live(hp)
    yield
    ds.release()
    assert live(hp) == base


def references(c, A, B, X0, dot):
    """restated_srpoly at degree 2 of the columns the case holds, under the case's m and numpy's bound."""
    m = cf.precond(c, A)[1]
    lmin, lmax = cf.bounds(c, A)
    return [restated_srpoly(A, B[k], m, ds.DEGREE, lmin, lmax, c["max_iter"], 0.0, x0=X0[k],
                            dot=lambda x, y: np.float64(dot(x, y))) for k in c["held"]]


@pytest.mark.parametrize("name", SHAPES)
def test_shape(hp, gpu, name):
    import oracle
    c = ds.case(name)
    max_iter = c["max_iter"]
    A = ds.matrix(name)
    n = A.nrow
    B, X0 = ds.columns(name)
    minv = cf.precond(c, A)[0]
    held = list(c["held"])
    assert ds.plan(n).ng in (17, 65, 257)
    M = build(hp, name)
    try:
        for degree in (ds.DEGREE, 0):
            first = srpoly_solve(hp, gpu, M, B[:1], X0[:1], max_iter, degree=degree, minv=minv)
            before = M.srpoly_workspace_bytes()
            second = srpoly_solve(hp, gpu, M, B, X0, max_iter, degree=degree, minv=minv)
            assert M.srpoly_workspace_bytes() > before if degree else M.srpoly_workspace_bytes() == before
            assert_same(second[:1], first)
            assert [g[1] for g in second] == [max_iter - 1] * 3
            for k in held[1:]:
                assert_same(srpoly_solve(hp, gpu, M, B[k:k + 1], X0[k:k + 1], max_iter, degree=degree, minv=minv),
                            second[k:k + 1])
            if degree == 0:
                assert_same(second, run(hp, gpu, "srcg", M, B, X0, max_iter, m=minv))
                continue
            ref = references(c, A, B, X0, oracle.ddot)
            tcf.check_columns("srpoly", [second[k] for k in held], ref, max_iter, "second call")
            assert_same(srpoly_solve(hp, gpu, M, B, X0, 2, degree=degree, minv=minv),
                        run(hp, gpu, "poly", M, B, X0, 2, m=minv, degree=degree))
    finally:
        M.close()
        ds.release(name)


@pytest.mark.parametrize("name", list(ds.GROUPS))
def test_group(hp, gpu, name):
    c = ds.case(name)
    max_iter = c["max_iter"]
    A = ds.matrix(name)
    B, X0 = ds.columns(name)
    minv = cf.precond(c, A)[0]
    rows = ds.members(name)
    held = list(c["held"])
    if c["csr"]:
        cs = Members(tpg.members_from_csr(hp, A, ds.counts(name)), rows)
    else:
        cs = Members(hp.group_generate(*c["dims"], c["P"]), rows)
    try:
        for rw in rows:
            assert ds.plan(rw.stop - rw.start).ng in (17, 65)
        for degree in (ds.DEGREE, 0):
            first = group_srpoly_solve(hp, gpu, cs, B[:1], X0[:1], max_iter, degree=degree, minv=minv)
            second = group_srpoly_solve(hp, gpu, cs, B, X0, max_iter, degree=degree, minv=minv)
            tpg.assert_same(second[:1], first)
            assert [g[1] for g in second] == [max_iter - 1] * 3
            for k in held[1:]:
                tpg.assert_same(group_srpoly_solve(hp, gpu, cs, B[k:k + 1], X0[k:k + 1], max_iter, degree=degree,
                                                   minv=minv), second[k:k + 1])
            if degree == 0:
                tpg.assert_same(second, group_run(hp, gpu, "srcg", cs, B, X0, max_iter, m=minv))
                continue
            ref = references(c, A, B, X0, rank_dot(rows))
            tcgf.check_columns("srpoly", [second[k] for k in held], ref, max_iter, "second call")
            tpg.assert_same(group_srpoly_solve(hp, gpu, cs, B, X0, 2, degree=degree, minv=minv),
                            group_run(hp, gpu, "poly", cs, B, X0, 2, m=minv, degree=degree))
    finally:
        cs.close()
        ds.release(name)
