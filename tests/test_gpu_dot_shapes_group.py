"""The group solvers where a member's dot completion changes shape: the
store_total arm of col_finalize and srcg_finalize (a member's totals go to
tot[] and the group's sum kernel adds them in rank order) at the sizes of
tests/dot_shapes.py. Two groups:

  csr_g65_g17  unequal members from the CSR with a value of its own at every
               entry, n = 2097153 + 524837 rows cut after row 2097153 by
               group_from_csr: member 0 is g65 (a second round of one group of
               one slice of one row), member 1 is g17; the halo is one row;
  gen_g65_g65  group_generate(1, 1, 2097153, 2): equal members, generated on
               the device.

Group batch, pcg, srcg, poly and poly32 are called with 1 and then 3 columns
(dot_shapes.columns: every member's last slice of b is scaled up) under a
caller's m and held to columns_fuzz.reference under the group's dot order
(test_gpu_poly32_group.rank_dot) by test_gpu_columns_group_fuzz.check_columns
at RTRANS_RTOL_MULTI: all three columns of the CSR group, column 0 of the
generated one (4.2 M rows). Bit for bit: a group batch column is group_HPCCG of
it, whose trace every member reports identically; m = 1 of group pcg is group
batch; degree 0 of group poly is group pcg; group srcg with max_iter 2 is group
pcg. On the generated group trace[0] with x0 = 0 and b = A 1 is the square root
of KAT-2's integer in every library and on every member of group_HPCCG. A group
of one member at g65 is bitwise the one-rank library, for all five.
"""
import numpy as np
import pytest

import columns_fuzz as cf
import dot_shapes as ds
import test_gpu_batch_group as tbg
import test_gpu_pcg_group as tpg
import test_gpu_poly32_group as tpoly32g
import test_gpu_poly_group as tpolyg
from test_gpu_columns_group_fuzz import check_columns
from test_gpu_dot_shapes import run
from test_gpu_pcg_group import assert_same
from test_gpu_poly32_group import rank_dot
from test_gpu_srcg_group import srcg_solve

pytestmark = pytest.mark.gpu


def live(hp):
    return (hp.batch_live_workspaces(), hp.group_pcg_live_workspaces(), hp.group_srcg_live_workspaces(),
            hp.group_poly_live_workspaces(), hp.group_poly32_live_workspaces(), hp.pcg_live_workspaces(),
            hp.srcg_live_workspaces(), hp.poly_live_workspaces(), hp.poly32_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _workspaces_are_back(hp):
    base = live(hp)
    yield
    ds.release()
    assert live(hp) == base


class Members:
    """A group with what the solve helpers of the group suites read (Ms, rows, N, split)."""

    def __init__(self, Ms, rows):
        self.Ms, self.rows, self.P, self.N = Ms, rows, len(Ms), rows[-1].stop
        assert [int(M.info()["nrow"]) for M in Ms] == [rw.stop - rw.start for rw in rows]

    def split(self, a):
        return [np.ascontiguousarray(a[:, rw]) for rw in self.rows]

    def close(self):
        for M in self.Ms:
            M.close()


def group_run(hp, gpu, lib, cs, B, X0, max_iter, m=None, degree=ds.DEGREE):
    """[(xs per member, niters, normr, trace)] per column; m: None (Jacobi), a number or a global array."""
    if lib == "batch":
        return tbg.batch_solve(hp, gpu, cs, B, X0, max_iter)
    if lib == "pcg":
        return tpg.pcg_solve(hp, gpu, cs, B, X0, max_iter, minv=m)
    if lib == "srcg":
        return srcg_solve(hp, gpu, cs, B, X0, max_iter, minv=m)
    f = tpolyg.poly_solve if lib == "poly" else tpoly32g.poly32_solve
    return f(hp, gpu, cs, B, X0, max_iter, degree=degree, minv=m)


@pytest.mark.parametrize("name", list(ds.GROUPS))
def test_group(hp, gpu, name):
    c = ds.case(name)
    max_iter = c["max_iter"]
    A = ds.matrix(name)
    B, X0 = ds.columns(name)
    minv = cf.precond(c, A)[0]
    rows = ds.members(name)
    if c["csr"]:
        cs = Members(tpg.members_from_csr(hp, A, ds.counts(name)), rows)
    else:
        cs = Members(hp.group_generate(*c["dims"], c["P"]), rows)
    try:
        for M, rw in zip(cs.Ms, rows):
            assert (int(M.get_option("has_a")), int(M.get_option("a_width"))) == (1, 3)
            assert ds.plan(rw.stop - rw.start).ng in (17, 65)
        held = len(c["held"])
        last = {}
        for lib in ds.GROUP_LIBS:
            ref = ds.references(c, lib, dot=rank_dot(rows))
            first = group_run(hp, gpu, lib, cs, B[:1], X0[:1], max_iter, m=minv)
            last[lib] = group_run(hp, gpu, lib, cs, B, X0, max_iter, m=minv)
            check_columns(lib, first, ref[:1], max_iter, "first call")
            check_columns(lib, last[lib][:held], ref, max_iter, "second call")
            assert_same(last[lib][:1], first)
        assert_same(last["batch"], tbg.single_solves(hp, gpu, cs, B, X0, max_iter))
        assert_same(group_run(hp, gpu, "pcg", cs, B, X0, max_iter, m=1.0), last["batch"])
        assert_same(group_run(hp, gpu, "poly", cs, B, X0, max_iter, m=minv, degree=0), last["pcg"])
        assert_same(group_run(hp, gpu, "srcg", cs, B, X0, 2, m=minv), group_run(hp, gpu, "pcg", cs, B, X0, 2, m=minv))
        if not c["csr"]:  # b = A 1 (oracle.generate's b, exact) and x0 = 0: the integer, in any order of the sums
            want = np.sqrt(np.float64(ds.rr0(name)))
            B1, Z = A.b[None].copy(), np.zeros((1, A.nrow))
            for lib in ds.GROUP_LIBS:
                got = group_run(hp, gpu, lib, cs, B1, Z, 2)
                assert got[0][3][0] == want, (lib, got[0][3][0], want)
            # (single_solves asserts that every member reports this trace)
            assert tbg.single_solves(hp, gpu, cs, B1, Z, 2)[0][3][0] == want
    finally:
        cs.close()
        ds.release(name)


def test_group_of_one_at_g65_is_the_one_rank_library(hp, gpu):
    """nranks == 1 runs the same code on a halo-free matrix: 0.0 + a total is the total."""
    n = ds.nrows("g65")
    B, X0 = ds.columns("g65")
    m = np.random.default_rng(65).uniform(0.25, 4.0, n)
    M = hp.Matrix.generate(*ds.TABLE["g65"][0])
    try:
        cs = Members([M], [slice(0, n)])
        for lib in ds.GROUP_LIBS:
            for k in (1, 3):
                got = group_run(hp, gpu, lib, cs, B[:k], X0[:k], 4, m=m)
                ref = run(hp, gpu, lib, M, B[:k], X0[:k], 4, m=m)
                assert_same(got, [([r[0]],) + tuple(r[1:4]) for r in ref])
    finally:
        M.close()
        ds.release("g65")
