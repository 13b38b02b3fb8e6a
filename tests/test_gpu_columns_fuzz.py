"""Seeded sweep of the one-rank multi-column solvers (batch, mixed, pcg, srcg,
poly, poly32) over the table of tests/columns_fuzz.py: 48 drawn cases (stencils
of both types with nx, ny in 1..24 and nz in 1..40, random SPD CSR in random
and in ascending row order, each unscaled, scaled by powers of two or of ten,
or perturbed) and 13 pinned shapes (slice counts around the 8 XCDs and the
64-slice dot group, uniform widths other than 27 and 7, 3x3x100). One test per
case; it builds the matrix once and runs every library the case is given
(columns_fuzz.libs) on it:

  * against the committed fp64 restatement of the library, every column:
    termination after conftest.check_final's rule (columns_fuzz.check_end), the
    trace by check_trace at RTRANS_RTOL_1GPU, x within 1e-9 max(1, max|x_ref|),
    and with ld > n the words between the columns untouched. The restatements
    differ from themselves by a tenth of these bars at most when the dot's
    order changes (tests/test_columns_fuzz_cpu.py), and the tolerance of a case
    is at least 1 % away from every residual of every restatement;
  * poly32: the restatement with the fp32 image inside the polynomial
    (restated32; on an exact image that is the fp64 one), and poly32_info's
    verdict is NumPy's;
  * mixed, inexact image: the per-sweep iteration counts of expect_refined, x,
    and normr against the fp64 residual of the returned x recomputed by the
    oracle (they differ in the dot's association only); exact image: the plain
    recurrence, and bitwise the batch columns;
  * HPC_sparsemv_batch and HPC_sparsemv_mixed at the case's nrhs and ld: bitwise
    oracle.sparsemv on the fp64 and on the float-rounded values;
  * what the headers promise bit for bit (x, niters, normr, trace): a batch
    column is HPCCG of that column alone; pcg with m = 1 is batch; poly at
    degree 0 is pcg; poly32 on an exact image is poly; srcg with max_iter <= 2
    is pcg;
  * the workspace: every library is called with nrhs_a and then nrhs columns on
    the same Matrix (it grows in some cases and is kept in others); both calls
    meet the reference and the second is bitwise the same columns on a fresh
    Matrix.

The image form the device reports is the one columns_fuzz.form predicts from
the CSR; test_form_census asserts that widths 27, 7, per-slice, another uniform
width and the SELL form each occur on more than one slice, and prints them.
"""
import numpy as np
import pytest

import columns_fuzz as cf
import oracle
import test_gpu_batch as tb
import test_gpu_mixed as tm
import test_gpu_pcg as tp
import test_gpu_poly as tpoly
import test_gpu_poly32 as tpoly32
import test_gpu_srcg as tsr
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_mixed import assert_same

pytestmark = pytest.mark.gpu

CASES = cf.cases("one")
_census = {}


def live(hp):
    return (hp.batch_live_workspaces(), hp.mixed_live_workspaces(), hp.pcg_live_workspaces(),
            hp.srcg_live_workspaces(), hp.poly_live_workspaces(), hp.poly32_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _workspaces_are_back(hp):
    base = live(hp)
    yield
    assert live(hp) == base


def build(hp, case):
    if cf.generated(case):
        prob = hp.generate_matrix(*case["dims"], use_7pt=case["s7"])
        M = hp.Matrix.from_hpc(prob)
        prob.close()
        return M
    A = cf.matrix(case)
    return hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)


def device_form(M, n):
    has_a = int(M.get_option("has_a"))
    return has_a, (int(M.get_option("a_width")) if has_a else None), (n + cf.SLICE - 1) // cf.SLICE


def solver(hp, gpu, case, A, lib):
    """solve(M, B, X0, max_iter=..., **changes) -> [(x, niters, normr, trace, ...)] of lib under the case's draws."""
    n = A.nrow
    ld = n + case["pad"]
    tol = cf.tolerance(case)
    minv = cf.precond(case, A)[0]
    lmin, lmax = cf.passed_bounds(case, A)

    def solve(M, B, X0, max_iter=case["max_iter"], degree=case["degree"], m=minv):
        if lib == "batch":
            return tb.batch_solve(hp, gpu, M, B, X0, max_iter, tol, ld=ld)
        if lib == "mixed":
            return tm.mixed_solve(hp, gpu, M, B, X0, max_iter, tol, ld=ld)
        if lib == "pcg":
            return tp.pcg_solve(hp, gpu, M, B, X0, max_iter, tol, minv=m, ld=ld)
        if lib == "srcg":
            return tsr.srcg_solve(hp, gpu, M, B, X0, max_iter, tol, minv=m, ld=ld)
        f = tpoly.poly_solve if lib == "poly" else tpoly32.poly32_solve
        return f(hp, gpu, M, B, X0, max_iter, tol, degree=degree, lmin=lmin, lmax=lmax, minv=m, ld=ld)
    return solve


def check_columns(lib, got, ref, max_iter, what):
    assert len(got) == len(ref)
    for c, (g, r) in enumerate(zip(got, ref)):
        where = (lib, what, c)
        cf.check_end(g, r, max_iter)
        assert len(g[3]) == g[1] + 1, where
        check_trace(g[3], r[3], RTRANS_RTOL_1GPU)
        scale = max(1.0, float(np.max(np.abs(r[0]))))
        err = float(np.max(np.abs(g[0] - r[0])))
        assert err <= 1e-9 * scale, (where, err, scale)


def check_refined(A, B, got, ref, what):
    """mixed on an inexact image."""
    for c, (g, r) in enumerate(zip(got, ref)):
        where = ("mixed", what, c)
        assert g[4][0].tobytes() == r[4][0].tobytes(), (where, g[4][0], r[4][0])
        assert g[1] == r[1] == int(np.sum(r[4][0])), where
        scale = max(1.0, float(np.max(np.abs(r[0]))))
        err = float(np.max(np.abs(g[0] - r[0])))
        assert err <= 1e-9 * scale, (where, err, scale)
        res = B[c] + (-1.0) * oracle.sparsemv(A, g[0])
        rr = float(oracle.ddot(res, res))
        assert abs(g[2] ** 2 - rr) <= RTRANS_RTOL_1GPU * rr, (where, g[2] ** 2, rr)


def check_spmm(hp, gpu, case, A, M, mixed):
    import torch
    n, nrhs = A.nrow, case["nrhs"]
    ld = n + case["pad"]
    V = np.random.default_rng(case["col_seed"] + 2).uniform(-1.0, 1.0, (nrhs, n))
    images = [(hp.HPC_sparsemv_batch, A)]
    if mixed:
        images.append((hp.HPC_sparsemv_mixed, tpoly32.fl32(A)))
    for f, At in images:
        Xd = tm.dev(gpu, V, ld)
        Yd = torch.full((nrhs, ld), -3.0, dtype=torch.float64, device=gpu)
        f(M, Xd, Yd)
        Y = Yd.cpu().numpy()
        for c in range(nrhs):
            ref = oracle.sparsemv(At, V[c])
            assert Y[c, :n].tobytes() == ref.tobytes(), (f.__name__, c, float(np.max(np.abs(Y[c, :n] - ref))))
        assert np.all(Y[:, n:] == -3.0), f.__name__
        assert Xd.cpu().numpy()[:, :n].tobytes() == V.tobytes()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_case(hp, gpu, case):
    A = cf.matrix(case)
    n = A.nrow
    B, X0 = cf.columns(case, A)
    na, nb = case["nrhs_a"], case["nrhs"]
    tol = cf.tolerance(case)
    max_iter = case["max_iter"]
    run = cf.libs(case, A)
    exact = cf.exact32(A)
    M, fresh = build(hp, case), build(hp, case)
    try:
        got_form = device_form(M, n)
        _census[case["name"]] = got_form
        assert got_form == cf.form(A), (got_form, cf.form(A))
        last = {}
        for lib in run:
            solve = solver(hp, gpu, case, A, lib)
            ref = cf.case_reference(case, lib, tol)
            held = getattr(M, lib + "_workspace_bytes")
            first = solve(M, B[:na], X0[:na])
            before = held()
            second = solve(M, B[:nb], X0[:nb])
            # the workspace is kept for no more columns than it has held, and never shrinks
            # (a batch of one column is the single solve itself and holds no vectors)
            assert held() == before if nb <= na else held() >= before, (lib, na, nb, before, held())
            assert held() > 0 or (lib == "batch" and max(na, nb) == 1), (lib, na, nb)
            for what, got, k in (("first call", first, na), ("second call", second, nb)):
                if lib == "mixed" and not exact:
                    check_refined(A, B, got, ref[:k], what)
                else:
                    check_columns(lib, got, ref[:k], max_iter, what)
            assert_same(second, solve(fresh, B[:nb], X0[:nb]), sweeps=lib == "mixed")
            last[lib] = second
        check_spmm(hp, gpu, case, A, M, "mixed" in run)
        # the identities of the headers
        assert_same(last["batch"], tm.single_solves(hp, gpu, M, B[:nb], X0[:nb], max_iter, tol))
        if "mixed" in run:
            assert M.mixed_info()["exact"] == int(exact)
            if exact:
                assert_same([g[:4] for g in last["mixed"]], last["batch"])
        if "pcg" in run:
            pcg = solver(hp, gpu, case, A, "pcg")
            assert_same(pcg(M, B[:nb], X0[:nb], m=1.0), last["batch"])
            poly0 = last["poly"] if case["degree"] == 0 else solver(hp, gpu, case, A, "poly")(M, B[:nb], X0[:nb], degree=0)
            assert_same(poly0, last["pcg"])
            assert hp.poly32_info(M)["exact"] == int(exact)
            if exact:
                assert_same(last["poly32"], last["poly"])
            short = min(max_iter, 2)
            assert_same(solver(hp, gpu, case, A, "srcg")(M, B[:nb], X0[:nb], max_iter=short),
                        pcg(M, B[:nb], X0[:nb], max_iter=short))
    finally:
        M.close()
        fresh.close()


def test_form_census(hp, gpu):
    """(has_a, a_width, nslices) over the table: every form on more than one slice."""
    for case in CASES:
        if case["name"] not in _census:
            M = build(hp, case)
            try:
                _census[case["name"]] = device_form(M, cf.matrix(case).nrow)
            finally:
                M.close()
    kinds = {"width 27": lambda f: f[:2] == (1, 27), "width 7": lambda f: f[:2] == (1, 7),
             "per-slice": lambda f: f[:2] == (1, 0), "another uniform width": lambda f: f[0] == 1 and f[1] not in (0, 7, 27),
             "SELL": lambda f: f[0] == 0}
    print()
    for kind, is_kind in kinds.items():
        found = sorted({(f[1], f[2]) for f in _census.values() if is_kind(f)}, key=str)
        print(f"{kind}: (a_width, nslices) {found}")
        assert any(s > 1 for _, s in found), kind
    assert _census["3x3x100"] == (1, 27, 2), _census["3x3x100"]
    for name, width in (("40x40x1", 9), ("2x2x300", 15), ("1x1x700", 3), ("1x24x24_7pt", 5), ("24x1x30_7pt", 5)):
        assert _census[name][:2] == (1, width) and _census[name][2] > 1, (name, _census[name])
    slices = {f[2] for f in _census.values()}
    assert {1, 2, 3, 5, 7, 9, 63, 64, 66} <= slices, sorted(slices)
