"""Chebyshev polynomial preconditioned CG whose steps stream an fp32 image of
the matrix (include/hpccg_hip_poly32.h, lib/libhpccg_hip_poly32.so): the
recurrence of hpccg_hip_poly.h with A~ = fl32(A) inside the polynomial, the
outer SpMM from the fp32 image only where that image is the matrix.

  1. every image form is exercised; poly32_info's verdict and count are NumPy's;
  2. on exact images every column is HPCCG_poly bit for bit, degrees 0 to 4;
  3. degree 0 is the pcg library bit for bit on every inexact image;
  4. on inexact images: the NumPy restatement with A~ inside P (trace, niters
     under a tolerance, x against xexact), degrees 1 to 4;
  5. it keeps what the polynomial is for: HPCCG_poly's iteration count, less
     than half of Jacobi's;
  6. column c of a multi-column call is bitwise the single-column call;
  7. degenerate columns beside ordinary ones;
  8. matrices outside fp32 range are refused;
  9. host solve, a caller's m, the workspace's life, the other libraries.

Shapes and helpers: those of test_gpu_poly.py, test_gpu_pcg.py and
test_gpu_mixed.py.

4.: the restatement (restated32 below) run on the CPU with two dot orders (a
sequential sum, oracle.ddot, and numpy's blocked one, np.dot) agrees with itself
on the checked part of the rtrans trace, worst over degrees 1 to 4, to
4.2e-11 (16c), 2.4e-12 (33c), 1.9e-14 (7pt), 2.0e-13 (band600), 3.7e-14
(csr513), 8.5e-11 (lap_16c) and 3.2e-10 (lap_33c), over 13 to 22 checked points.
Every shape/degree pair is under a tenth of RTRANS_RTOL_1GPU and is kept. The
check discriminates: test_gpu_poly.restated (A inside P) differs from restated32
on the same part of the rtrans trace by 1.3e-7 to 2.7e-6 relative on p10_lap_16c,
2.8e-7 to 1.4e-6 on p10_lap_33c and at least 1.3e-7 on every other shape and
degree, so a build that streamed fp64 values in the steps would miss the bar.
At degree 3 and 1e-10 r0 on p10_lap_33c both restatements take 26 iterations.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import test_gpu_pcg as tp
import test_gpu_poly as tpoly
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_mixed import assert_same, columns, dev, single_solves
from test_gpu_pcg import BASE, P2, csr_diagonal
from test_gpu_poly import LAP, coefficients, numpy_bound, problem

pytestmark = pytest.mark.gpu

EINVAL = -1
EIG_RATIO = 30.0
P10 = list(tpoly.P10) + ["p10_lap_33c"]
EXACT = BASE + P2 + LAP + ["p2_lap_16c"]
DEGREES = (1, 2, 3, 4)
# stored values that do not survive the round trip through float (NumPy, on the CPU): every one
INEXACT_VALUES = {"p10_16c": 97336, "p10_33c": 912673, "p10_12x10x16_7pt": 12496, "p10_band600": 1960,
                  "p10_dyadic_csr513": 3249}


@pytest.fixture(scope="module", autouse=True)
def _close_problems(hp):
    yield
    for cache in (tpoly._problems, tp._problems):
        for M, _, _ in cache.values():
            M.close()
        cache.clear()
    assert hp.poly32_live_workspaces() == 0
    assert hp.poly_live_workspaces() == 0
    assert hp.pcg_live_workspaces() == 0


def poly32_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, degree=2, lmin=None, lmax=None, minv=None, ld=None):
    """[(x, niters, normr, trace)] per column of a device solve; minv: None
    (Jacobi), a number (that value everywhere) or an array."""
    import torch
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    if minv is not None:
        minv = torch.from_numpy(np.full(n, 1.0) * np.float64(minv)).to(gpu)
    ierr, its, nrs, times = hp.HPCCG_poly32(M, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, minv=minv, device=True,
                                            max_iter=max_iter, tolerance=tol)
    assert ierr == 0 and times[0] > 0.0 and not times[1:].any()
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_poly32(c).copy()) for c in range(B.shape[0])]


def fl32(A):
    """A with every stored value through float32: the matrix the steps read."""
    return oracle.CSR(A.row_ptr, A.cols, A.vals.astype(np.float32).astype(np.float64), None, None, None)


# ---------------------------------------------------------------------------
# The recurrence of include/hpccg_hip_poly32.h restated: test_gpu_poly.restated
# with test_gpu_poly.apply_poly evaluated on A~ (At), and A everywhere else.
# ---------------------------------------------------------------------------
def restated32(A, At, b, minv, d, lmin, lmax, max_iter, tol=0.0, x0=None, dot=oracle.ddot):
    co = coefficients(lmin, lmax, d) if d else None
    with np.errstate(all="ignore"):
        x = np.zeros(A.nrow) if x0 is None else np.array(x0, np.float64)
        p = x + 0.0 * x
        Ap = oracle.sparsemv(A, p)
        r = b + (-1.0) * Ap
        z = tpoly.apply_poly(At, r, minv, d, co)
        rz = np.float64(dot(r, z))
        oldrz = rz
        hist = [np.float64(dot(r, r))]
        normr = np.sqrt(hist[0])
        trace = [normr]
        k = 1
        while k < max_iter and normr > tol:
            p = z + 0.0 * z if k == 1 else z + (rz / oldrz) * p
            normr = np.sqrt(hist[k - 1])
            trace.append(normr)
            Ap = oracle.sparsemv(A, p)
            alpha = rz / np.float64(dot(p, Ap))
            x = x + alpha * p
            r = r + (-alpha) * Ap
            z = tpoly.apply_poly(At, r, minv, d, co)
            oldrz = rz
            rz = np.float64(dot(r, z))
            hist.append(np.float64(dot(r, r)))
            k += 1
    return x, k - 1, float(normr), np.array(trace)


# ---------------------------------------------------------------------------
# 1. the image forms, the verdict, the count
# ---------------------------------------------------------------------------
def test_every_image_form_is_exercised(hp, gpu):
    """Widths 27, 7, per-slice (0) of SELL-512-A and the SELL-512 form, plain and scaled;
    exact and inexact images of each."""
    forms = {}
    for name in EXACT + ["p2_lap_33c"] + P10:
        M, A, _ = problem(hp, name)
        forms[name] = (M.get_option("has_a"), M.get_option("a_width") if M.get_option("has_a") else None)
        info = hp.poly32_info(M)
        inexact = int(np.count_nonzero(fl32(A).vals != A.vals))
        assert info["inexact_values"] == inexact, (name, info, inexact)
        assert info["exact"] == (1 if inexact == 0 else 0), (name, info)
        assert info["image_bytes"] >= 4 * A.vals.size and info["image_bytes"] % (4 * 512) == 0, (name, info)
        if name in P10:
            assert info["exact"] == 0 and inexact == A.vals.size, (name, inexact, A.vals.size)
            if name in INEXACT_VALUES:
                assert inexact == INEXACT_VALUES[name], (name, inexact)
        else:
            assert info["exact"] == 1, (name, info)
        assert M.poly32_workspace_bytes() >= info["image_bytes"]
    for pre in ("", "p2_", "p10_"):
        assert forms[pre + "33c"] == (1, 27) and forms[pre + "16c"] == (1, 27), forms
        assert forms[pre + "12x10x16_7pt"] == (1, 7), forms
        assert forms[pre + "band600"] == (1, 0), forms
        assert forms[pre + "dyadic_csr513"] == (0, None), forms
    assert forms["dyadic_csr3000"] == (0, None) and forms["p2_dyadic_csr3000"] == (0, None), forms
    for name in LAP + ["p2_lap_16c", "p2_lap_33c", "p10_lap_16c", "p10_lap_33c"]:
        assert forms[name] == (1, 27), (name, forms[name])


# ---------------------------------------------------------------------------
# 2. exact images: the fp64 polynomial, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EXACT)
def test_exact_image_is_the_fp64_polynomial(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    assert hp.poly32_info(M)["exact"] == 1
    B, X0 = columns(A.b, A.xexact, 5)
    # (columns are independent -- 6. -- so a reference of five columns serves every column count)
    forms = ((4, n), (3, n + 3), (2, n), (1, n))
    for degree in range(5):
        for mi, minv in enumerate((None, 1.0)):
            kw = dict(degree=degree, minv=minv)
            full = tpoly.poly_solve(hp, gpu, M, B, X0, 60, **kw)
            spectrum = M.last_spectrum_poly()
            # five columns (a chunk of four and a remainder) down to one; m = 1: five and one smaller form in turn
            for nrhs, ld in ((5, n),) + (forms if minv is None else (forms[degree % 4],)):
                got = poly32_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 60, ld=ld, **kw)
                assert_same(got, full[:nrhs])
            assert M.last_spectrum_poly32() == spectrum
            if (degree, mi) not in ((0, 1), (2, 0), (3, 1)):
                continue
            # a tolerance that column 0 meets part-way: just above the smallest residual of its first half
            tr0 = full[0][3]
            tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10) if len(tr0) > 4 else 0.0
            for max_iter, t in ((60, tol), (1, 0.0), (0, 0.0)):
                ref = tpoly.poly_solve(hp, gpu, M, B, X0, max_iter, t, **kw)
                if t > 0.0:
                    assert ref[0][1] < full[0][1], (ref[0][1], full[0][1])
                for nrhs, ld in ((5, n + 3), (2, n)):
                    got = poly32_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], max_iter, t, ld=ld, **kw)
                    assert_same(got, ref[:nrhs])
    assert hp.poly32_bound(M) == hp.poly_bound(M)


# ---------------------------------------------------------------------------
# 3. degree 0 is the pcg library, whatever the image
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P10)
def test_degree_0_is_the_pcg_solve_on_inexact_images(hp, gpu, shape):
    """... so the outer SpMM streams the fp64 values where the image is not the matrix."""
    M, A, _ = problem(hp, shape)
    n = A.nrow
    assert hp.poly32_info(M)["exact"] == 0
    B, X0 = columns(A.b, A.xexact, 5)
    for minv in (None, 1.0):
        for max_iter in (40, 1):
            ref = tp.pcg_solve(hp, gpu, M, B, X0, max_iter, minv=minv)
            for nrhs, ld in ((5, n), (3, n + 3), (2, n), (1, n)):
                got = poly32_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], max_iter, degree=0, minv=minv, ld=ld)
                assert_same(got, ref[:nrhs])


# ---------------------------------------------------------------------------
# 4. inexact images: the restatement with A~ inside P
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("shape", P10)
def test_inexact_image_follows_the_restatement(hp, gpu, shape, degree):
    M, A, _ = problem(hp, shape)
    At = fl32(A)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    # converged is normr <= 1e-14 r0
    x, niters, normr, tr = poly32_solve(hp, gpu, M, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    lmin, lmax = M.last_spectrum_poly32()
    # the interval is the fp64 image's
    assert lmax == hp.poly32_bound(M) == hp.poly_bound(M) and lmin == lmax / EIG_RATIO, (lmin, lmax)
    _, _, _, tr_ref = restated32(A, At, A.b, minv, degree, lmin, lmax, 200)
    assert tr_ref[0] == r0
    checked = check_trace(tr, tr_ref, RTRANS_RTOL_1GPU)
    print(f"{shape} degree {degree}: {checked} trace points checked, niters {niters}")
    assert checked >= 8, checked
    err = float(np.max(np.abs(x - A.xexact)))
    print(f"{shape} degree {degree}: normr/r0 {normr / r0:.3e} max |x - xexact| {err:.3e}")
    assert normr <= 1e-14 * r0 and niters < 199
    assert err <= 1e-9, err
    # niters under a tolerance between two residuals of the restatement: the
    # widest gap in the middle third of the checked part
    lo, hi = checked // 3, 2 * checked // 3
    k = lo + int(np.argmax(tr_ref[lo:hi] / tr_ref[lo + 1:hi + 1]))
    assert tr_ref[k] > 1.01 * tr_ref[k + 1], (k, tr_ref[k], tr_ref[k + 1])
    tol = float(np.sqrt(tr_ref[k] * tr_ref[k + 1]))
    _, it_ref, nr_ref, _ = restated32(A, At, A.b, minv, degree, lmin, lmax, 200, tol)
    _, it, nr, _ = poly32_solve(hp, gpu, M, B, X0, 200, tol, degree=degree)[0]
    assert it == it_ref and 0 < it < niters, (it, it_ref, niters)
    assert abs(nr - nr_ref) <= RTRANS_RTOL_1GPU * nr_ref, (nr, nr_ref)


# ---------------------------------------------------------------------------
# 5. it keeps what the polynomial is for
# ---------------------------------------------------------------------------
def test_degree_3_keeps_the_fp64_polynomials_iterations(hp, gpu):
    M, A, _ = problem(hp, "p10_lap_33c")
    n = A.nrow
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    tol = 1e-10 * r0
    _, it, nr, _ = poly32_solve(hp, gpu, M, B, X0, 200, tol, degree=3)[0]
    _, it64, nr64, _ = tpoly.poly_solve(hp, gpu, M, B, X0, 200, tol, degree=3)[0]
    jac = tp.pcg_solve(hp, gpu, M, B, X0, 200, tol)[0]
    print(f"p10_lap_33c: degree 3 {it} iterations (fp64 polynomial {it64}), Jacobi {jac[1]}; normr/r0 {nr / r0:.3e}")
    assert abs(it - it64) <= 1, (it, it64)
    assert nr <= tol and nr64 <= tol and jac[2] <= tol
    assert 2 * it < jac[1], (it, jac[1])


# ---------------------------------------------------------------------------
# 6. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2_33c", "p10_dyadic_csr513"], ids=["exact", "inexact"])
def test_columns_are_single_column_calls(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    rng = np.random.default_rng(9)
    # the same tolerance meets differently scaled residuals at different iterations
    B = np.stack([A.b, A.b * 2.0 ** -20, rng.uniform(-1.0, 1.0, n) * 2.0 ** 10, A.b * 2.0 ** -40, A.b])
    X0 = np.zeros((5, n))
    X0[4] = A.xexact  # (ends before its first iteration)
    tol = 1e-8 * float(np.linalg.norm(A.b))
    one = [poly32_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 150, tol)[0] for c in range(5)]
    stops = [o[1] for o in one]
    print(f"{shape}: stops {stops}")
    assert len(set(stops)) >= 3 and max(stops) < 149 and stops[4] == 0, stops
    for nrhs, ld in ((5, n + 5), (4, n), (3, n), (2, n)):
        got = poly32_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 150, tol, ld=ld)
        assert_same(got, one[:nrhs])
        for g in got[:4]:
            assert len(g[3]) == g[1] + 1 and g[2] == g[3][-1]
    # ... and when the iterations run out first
    for max_iter in (2, 7):
        got = poly32_solve(hp, gpu, M, B, X0, max_iter, tol)
        assert max(g[1] for g in got) == max_iter - 1 and got[4][1] == 0
        assert_same(got, [poly32_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], max_iter, tol)[0] for c in range(5)])


# ---------------------------------------------------------------------------
# 7. degenerate columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["16c", "p10_dyadic_csr513", "p10_12x10x16_7pt"])
def test_degenerate_columns_beside_ordinary_ones(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    At = fl32(A)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    rng = np.random.default_rng(41)
    nan_b = A.b.copy()
    nan_b[n // 2] = np.nan
    B = np.stack([A.b, A.b, nan_b, rng.uniform(-1.0, 1.0, n)])
    X0 = np.zeros((4, n))
    X0[1] = A.xexact  # a zero residual
    mi = 25
    alone = {c: poly32_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], mi)[0] for c in (0, 3)}
    poly32_solve(hp, gpu, M, np.tile(A.b, (4, 1)), np.zeros((4, n)), mi)  # four finite columns: the workspace at this call's size
    size = M.poly32_workspace_bytes()
    got = poly32_solve(hp, gpu, M, B, X0, mi)
    assert M.poly32_workspace_bytes() == size > 0
    lmin, lmax = M.last_spectrum_poly32()
    for c in (0, 3):
        assert_same(got[c:c + 1], [alone[c]])
        assert got[c][1] == mi - 1 and np.all(np.isfinite(got[c][0]))
    for c in (1, 2):
        x, it, nr, tr = restated32(A, At, B[c], minv, 2, lmin, lmax, mi, x0=X0[c])
        assert got[c][1] == it == 0, (c, got[c][1], it)
        assert math.isnan(got[c][2]) == math.isnan(nr) and (got[c][2] == 0.0) == (nr == 0.0), (c, got[c][2], nr)
        assert len(got[c][3]) == len(tr) == 1
        assert got[c][0].tobytes() == X0[c].tobytes()  # x untouched
    assert math.isnan(got[2][2]) and got[1][2] == 0.0
    # ... and nothing of them stays
    for c in (0, 3):
        assert_same(poly32_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], mi), [alone[c]])


# ---------------------------------------------------------------------------
# 8. values outside fp32 range
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [1e39, 1e-40], ids=["overflow", "underflow"])
def test_values_outside_fp32_range_are_refused(hp, gpu, bad):
    import torch
    if bad > 1.0:
        vals = [bad, -1.0, -1.0, 4.0, -1.0, -1.0, 4.0]
    else:
        vals = [4.0, bad, bad, 4.0, -1.0, -1.0, 4.0]
    M = hp.Matrix.from_csr([0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2], vals)
    try:
        Bd = torch.ones((2, 3), dtype=torch.float64, device=gpu)
        Xd = torch.full((2, 3), 0.5, dtype=torch.float64, device=gpu)
        for _ in range(2):  # (the verdict is kept)
            for degree in (2, 0):
                with pytest.raises(hp.HPCCGError, match="outside fp32 range"):
                    hp.HPCCG_poly32(M, Bd, Xd, degree=degree, max_iter=10, device=True)
            with pytest.raises(hp.HPCCGError, match="outside fp32 range"):
                hp.poly32_info(M)
        it = (C.c_int * 2)()
        nr = (C.c_double * 2)()
        assert hp.poly32_lib().hpccg_hip_poly32_solve_device(M.h, 2, Bd.data_ptr(), 3, Xd.data_ptr(), 3, None, 2, 0.0,
                                                             0.0, 10, 0.0, it, nr, None) == EINVAL
        assert torch.all(Xd == 0.5)
        # the fp64 polynomial takes the matrix as it is
        assert hp.HPCCG_poly(M, Bd, Xd.clone(), max_iter=5, device=True)[0] == 0
    finally:
        M.close()
    # ... and a good matrix afterwards
    G, A, _ = problem(hp, "16c")
    B, X0 = columns(A.b, A.xexact, 2)
    assert_same(poly32_solve(hp, gpu, G, B, X0, 10), tpoly.poly_solve(hp, gpu, G, B, X0, 10))


# ---------------------------------------------------------------------------
# 9. lifecycle and neighbours
# ---------------------------------------------------------------------------
def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.poly32_lib()
    M, A, _ = problem(hp, "p10_16c")
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = poly32_solve(hp, gpu, M, B, X0, 10)
    err = hp.lib().hpccg_hip_last_error

    def call(h, nrhs=2, ldb=n, ldx=n, minv=None, degree=2, lmin=0.0, lmax=0.0, max_iter=10):
        return L.hpccg_hip_poly32_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, minv, degree, lmin,
                                               lmax, max_iter, 0.0, it, nr, None)

    members = hp.group_generate(8, 8, 8, nranks=2)
    try:
        for m in members:
            assert call(m.h) == EINVAL
            assert b"group" in err()
            with pytest.raises(hp.HPCCGError):
                hp.poly32_bound(m)
            with pytest.raises(hp.HPCCGError):
                hp.poly32_info(m)
    finally:
        for m in members:
            m.close()
    mv = np.ones(n)
    mv[700] = float("nan")
    md = torch.from_numpy(mv).to(gpu)
    assert call(M.h, minv=md.data_ptr()) == EINVAL
    assert b"minv[700]" in err()
    bound = hp.poly32_bound(M)
    for lmin, lmax in ((2.0, 2.0), (float("nan"), 2.0), (bound, 0.0)):  # (the last: against the computed lmax)
        assert call(M.h, lmin=lmin, lmax=lmax) == EINVAL, (lmin, lmax)
        assert b"bounds" in err()
    for degree in (-1, 17):
        assert call(M.h, degree=degree) == EINVAL
    assert call(M.h, ldb=n - 1) == EINVAL
    assert b"leading dimension" in err()
    assert call(M.h, ldx=n - 1) == EINVAL
    assert call(M.h, max_iter=-1) == EINVAL
    assert call(M.h, nrhs=0) == EINVAL
    assert call(None) == EINVAL
    assert Xd.cpu().numpy().tobytes() == X0.tobytes()  # nothing was touched
    # ... and a good solve afterwards
    assert_same(poly32_solve(hp, gpu, M, B, X0, 10), ref)
    assert call(M.h, degree=16) == 0


@pytest.mark.parametrize("shape", ["p2_33c", "p10_dyadic_csr513", "p10_band600"])
def test_host_solve_and_explicit_jacobi_are_the_device_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 3)
    ref = poly32_solve(hp, gpu, M, B, X0, 25, degree=3)
    spectrum = M.last_spectrum_poly32()

    def host(**kw):
        X = X0.copy()
        ierr, its, nrs, times = hp.HPCCG_poly32(M, B, X, degree=3, max_iter=25, **kw)
        assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
        return [(X[c], int(its[c]), float(nrs[c]), M.last_trace_poly32(c).copy()) for c in range(3)]

    assert_same(host(), ref)
    minv = 1.0 / M.diagonal_pcg()
    assert_same(poly32_solve(hp, gpu, M, B, X0, 25, degree=3, minv=minv), ref)  # (its bound computed in the call)
    assert M.last_spectrum_poly32() == spectrum
    assert_same(host(minv=minv), ref)
    assert_same(host(lmin=spectrum[0], lmax=spectrum[1]), ref)
    # one column as a vector, updated in place
    x = X0[1].copy()
    hp.HPCCG_poly32(M, B[1].copy(), x, degree=3, max_iter=25)
    assert x.tobytes() == ref[1][0].tobytes()
    # a caller's m that is not Jacobi: the bound is NumPy's, and on the exact shape the solve is HPCCG_poly's
    m = np.random.default_rng(23).uniform(0.25, 4.0, A.nrow)
    got = poly32_solve(hp, gpu, M, B, X0, 25, degree=3, minv=m)
    rm, w = numpy_bound(A, m)
    assert abs(M.last_spectrum_poly32()[1] - rm) <= (w + 3) * 2.0 ** -52 * rm
    if hp.poly32_info(M)["exact"]:
        assert_same(got, tpoly.poly_solve(hp, gpu, M, B, X0, 25, degree=3, minv=m))


@pytest.mark.parametrize("shape", ["33c", "p10_dyadic_csr513"])
def test_other_solves_and_repeats_are_undisturbed(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 3)

    def others():
        single = single_solves(hp, gpu, M, B[:2], X0[:2], 40)
        Bd, Xd = dev(gpu, B), dev(gpu, X0)
        ierr, its, nrs, _ = hp.HPCCG_batch(M, Bd, Xd, max_iter=40, device=True)
        assert ierr == 0
        Bm, Xm = dev(gpu, B), dev(gpu, X0)
        ierr, itm, nrm, _ = hp.HPCCG_mixed(M, Bm, Xm, max_iter=40, device=True)
        assert ierr == 0
        return (single + tp.pcg_solve(hp, gpu, M, B, X0, 40) + tpoly.poly_solve(hp, gpu, M, B, X0, 40),
                (Xd.cpu().numpy().tobytes(), its.tobytes(), nrs.tobytes(), Xm.cpu().numpy().tobytes(), itm.tobytes(),
                 nrm.tobytes()))

    before = others()
    first = poly32_solve(hp, gpu, M, B, X0, 40)
    after = others()
    assert_same(after[0], before[0])
    assert after[1] == before[1]
    for _ in range(3):
        assert_same(poly32_solve(hp, gpu, M, B, X0, 40), first)
    assert M.poly32_workspace_bytes() > 0
    M.batch_release()
    M.mixed_release()


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.poly32_live_workspaces()
    prob = hp.generate_matrix(8, 8, 8)
    M = hp.Matrix.from_hpc(prob)
    M2 = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 2)
        first = poly32_solve(hp, gpu, M, B, X0, 10)
        poly32_solve(hp, gpu, M2, B, X0, 10)
        assert hp.poly32_live_workspaces() == base + 2
        image = hp.poly32_info(M2)["image_bytes"]
        assert image == 4 * 27 * 512  # one slice of 27 slots
        assert M2.poly32_workspace_bytes() > image + 2 * 8 * 512
        M2.poly32_release()
        assert hp.poly32_live_workspaces() == base + 1 and M2.poly32_workspace_bytes() == 0
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            M2.last_spectrum_poly32()
        assert_same(poly32_solve(hp, gpu, M2, B, X0, 10), first)  # rebuilt on demand, the image and the caches too
        small = M2.poly32_workspace_bytes()
        poly32_solve(hp, gpu, M2, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the image and the caches stay
        assert M2.poly32_workspace_bytes() > small
        assert_same(poly32_solve(hp, gpu, M2, B, X0, 10), first)
        M2.poly32_release()
        M2.poly32_release()  # (idempotent)
        assert hp.poly32_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()  # (the destroy hook frees M's workspace)
        M2.close()
        prob.close()
    assert hp.poly32_live_workspaces() == base
