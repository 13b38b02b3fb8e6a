"""Chebyshev polynomial preconditioned CG (include/hpccg_hip_poly.h,
lib/libhpccg_hip_poly.so): per column the preconditioned recurrence of
hpccg_hip_pcg.h with z = P(r), P the Chebyshev iteration of `degree` steps for
diag(m) A on [lmin, lmax]; loop test, niters, normr and trace on the 2-norm of r.

  1. degree 0 is the pcg library bit for bit (x, niters, normr, trace);
  2. column c of a multi-column call is bitwise the single-column call;
  3. Jacobi-Chebyshev on S A S with S b, S powers of two, explicit bounds:
     s_i x'_i is bitwise the x on A with b (every quantity scales exactly);
  4. the symmetric Gershgorin bound against NumPy's, and its exact scaling;
  5. on matrices scaled by s_i = 10^u_i: the NumPy restatement below (trace,
     niters under a tolerance, x against xexact), degrees 1 to 4;
  6. it does what it is for: a third of Jacobi's iterations on a weakly
     diagonally dominant matrix;
  7. degenerate columns beside ordinary ones;
  8. refusals and the workspace's life.

Shapes: those of test_gpu_pcg.py (its BASE, "p2_" and "p10_" forms), and
"lap_16c", "lap_33c": the generated 27-point pattern with every diagonal entry
26.0 (weakly diagonally dominant), built through Matrix.from_csr.

5.: the restatement run with two dot orders (a sequential sum and numpy's
blocked one) agrees with itself on the checked part of the rtrans trace, worst
over degrees 1 to 4, to 8.3e-11 (16c), 1.4e-12 (33c), 3.3e-14 (7pt), 7.2e-13
(band600), 2.9e-14 (csr513) and 1.0e-10 (lap_16c): every shape/degree pair is
within a tenth of RTRANS_RTOL_1GPU and is kept. There the restatement's own x is
within 1.9e-11 of xexact at normr <= 1e-14 r0.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import test_gpu_pcg as tp
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_mixed import STENCILS, assert_same, columns, dev, finish, single_solves
from test_gpu_pcg import BASE, P2, csr_diagonal, rows_of, scale_of, scaled

pytestmark = pytest.mark.gpu

EINVAL = -1
EIG_RATIO = 30.0
LAP = ["lap_16c", "lap_33c"]
P10 = list(tp.P10) + ["p10_lap_16c"]
DEGREES = (1, 2, 3, 4)


# ---------------------------------------------------------------------------
# problems: name -> (Matrix, oracle.CSR with b = A 1, scale s or None);
# test_gpu_pcg.py's own, and the "lap_" forms beside them
# ---------------------------------------------------------------------------
def lap_csr(name):
    nx, ny, nz, s7 = STENCILS[name[4:]]
    G = oracle.generate(nx, ny, nz, use_7pt=s7)
    vals = G.vals.copy()
    vals[rows_of(G) == G.cols] = 26.0
    return finish(G.row_ptr, G.cols, vals)


_problems = {}


def problem(hp, name):
    kind, _, rest = name.partition("_")
    if not (name in LAP or (kind in ("p2", "p10") and rest in LAP)):
        return tp.problem(hp, name)
    if name not in _problems:
        if name in LAP:
            A, s = lap_csr(name), None
        else:
            A0 = lap_csr(rest)
            s = scale_of(kind, A0.nrow)
            A = scaled(A0, s)
        _problems[name] = (hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals), A, s)
    return _problems[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems(hp):
    yield
    for cache in (_problems, tp._problems):
        for M, _, _ in cache.values():
            M.close()
        cache.clear()
    assert hp.poly_live_workspaces() == 0
    assert hp.pcg_live_workspaces() == 0


def poly_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, degree=2, lmin=None, lmax=None, minv=None, ld=None):
    """[(x, niters, normr, trace)] per column of a device solve; minv: None
    (Jacobi), a number (that value everywhere) or an array."""
    import torch
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    if minv is not None:
        minv = torch.from_numpy(np.full(n, 1.0) * np.float64(minv)).to(gpu)
    ierr, its, nrs, times = hp.HPCCG_poly(M, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, minv=minv, device=True,
                                          max_iter=max_iter, tolerance=tol)
    assert ierr == 0 and times[0] > 0.0 and not times[1:].any()
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_poly(c).copy()) for c in range(B.shape[0])]


# ---------------------------------------------------------------------------
# The recurrence of include/hpccg_hip_poly.h restated: test_gpu_pcg.restated
# with the Chebyshev application, on oracle.sparsemv and a fixed-order
# (sequential) float64 dot.
# ---------------------------------------------------------------------------
def coefficients(lmin, lmax, d):
    lmin, lmax = np.float64(lmin), np.float64(lmax)
    theta = np.float64(0.5) * (lmax + lmin)
    delta = np.float64(0.5) * (lmax - lmin)
    sigma = theta / delta
    rho = np.float64(1.0) / sigma
    c0 = np.float64(1.0) / theta
    a, b = [], []
    for _ in range(d):
        rho_new = np.float64(1.0) / (np.float64(2.0) * sigma - rho)
        a.append(rho_new * rho)
        b.append(np.float64(2.0) * rho_new / delta)
        rho = rho_new
    return c0, a, b


def apply_poly(A, r, minv, d, co):
    if d == 0:
        return minv * r
    c0, a, b = co
    t = minv * r
    dd = c0 * t
    z = dd
    for j in range(d):
        w = oracle.sparsemv(A, z)
        t = minv * (r - w)
        dd = a[j] * dd + b[j] * t
        z = z + dd
    return z


def restated(A, b, minv, d, lmin, lmax, max_iter, tol=0.0, x0=None, dot=oracle.ddot):
    co = coefficients(lmin, lmax, d) if d else None
    with np.errstate(all="ignore"):
        x = np.zeros(A.nrow) if x0 is None else np.array(x0, np.float64)
        p = x + 0.0 * x
        Ap = oracle.sparsemv(A, p)
        r = b + (-1.0) * Ap
        z = apply_poly(A, r, minv, d, co)
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
            z = apply_poly(A, r, minv, d, co)
            oldrz = rz
            rz = np.float64(dot(r, z))
            hist.append(np.float64(dot(r, r)))
            k += 1
    return x, k - 1, float(normr), np.array(trace)


def numpy_bound(A, minv):
    """max_i q_i sum_j |a_ij| q_j with q = sqrt(minv), and the widest row."""
    q = np.sqrt(minv)
    rows = rows_of(A)
    g = np.zeros(A.nrow)
    np.add.at(g, rows, np.abs(A.vals) * q[A.cols.astype(np.int64)])
    return float(np.max(q * g)), int(np.max(np.diff(A.row_ptr)))


def test_every_image_form_is_exercised(hp, gpu):
    """Widths 27, 7, per-slice (0) of SELL-512-A and the SELL-512 form, plain and scaled."""
    forms = {}
    for name in BASE + P2 + P10 + LAP + ["p2_lap_16c", "p2_lap_33c", "p10_lap_33c"]:
        M = problem(hp, name)[0]
        forms[name] = (M.get_option("has_a"), M.get_option("a_width") if M.get_option("has_a") else None)
    for pre in ("", "p2_", "p10_"):
        assert forms[pre + "33c"] == (1, 27) and forms[pre + "16c"] == (1, 27), forms
        assert forms[pre + "12x10x16_7pt"] == (1, 7), forms
        assert forms[pre + "band600"] == (1, 0), forms
        assert forms[pre + "dyadic_csr513"] == (0, None), forms
    assert forms["dyadic_csr3000"] == (0, None) and forms["p2_dyadic_csr3000"] == (0, None), forms
    for name in LAP + ["p2_lap_16c", "p2_lap_33c", "p10_lap_16c", "p10_lap_33c"]:
        assert forms[name] == (1, 27), (name, forms[name])


# ---------------------------------------------------------------------------
# 1. degree 0 is the pcg library
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2)
def test_degree_0_is_the_pcg_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 5)
    for minv in (None, 1.0):
        full = tp.pcg_solve(hp, gpu, M, B, X0, 60, minv=minv)
        # a tolerance that column 0 meets part-way: just above the smallest residual of its first half
        tr0 = full[0][3]
        tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10) if len(tr0) > 4 else 0.0
        part = tp.pcg_solve(hp, gpu, M, B, X0, 60, tol, minv=minv)
        if n > 1:
            assert part[0][1] < full[0][1], (part[0][1], full[0][1])
        for max_iter, t, ref in ((60, 0.0, full), (60, tol, part), (1, 0.0, None), (0, 0.0, None)):
            if ref is None:
                ref = tp.pcg_solve(hp, gpu, M, B, X0, max_iter, t, minv=minv)
            for nrhs, ld in ((5, n), (4, n), (3, n + 3), (2, n), (1, n)):
                got = poly_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], max_iter, t, degree=0, minv=minv, ld=ld)
                assert_same(got, ref[:nrhs])
    # ... and so, with m = 1, the single solve
    assert_same(poly_solve(hp, gpu, M, B[:2], X0[:2], 60, degree=0, minv=1.0), single_solves(hp, gpu, M, B[:2], X0[:2], 60))


# ---------------------------------------------------------------------------
# 2. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2_33c", "p10_dyadic_csr513", "12x10x16_7pt"])
def test_columns_are_single_column_calls(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    rng = np.random.default_rng(9)
    # the same tolerance meets differently scaled residuals at different iterations
    B = np.stack([A.b, A.b * 2.0 ** -20, rng.uniform(-1.0, 1.0, n) * 2.0 ** 10, A.b * 2.0 ** -40, A.b])
    X0 = np.zeros((5, n))
    X0[4] = A.xexact  # (ends before its first iteration)
    tol = 1e-8 * float(np.linalg.norm(A.b))
    one = [poly_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 150, tol)[0] for c in range(5)]
    stops = [o[1] for o in one]
    print(f"{shape}: stops {stops}")
    assert len(set(stops)) >= 3 and max(stops) < 149 and stops[4] == 0, stops
    for nrhs, ld in ((5, n + 5), (4, n), (3, n), (2, n)):
        got = poly_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 150, tol, ld=ld)
        assert_same(got, one[:nrhs])
        for g in got[:4]:
            assert len(g[3]) == g[1] + 1 and g[2] == g[3][-1]
    # ... and when the iterations run out first
    for max_iter in (2, 7):
        got = poly_solve(hp, gpu, M, B, X0, max_iter, tol)
        assert max(g[1] for g in got) == max_iter - 1 and got[4][1] == 0
        assert_same(got, [poly_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], max_iter, tol)[0] for c in range(5)])


# ---------------------------------------------------------------------------
# 3. exact scaling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["33c", "16c", "dyadic_csr3000", "dyadic_csr513"])
def test_chebyshev_commutes_with_a_power_of_two_scaling(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    Ms, As, s = problem(hp, "p2_" + shape)
    n = A.nrow
    rng = np.random.default_rng(3)
    B = np.stack([A.b, rng.uniform(-1.0, 1.0, n), A.b * 2.0 ** -7, rng.uniform(-1.0, 1.0, n)])
    X0 = np.zeros((4, n))
    # (2.0 bounds the Jacobi-scaled spectrum of these diagonally dominant matrices)
    kw = dict(degree=3, lmin=2.0 / EIG_RATIO, lmax=2.0)
    for nrhs in (4, 1, 2):
        got = poly_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 12, **kw)
        gots = poly_solve(hp, gpu, Ms, B[:nrhs] * s, X0[:nrhs], 12, **kw)
        assert M.last_spectrum_poly() == Ms.last_spectrum_poly() == (2.0 / EIG_RATIO, 2.0)
        for c in range(nrhs):
            assert got[c][1] == gots[c][1] == 11
            assert (gots[c][0] * s).tobytes() == got[c][0].tobytes(), (nrhs, c, float(np.max(np.abs(gots[c][0] * s - got[c][0]))))
            assert np.all(np.isfinite(got[c][0])) and got[c][0].any()


# ---------------------------------------------------------------------------
# 4. the bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + LAP)
def test_the_bound_is_numpys_and_scales_exactly(hp, gpu, shape):
    import torch
    M, A, _ = problem(hp, shape)
    jac = 1.0 / csr_diagonal(A)
    got = hp.poly_bound(M)
    ref, w = numpy_bound(A, jac)
    # one rounding per added term, the two products and the sqrt
    margin = (w + 3) * 2.0 ** -52
    print(f"{shape}: bound {got!r} numpy {ref!r} widest row {w}")
    assert abs(got - ref) <= margin * ref, (got, ref)
    assert hp.poly_bound(M) == got  # (cached)
    assert hp.poly_bound(M, torch.from_numpy(jac).to(gpu)) == got  # a caller's m: the same kernels
    for kind in ("p2", "p10"):
        Ms, As, s = problem(hp, f"{kind}_{shape}")
        gs = hp.poly_bound(Ms)
        if kind == "p2":  # q_i / s_i, |a_ij| s_i s_j: exact with a correctly rounded sqrt
            assert np.float64(gs).tobytes() == np.float64(got).tobytes(), (gs, got)
        rs, ws = numpy_bound(As, 1.0 / csr_diagonal(As))
        assert ws == w and abs(gs - rs) <= margin * rs, (gs, rs)
    # a caller's m
    m = np.random.default_rng(23).uniform(0.25, 4.0, A.nrow)
    rm, _ = numpy_bound(A, m)
    gm = hp.poly_bound(M, torch.from_numpy(m).to(gpu))
    assert abs(gm - rm) <= margin * rm, (gm, rm)
    exact = {"1x1x1": 1.0, "33c": 53.0 / 27.0, "lap_33c": 2.0}.get(shape)
    if exact is not None:
        assert abs(got - exact) <= margin * exact, (got, exact)


# ---------------------------------------------------------------------------
# 5. the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("shape", P10)
def test_chebyshev_follows_the_restatement(hp, gpu, shape, degree):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    # converged is normr <= 1e-14 r0
    x, niters, normr, tr = poly_solve(hp, gpu, M, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    lmin, lmax = M.last_spectrum_poly()
    assert lmax == hp.poly_bound(M) and lmin == lmax / EIG_RATIO, (lmin, lmax)
    _, _, _, tr_ref = restated(A, A.b, minv, degree, lmin, lmax, 200)
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
    _, it_ref, nr_ref, _ = restated(A, A.b, minv, degree, lmin, lmax, 200, tol)
    _, it, nr, _ = poly_solve(hp, gpu, M, B, X0, 200, tol, degree=degree)[0]
    assert it == it_ref and 0 < it < niters, (it, it_ref, niters)
    assert abs(nr - nr_ref) <= RTRANS_RTOL_1GPU * nr_ref, (nr, nr_ref)


# ---------------------------------------------------------------------------
# 6. it does what it is for
# ---------------------------------------------------------------------------
def test_degree_3_halves_jacobis_iterations(hp, gpu):
    M, A, _ = problem(hp, "p10_lap_33c")
    n = A.nrow
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    tol = 1e-10 * r0
    x, it, nr, _ = poly_solve(hp, gpu, M, B, X0, 200, tol, degree=3)[0]
    lmin, lmax = M.last_spectrum_poly()
    _, it_ref, _, _ = restated(A, A.b, 1.0 / csr_diagonal(A), 3, lmin, lmax, 200, tol)
    jac = tp.pcg_solve(hp, gpu, M, B, X0, 200, tol)[0]
    print(f"p10_lap_33c: degree 3 {it} iterations (restatement {it_ref}), Jacobi {jac[1]}; normr/r0 {nr / r0:.3e}")
    assert abs(it - it_ref) <= 2, (it, it_ref)
    assert nr <= tol and jac[2] <= tol
    assert 2 * it <= jac[1], (it, jac[1])


# ---------------------------------------------------------------------------
# 7. degenerate columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["16c", "p2_dyadic_csr513", "12x10x16_7pt"])
def test_degenerate_columns_beside_ordinary_ones(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    rng = np.random.default_rng(41)
    nan_b = A.b.copy()
    nan_b[n // 2] = np.nan
    B = np.stack([A.b, A.b, nan_b, rng.uniform(-1.0, 1.0, n)])
    X0 = np.zeros((4, n))
    X0[1] = A.xexact  # a zero residual
    mi = 25
    alone = {c: poly_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], mi)[0] for c in (0, 3)}
    poly_solve(hp, gpu, M, np.tile(A.b, (4, 1)), np.zeros((4, n)), mi)  # four finite columns: the workspace at this call's size
    size = M.poly_workspace_bytes()
    got = poly_solve(hp, gpu, M, B, X0, mi)
    assert M.poly_workspace_bytes() == size > 0
    lmin, lmax = M.last_spectrum_poly()
    for c in (0, 3):
        assert_same(got[c:c + 1], [alone[c]])
        assert got[c][1] == mi - 1 and np.all(np.isfinite(got[c][0]))
    for c in (1, 2):
        x, it, nr, tr = restated(A, B[c], minv, 2, lmin, lmax, mi, x0=X0[c])
        assert got[c][1] == it == 0, (c, got[c][1], it)
        assert math.isnan(got[c][2]) == math.isnan(nr) and (got[c][2] == 0.0) == (nr == 0.0), (c, got[c][2], nr)
        assert len(got[c][3]) == len(tr) == 1
        assert got[c][0].tobytes() == X0[c].tobytes()  # x untouched
    assert math.isnan(got[2][2]) and got[1][2] == 0.0
    # ... and nothing of them stays
    for c in (0, 3):
        assert_same(poly_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], mi), [alone[c]])


# ---------------------------------------------------------------------------
# 8. refusals, the workspace
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("base,edit", [("band600", tp._zero_diag), ("dyadic_csr513", tp._negative_diag)],
                         ids=["zero_a", "negative_sell"])
def test_a_bad_diagonal_is_refused(hp, gpu, base, edit):
    import torch
    A = tp.base_csr(base)
    n = A.nrow
    rp, cols, vals, row = tp._edited(A, edit)
    M = hp.Matrix.from_csr(rp, cols, vals)
    try:
        Bd = torch.ones((2, n), dtype=torch.float64, device=gpu)
        Xd = torch.full((2, n), 0.5, dtype=torch.float64, device=gpu)
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match=rf"row {row} "):
                hp.HPCCG_poly(M, Bd, Xd, max_iter=10, device=True)
        with pytest.raises(hp.HPCCGError, match=rf"row {row} "):
            hp.poly_bound(M)
        assert torch.all(Xd == 0.5)
        # a caller's m is taken on the same matrix
        assert hp.HPCCG_poly(M, Bd, Xd.clone(), max_iter=3, minv=torch.ones(n, dtype=torch.float64, device=gpu),
                             device=True)[0] == 0
    finally:
        M.close()


def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.poly_lib()
    M, A, _ = problem(hp, "16c")
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = poly_solve(hp, gpu, M, B, X0, 10)
    err = hp.lib().hpccg_hip_last_error

    def call(h, nrhs=2, ldb=n, ldx=n, minv=None, degree=2, lmin=0.0, lmax=0.0, max_iter=10):
        return L.hpccg_hip_poly_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, minv, degree, lmin, lmax,
                                             max_iter, 0.0, it, nr, None)

    members = hp.group_generate(8, 8, 8, nranks=2)
    try:
        for m in members:
            assert call(m.h) == EINVAL
            assert b"group" in err()
            with pytest.raises(hp.HPCCGError):
                hp.poly_bound(m)
    finally:
        for m in members:
            m.close()
    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        mv = np.ones(n)
        mv[700] = bad
        mv[3000] = bad
        md = torch.from_numpy(mv).to(gpu)
        assert call(M.h, minv=md.data_ptr()) == EINVAL
        assert b"minv[700]" in err()
        with pytest.raises(hp.HPCCGError, match=r"minv\[700\]"):
            hp.HPCCG_poly(M, B.copy(), X0.copy(), max_iter=10, minv=mv)
        with pytest.raises(hp.HPCCGError, match=r"minv\[700\]"):
            hp.poly_bound(M, md)
    bound = hp.poly_bound(M)
    for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (-1.0, 2.0), (float("nan"), 2.0), (0.5, float("inf")),
                       (bound, 0.0), (2.0 * bound, 0.0)):  # (the last two: against the computed lmax)
        assert call(M.h, lmin=lmin, lmax=lmax) == EINVAL, (lmin, lmax)
        assert b"bounds" in err()
    for degree in (-1, 17):
        assert call(M.h, degree=degree) == EINVAL
        assert b"degree" in err()
    assert call(M.h, ldb=n - 1) == EINVAL
    assert b"leading dimension" in err()
    assert call(M.h, ldx=n - 1) == EINVAL
    assert call(M.h, max_iter=-1) == EINVAL
    assert call(M.h, nrhs=0) == EINVAL
    assert call(None) == EINVAL
    assert Xd.cpu().numpy().tobytes() == X0.tobytes()  # nothing was touched
    # ... and a good solve afterwards
    assert_same(poly_solve(hp, gpu, M, B, X0, 10), ref)
    assert call(M.h, degree=16) == 0


@pytest.mark.parametrize("shape", ["p2_33c", "p10_dyadic_csr513", "band600"])
def test_host_solve_and_explicit_jacobi_are_the_device_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 3)
    ref = poly_solve(hp, gpu, M, B, X0, 25, degree=3)
    spectrum = M.last_spectrum_poly()

    def host(**kw):
        X = X0.copy()
        ierr, its, nrs, times = hp.HPCCG_poly(M, B, X, degree=3, max_iter=25, **kw)
        assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
        return [(X[c], int(its[c]), float(nrs[c]), M.last_trace_poly(c).copy()) for c in range(3)]

    assert_same(host(), ref)
    minv = 1.0 / M.diagonal_pcg()
    assert_same(poly_solve(hp, gpu, M, B, X0, 25, degree=3, minv=minv), ref)  # (its bound computed in the call)
    assert M.last_spectrum_poly() == spectrum
    assert_same(host(minv=minv), ref)
    assert_same(host(minv=minv, lmax=spectrum[1]), ref)
    assert_same(host(lmin=spectrum[0], lmax=spectrum[1]), ref)
    # one column as a vector, updated in place
    x = X0[1].copy()
    hp.HPCCG_poly(M, B[1].copy(), x, degree=3, max_iter=25)
    assert x.tobytes() == ref[1][0].tobytes()


@pytest.mark.parametrize("shape", ["33c", "p2_dyadic_csr3000"])
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
        return single + tp.pcg_solve(hp, gpu, M, B, X0, 40), (Xd.cpu().numpy().tobytes(), its.tobytes(), nrs.tobytes(),
                                                              Xm.cpu().numpy().tobytes(), itm.tobytes(), nrm.tobytes())

    before = others()
    first = poly_solve(hp, gpu, M, B, X0, 40)
    after = others()
    assert_same(after[0], before[0])
    assert after[1] == before[1]
    for _ in range(3):
        assert_same(poly_solve(hp, gpu, M, B, X0, 40), first)
    assert M.poly_workspace_bytes() > 0
    M.batch_release()
    M.mixed_release()


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.poly_live_workspaces()
    prob = hp.generate_matrix(8, 8, 8)
    M = hp.Matrix.from_hpc(prob)
    M2 = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 2)
        first = poly_solve(hp, gpu, M, B, X0, 10)
        poly_solve(hp, gpu, M2, B, X0, 10)
        assert hp.poly_live_workspaces() == base + 2
        assert M2.poly_workspace_bytes() > 2 * 8 * 512
        M2.poly_release()
        assert hp.poly_live_workspaces() == base + 1 and M2.poly_workspace_bytes() == 0
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            M2.last_spectrum_poly()
        assert_same(poly_solve(hp, gpu, M2, B, X0, 10), first)  # rebuilt on demand, the caches too
        small = M2.poly_workspace_bytes()
        poly_solve(hp, gpu, M2, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the caches stay
        assert M2.poly_workspace_bytes() > small
        assert_same(poly_solve(hp, gpu, M2, B, X0, 10), first)
        M2.poly_release()
        M2.poly_release()  # (idempotent)
        assert hp.poly_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()
        M2.close()
        prob.close()
    assert hp.poly_live_workspaces() == base
