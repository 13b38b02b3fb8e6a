"""Single-reduction CG with the Chebyshev polynomial preconditioner
(include/hpccg_hip_srpoly.h, lib/libhpccg_hip_srpoly.so): HPCCG_srcg's
recurrence with u = P(r) of HPCCG_poly, restated below in NumPy
(restated_srpoly, importable without a GPU: tests/test_srpoly_cpu.py pins it
against test_gpu_poly.restated and test_gpu_srcg.restated_sr).

  1. degree 0 is HPCCG_srcg bit for bit (x, niters, normr, trace);
  2. degrees 1 to 4: max_iter <= 2 is HPCCG_poly bit for bit with the same
     interval, the trace still at max_iter 3;
  3. column c of a call of 5, 4, 3 (padded ld), 2 and 1 columns is bitwise its
     one-column call, at tolerance 0 and at one that freezes columns part-way;
  4. Jacobi-Chebyshev on S A S with S b, S powers of two, explicit bounds;
  5. on matrices scaled by s_i = 10^u_i, degrees 1 to 4: the restatement (trace,
     niters under a tolerance), HPCCG_poly's niters, x against xexact;
  6. the bound is poly_bound's; 7. host = device = explicit Jacobi m;
  8. degenerate columns; 9. refusals; 10. both non-temporal arms; 11. other
     solvers and repeats undisturbed; 12. the workspace's life.

Shapes and helpers: those of test_gpu_poly.py, test_gpu_pcg.py and
test_gpu_mixed.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import columns_cases as cc
import oracle
import test_gpu_mixed as tm
import test_gpu_nt as tn
import test_gpu_pcg as tp
import test_gpu_poly as tpo
import test_gpu_srcg as ts
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_mixed import assert_same, columns, dev, single_solves
from test_gpu_pcg import BASE, P2, csr_diagonal
from test_gpu_poly import DEGREES, EIG_RATIO, LAP, P10, apply_poly, coefficients, problem
from test_gpu_srcg import seq_dot

pytestmark = pytest.mark.gpu

EINVAL = -1


# ---------------------------------------------------------------------------
# The recurrence of include/hpccg_hip_srpoly.h restated: test_gpu_srcg.restated_sr
# with u = test_gpu_poly.apply_poly(r), on oracle.sparsemv and a fixed-order
# (sequential) float64 dot by default.
# ---------------------------------------------------------------------------
def restated_srpoly(A, b, minv, d, lmin, lmax, max_iter, tol=0.0, x0=None, dot=seq_dot):
    co = coefficients(lmin, lmax, d) if d else None
    with np.errstate(all="ignore"):
        x = np.zeros(A.nrow) if x0 is None else np.array(x0, np.float64)
        t = x + 0.0 * x
        r = b + (-1.0) * oracle.sparsemv(A, t)
        u = apply_poly(A, r, minv, d, co)
        w = oracle.sparsemv(A, u)
        gamma, delta = dot(r, u), dot(u, w)
        hist = [dot(r, r)]
        beta, alpha = np.float64(0.0), gamma / delta
        normr = np.sqrt(hist[0])
        trace = [normr]
        p = s = None
        k = 1
        while k < max_iter and normr > tol:
            normr = np.sqrt(hist[k - 1])
            trace.append(normr)
            p = u + beta * (u if k == 1 else p)
            s = w + beta * (w if k == 1 else s)
            x = x + alpha * p
            r = r + (-alpha) * s
            u = apply_poly(A, r, minv, d, co)
            w = oracle.sparsemv(A, u)
            gold, aold = gamma, alpha
            gamma, delta = dot(r, u), dot(u, w)
            hist.append(dot(r, r))
            beta = gamma / gold
            alpha = gamma / (delta - (beta * gamma) / aold)
            k += 1
    return x, k - 1, float(normr), np.array(trace)


@pytest.fixture(scope="module", autouse=True)
def _close_problems(hp):
    yield
    for cache in (tpo._problems, tm._problems, tp._problems):
        for M, _, _ in cache.values():
            M.close()
        cache.clear()
    assert hp.srpoly_live_workspaces() == 0
    assert hp.poly_live_workspaces() == 0
    assert hp.srcg_live_workspaces() == 0


def srpoly_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, degree=2, lmin=None, lmax=None, minv=None, ld=None):
    """[(x, niters, normr, trace)] per column of a device solve; minv: None
    (Jacobi), a number (that value everywhere) or an array."""
    import torch
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    if minv is not None:
        minv = torch.from_numpy(np.full(n, 1.0) * np.float64(minv)).to(gpu)
    ierr, its, nrs, times = hp.HPCCG_srpoly(M, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, minv=minv, device=True,
                                            max_iter=max_iter, tolerance=tol)
    assert ierr == 0 and times[0] > 0.0 and not times[1:].any()
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_srpoly(c).copy()) for c in range(B.shape[0])]


def part_way(full):
    """A tolerance that column 0 meets part-way: just above the smallest residual of its first half."""
    tr0 = full[0][3]
    half = tr0[:len(tr0) // 2 + 1]
    half = half[np.isfinite(half) & (half > 0.0)]
    return float(np.min(half)) * (1.0 + 2.0 ** -10) if len(tr0) > 4 and len(half) else 0.0


# ---------------------------------------------------------------------------
# 1. degree 0 is the srcg library
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2)
def test_degree_0_is_the_srcg_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 5)
    for minv in (None, 1.0):
        full = ts.srcg_solve(hp, gpu, M, B, X0, 60, minv=minv)
        tol = part_way(full)
        for max_iter, t in ((60, 0.0), (60, tol), (1, 0.0), (0, 0.0)):
            ref = full if (max_iter, t) == (60, 0.0) else ts.srcg_solve(hp, gpu, M, B, X0, max_iter, t, minv=minv)
            assert_same(srpoly_solve(hp, gpu, M, B, X0, max_iter, t, degree=0, minv=minv), ref)
    # the bounds are kept, not used
    srpoly_solve(hp, gpu, M, B[:1], X0[:1], 3, degree=0, lmax=3.0)
    assert M.last_spectrum_srpoly() == (3.0 / EIG_RATIO, 3.0)


# ---------------------------------------------------------------------------
# 2. the first iteration
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2 + LAP)
def test_the_first_iteration_is_polys(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 5)
    assert X0[1].any()  # a nonzero x0 among them
    for degree in DEGREES:
        for minv in (None, 1.0):
            for max_iter in (0, 1, 2):
                ref = tpo.poly_solve(hp, gpu, M, B, X0, max_iter, degree=degree, minv=minv)
                assert_same(srpoly_solve(hp, gpu, M, B, X0, max_iter, degree=degree, minv=minv), ref)
                assert M.last_spectrum_srpoly() == M.last_spectrum_poly()
                assert max(r[1] for r in ref) == max(max_iter, 1) - 1
            ref = tpo.poly_solve(hp, gpu, M, B, X0, 3, degree=degree, minv=minv)
            got = srpoly_solve(hp, gpu, M, B, X0, 3, degree=degree, minv=minv)
            for c in range(5):
                assert got[c][1] == ref[c][1] and got[c][3].tobytes() == ref[c][3].tobytes(), (degree, minv, c)


# ---------------------------------------------------------------------------
# 3. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (1, 2))
@pytest.mark.parametrize("shape", BASE + P2)
def test_columns_are_single_column_calls(hp, gpu, shape, degree):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 5)

    def ones(tol):
        return [srpoly_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 30, tol, degree=degree)[0] for c in range(5)]

    full = ones(0.0)
    tol = part_way(full)
    part = ones(tol)
    print(f"{shape} degree {degree}: stops {[r[1] for r in part]} under the tolerance, {[r[1] for r in full]} without")
    if n > 1:
        assert part[0][1] < full[0][1], (part[0][1], full[0][1])
    assert full[2][1] == 0  # (x0 = xexact: frozen since the prologue)
    for t, ref in ((0.0, full), (tol, part)):
        for nrhs, ld in ((5, n), (4, n), (3, n + 3), (2, n), (1, n)):
            assert_same(srpoly_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 30, t, degree=degree, ld=ld), ref[:nrhs])


# ---------------------------------------------------------------------------
# 4. exact scaling
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
        got = srpoly_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 12, **kw)
        gots = srpoly_solve(hp, gpu, Ms, B[:nrhs] * s, X0[:nrhs], 12, **kw)
        assert M.last_spectrum_srpoly() == Ms.last_spectrum_srpoly() == (2.0 / EIG_RATIO, 2.0)
        for c in range(nrhs):
            assert got[c][1] == gots[c][1] == 11
            assert (gots[c][0] * s).tobytes() == got[c][0].tobytes(), (nrhs, c, float(np.max(np.abs(gots[c][0] * s - got[c][0]))))
            assert np.all(np.isfinite(got[c][0])) and got[c][0].any()


# ---------------------------------------------------------------------------
# 5. the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("shape", P10)
def test_srpoly_follows_the_restatement(hp, gpu, shape, degree):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    # converged is normr <= 1e-14 r0
    x, niters, normr, tr = srpoly_solve(hp, gpu, M, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    lmin, lmax = M.last_spectrum_srpoly()
    assert lmax == hp.srpoly_bound(M) and lmin == lmax / EIG_RATIO, (lmin, lmax)
    _, _, _, tr_ref = restated_srpoly(A, A.b, minv, degree, lmin, lmax, 200)
    assert tr_ref[0] == r0
    checked = check_trace(tr, tr_ref, RTRANS_RTOL_1GPU)
    print(f"{shape} degree {degree}: {checked} trace points checked, niters {niters}")
    assert checked >= 8, checked
    err = float(np.max(np.abs(x - A.xexact)))
    print(f"{shape} degree {degree}: normr/r0 {normr / r0:.3e} max |x - xexact| {err:.3e}")
    assert normr <= 1e-14 * r0 and niters < 199
    assert err <= 1e-9, err
    # the classic form on the device stops at the same iteration
    _, it_poly, _, _ = tpo.poly_solve(hp, gpu, M, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    assert niters == it_poly, (niters, it_poly)
    # niters under a tolerance between two residuals of the restatement: the
    # widest gap in the middle third of the checked part
    lo, hi = checked // 3, 2 * checked // 3
    k = lo + int(np.argmax(tr_ref[lo:hi] / tr_ref[lo + 1:hi + 1]))
    assert tr_ref[k] > 1.01 * tr_ref[k + 1], (k, tr_ref[k], tr_ref[k + 1])
    tol = float(np.sqrt(tr_ref[k] * tr_ref[k + 1]))
    _, it_ref, nr_ref, _ = restated_srpoly(A, A.b, minv, degree, lmin, lmax, 200, tol)
    _, it, nr, _ = srpoly_solve(hp, gpu, M, B, X0, 200, tol, degree=degree)[0]
    assert it == it_ref and 0 < it < niters, (it, it_ref, niters)
    assert abs(nr - nr_ref) <= RTRANS_RTOL_1GPU * nr_ref, (nr, nr_ref)


# ---------------------------------------------------------------------------
# 6. the bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + LAP + ["p2_33c", "p10_band600"])
def test_the_bound_is_poly_bounds(hp, gpu, shape):
    import torch
    M, A, _ = problem(hp, shape)
    ref = hp.poly_bound(M)
    assert np.float64(hp.srpoly_bound(M)).tobytes() == np.float64(ref).tobytes()
    assert hp.srpoly_bound(M) == ref  # (cached)
    m = torch.from_numpy(np.random.default_rng(23).uniform(0.25, 4.0, A.nrow)).to(gpu)
    assert np.float64(hp.srpoly_bound(M, m)).tobytes() == np.float64(hp.poly_bound(M, m)).tobytes()


# ---------------------------------------------------------------------------
# 7. host and device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2_33c", "p10_dyadic_csr513", "band600"])
def test_host_solve_and_explicit_jacobi_are_the_device_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 3)
    ref = srpoly_solve(hp, gpu, M, B, X0, 25, degree=3)
    spectrum = M.last_spectrum_srpoly()

    def host(**kw):
        X = X0.copy()
        ierr, its, nrs, times = hp.HPCCG_srpoly(M, B, X, degree=3, max_iter=25, **kw)
        assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
        return [(X[c], int(its[c]), float(nrs[c]), M.last_trace_srpoly(c).copy()) for c in range(3)]

    assert_same(host(), ref)
    minv = 1.0 / csr_diagonal(A)
    assert_same(srpoly_solve(hp, gpu, M, B, X0, 25, degree=3, minv=minv), ref)  # (its bound computed in the call)
    assert M.last_spectrum_srpoly() == spectrum
    assert_same(host(minv=minv), ref)
    assert_same(host(minv=minv, lmax=spectrum[1]), ref)
    assert_same(host(lmin=spectrum[0], lmax=spectrum[1]), ref)
    # one column as a vector, updated in place
    x = X0[1].copy()
    hp.HPCCG_srpoly(M, B[1].copy(), x, degree=3, max_iter=25)
    assert x.tobytes() == ref[1][0].tobytes()


# ---------------------------------------------------------------------------
# 8. degenerate columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (0, 2))
@pytest.mark.parametrize("shape", cc.SHAPES)
def test_degenerate_columns(hp, gpu, shape, degree):
    M, A, _ = (tm if shape in cc.REFINED else tp).problem(hp, shape)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    FB, FX = cc.finite_columns(A.b, A.xexact)
    todo = cc.shape_cases(shape, A)
    by_name = {name: (b, x0) for name, b, x0, _, _ in todo}
    refs = {}

    def one(b, x0, mi, tol):
        key = (b.tobytes(), x0.tobytes(), mi, tol)
        if key not in refs:
            refs[key] = srpoly_solve(hp, gpu, M, b.reshape(1, n).copy(), x0.reshape(1, n).copy(), mi, tol,
                                     degree=degree)[0]
        return refs[key]

    usual = srpoly_solve(hp, gpu, M, FB, FX, cc.MAX_ITER, degree=degree)
    lmin, lmax = M.last_spectrum_srpoly()
    # a bad column alone: the outcome every case comes to, with the classic restatement's niters
    for name, b, x0, mi, tol in todo:
        got = one(b, x0, mi, tol)
        try:
            cc.degenerate(*got, x0)
            if degree == 0:
                _, it, nr, _ = cc.expect_pcg(A, b, x0, mi, tol)
            else:
                _, it, nr, _ = tpo.restated(A, b, minv, degree, lmin, lmax, mi, tol, x0=x0)
            assert got[1] == it, (got[1], it)
            assert math.isnan(got[2]) == math.isnan(nr) and (got[2] == 0.0) == (nr == 0.0), (got[2], nr)
        except AssertionError as e:
            raise AssertionError(f"{shape}/{name}: {e}") from None
    # among finite columns
    for label, cols, tol in cc.arrangements([t[0] for t in todo]):
        B, X0 = cc.assemble(cols, FB, FX, by_name)
        got = srpoly_solve(hp, gpu, M, B, X0, cc.MAX_ITER, tol, degree=degree)
        for c, col in enumerate(cols):
            try:
                if isinstance(col, int):
                    assert_same([got[c]], [one(FB[col], FX[col], cc.MAX_ITER, tol)])
                    assert np.all(np.isfinite(got[c][0]))
                else:
                    ts.same_outcome(got[c], one(*by_name[col], cc.MAX_ITER, tol))
            except AssertionError as e:
                raise AssertionError(f"{shape} {label} column {c} ({col}): {e}") from None
        # nothing of a bad column stays in the workspace
        if label in ("4/nan_b@0", "5/bad@4", "3/two_bad"):
            assert_same(srpoly_solve(hp, gpu, M, FB, FX, cc.MAX_ITER, degree=degree), usual)
    assert_same(srpoly_solve(hp, gpu, M, FB, FX, cc.MAX_ITER, degree=degree), usual)


# ---------------------------------------------------------------------------
# 9. refusals
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
                hp.HPCCG_srpoly(M, Bd, Xd, max_iter=10, device=True)
        with pytest.raises(hp.HPCCGError, match=rf"row {row} "):
            hp.srpoly_bound(M)
        assert hp.lib().hpccg_hip_last_error().startswith(b"srpoly:")
        assert torch.all(Xd == 0.5)
        # a caller's m is taken on the same matrix
        assert hp.HPCCG_srpoly(M, Bd, Xd.clone(), max_iter=3, minv=torch.ones(n, dtype=torch.float64, device=gpu),
                               device=True)[0] == 0
    finally:
        M.close()


def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.srpoly_lib()
    M, A, _ = problem(hp, "16c")
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = srpoly_solve(hp, gpu, M, B, X0, 10)
    err = hp.lib().hpccg_hip_last_error

    def call(h, nrhs=2, ldb=n, ldx=n, minv=None, degree=2, lmin=0.0, lmax=0.0, max_iter=10):
        return L.hpccg_hip_srpoly_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, minv, degree, lmin,
                                               lmax, max_iter, 0.0, it, nr, None)

    members = hp.group_generate(8, 8, 8, nranks=2)
    try:
        for m in members:
            assert call(m.h) == EINVAL
            assert b"group" in err()
            with pytest.raises(hp.HPCCGError):
                hp.srpoly_bound(m)
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
            hp.HPCCG_srpoly(M, B.copy(), X0.copy(), max_iter=10, minv=mv)
        with pytest.raises(hp.HPCCGError, match=r"minv\[700\]"):
            hp.srpoly_bound(M, md)
    bound = hp.srpoly_bound(M)
    for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (-1.0, 2.0), (float("nan"), 2.0), (0.5, float("inf")),
                       (bound, 0.0), (2.0 * bound, 0.0)):  # (the last two: against the computed lmax)
        assert call(M.h, lmin=lmin, lmax=lmax) == EINVAL, (lmin, lmax)
        assert b"bounds" in err() and err().startswith(b"srpoly:")
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
    assert_same(srpoly_solve(hp, gpu, M, B, X0, 10), ref)
    assert call(M.h, degree=16) == 0


# ---------------------------------------------------------------------------
# 10. both non-temporal arms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tn.SHAPES)
def test_both_nt_arms_give_the_same_bits(hp, gpu, shape):
    """(The nt = 0 forms are held to HPCCG_poly and the restatement above; a
    chunk whose columns all run takes the arm, one with an ended column the
    general slot loop. Degree 3: steps into both z buffers, u in buffer 1;
    degree 2: u in buffer 0.)"""
    M, A = tn.problem(hp, shape)
    assert M.get_option("nt") == 0  # (the automatic flag at these sizes)
    sets = (tn.active_columns(A.b, 4), columns(A.b, A.xexact, 4))
    degrees = (3, 2)
    refs = [[srpoly_solve(hp, gpu, M, B, X0, 25, degree=d) for d in degrees] for B, X0 in sets]
    assert [r[1] for r in refs[0][0]] == [24] * 4 and refs[1][0][2][1] == 0
    try:
        for nt in (1, 0):
            M.set_option("nt", nt)
            assert M.get_option("nt") == nt
            for (B, X0), ref in zip(sets, refs):
                for nrhs in (4, 2, 1):
                    for d, want in zip(degrees, ref):
                        assert_same(srpoly_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 25, degree=d), want[:nrhs])
    finally:
        M.set_option("nt", -1)
    assert M.get_option("nt") == 0
    assert_same(srpoly_solve(hp, gpu, M, *sets[0], 25, degree=3), refs[0][0])  # nothing of the forced runs stays


# ---------------------------------------------------------------------------
# 11., 12. other solves, repeats, the workspace
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["33c", "p2_dyadic_csr3000"])
def test_other_solves_and_repeats_are_undisturbed(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 3)

    def others():
        single = single_solves(hp, gpu, M, B[:2], X0[:2], 40)
        Bd, Xd = dev(gpu, B), dev(gpu, X0)
        ierr, its, nrs, _ = hp.HPCCG_batch(M, Bd, Xd, max_iter=40, device=True)
        assert ierr == 0
        rest = tp.pcg_solve(hp, gpu, M, B, X0, 40) + ts.srcg_solve(hp, gpu, M, B, X0, 40) + \
            tpo.poly_solve(hp, gpu, M, B, X0, 40)
        return single + rest, (Xd.cpu().numpy().tobytes(), its.tobytes(), nrs.tobytes())

    before = others()
    first = srpoly_solve(hp, gpu, M, B, X0, 40)
    after = others()
    assert_same(after[0], before[0])
    assert after[1] == before[1]
    for _ in range(3):
        assert_same(srpoly_solve(hp, gpu, M, B, X0, 40), first)
    # a solve of another degree between two leaves nothing behind (u moves between the z buffers)
    srpoly_solve(hp, gpu, M, B, X0, 40, degree=3)
    srpoly_solve(hp, gpu, M, B, X0, 40, degree=0)
    assert_same(srpoly_solve(hp, gpu, M, B, X0, 40), first)
    assert M.srpoly_workspace_bytes() > 0
    M.batch_release()


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.srpoly_live_workspaces()
    prob = hp.generate_matrix(8, 8, 8)
    M = hp.Matrix.from_hpc(prob)
    M2 = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 2)
        first = srpoly_solve(hp, gpu, M, B, X0, 10)
        srpoly_solve(hp, gpu, M2, B, X0, 10)
        assert hp.srpoly_live_workspaces() == base + 2
        assert M2.srpoly_workspace_bytes() > 2 * 8 * 512
        M2.srpoly_release()
        assert hp.srpoly_live_workspaces() == base + 1 and M2.srpoly_workspace_bytes() == 0
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            M2.last_spectrum_srpoly()
        assert_same(srpoly_solve(hp, gpu, M2, B, X0, 10), first)  # rebuilt on demand, the caches too
        small = M2.srpoly_workspace_bytes()
        srpoly_solve(hp, gpu, M2, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the caches stay
        assert M2.srpoly_workspace_bytes() > small
        assert_same(srpoly_solve(hp, gpu, M2, B, X0, 10), first)  # (p and s of the larger call are never read)
        M2.srpoly_release()
        M2.srpoly_release()  # (idempotent)
        assert hp.srpoly_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()
        M2.close()
        prob.close()
    assert hp.srpoly_live_workspaces() == base
