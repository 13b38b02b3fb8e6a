"""Single-reduction preconditioned CG (include/hpccg_hip_srcg.h,
lib/libhpccg_hip_srcg.so): the Chronopoulos-Gear form of HPCCG_pcg, per column
the recurrence of the header, restated below in NumPy (restated_sr, importable
without a GPU: tests/test_srcg_cpu.py pins it against test_gpu_pcg.restated).

  1. the first iteration is HPCCG_pcg's bit for bit (max_iter 0, 1, 2; the
     trace still at max_iter 3);
  2. column c of a multi-column call is bitwise the one-column call, under a
     tolerance that freezes columns part-way too;
  3. m = 2^-3 and m = 2^5 everywhere: the bits of m = 1;
  4. Jacobi on S A S with S b, S powers of two: s_i x'_i is bitwise the x of
     Jacobi on A with b;
  5. on matrices scaled by s_i = 10^u_i: the restatement (trace, niters under a
     tolerance, x against xexact), and HPCCG_pcg's trace and niters;
  6. host solve = device solve = explicit 1 / diagonal;
  7. refusals; 8. degenerate columns; 9. both non-temporal arms; 10. other
     solvers and repeats undisturbed; 11. the workspace's life.

Shapes and helpers: those of test_gpu_pcg.py and test_gpu_mixed.py.
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
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_mixed import assert_same, columns, dev, single_solves
from test_gpu_pcg import BASE, P2, P10, csr_diagonal, problem

pytestmark = pytest.mark.gpu

EINVAL = -1


# ---------------------------------------------------------------------------
# The recurrence of include/hpccg_hip_srcg.h restated: oracle.sparsemv and a
# fixed-order (sequential) float64 dot by default (dot: another order, for the
# restatement's own error). trace[k] is the normr iteration k reports,
# sqrt(rr_{k-1}), as in every solver here. steps (a list): (k, p, s) of every
# iteration is appended to it.
# ---------------------------------------------------------------------------
def seq_dot(x, y):
    return np.float64(oracle.ddot(x, y))


def restated_sr(A, b, minv, max_iter, tol=0.0, x0=None, dot=seq_dot, steps=None):
    with np.errstate(all="ignore"):
        x = np.zeros(A.nrow) if x0 is None else np.array(x0, np.float64)
        t = x + 0.0 * x
        r = b + (-1.0) * oracle.sparsemv(A, t)
        u = minv * r
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
            if steps is not None:
                steps.append((k, p.copy(), s.copy()))
            x = x + alpha * p
            r = r + (-alpha) * s
            u = minv * r
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
    for cache in (tm._problems, tp._problems):
        for M, _, _ in cache.values():
            M.close()
        cache.clear()
    assert hp.srcg_live_workspaces() == 0
    assert hp.pcg_live_workspaces() == 0


def srcg_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, minv=None, ld=None):
    """[(x, niters, normr, trace)] per column of a device solve; minv: None
    (Jacobi), a number (that value everywhere) or an array."""
    import torch
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    if minv is not None:
        minv = torch.from_numpy(np.full(n, 1.0) * np.float64(minv)).to(gpu)
    ierr, its, nrs, times = hp.HPCCG_srcg(M, Bd, Xd, max_iter=max_iter, tolerance=tol, minv=minv, device=True)
    assert ierr == 0 and times[0] > 0.0 and not times[1:].any()
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_srcg(c).copy()) for c in range(B.shape[0])]


def test_every_image_form_is_exercised(hp, gpu):
    """Widths 27, 7, per-slice (0) of SELL-512-A and the SELL-512 form, plain and scaled."""
    forms = {}
    for name in BASE + P2 + P10:
        M, _, _ = problem(hp, name)
        forms[name] = (M.get_option("has_a"), M.get_option("a_width") if M.get_option("has_a") else None)
    for pre in ("", "p2_", "p10_"):
        assert forms[pre + "33c"] == (1, 27) and forms[pre + "16c"] == (1, 27), forms
        assert forms[pre + "12x10x16_7pt"] == (1, 7), forms
        assert forms[pre + "band600"] == (1, 0), forms
        assert forms[pre + "dyadic_csr513"] == (0, None), forms
    assert forms["dyadic_csr3000"] == (0, None) and forms["p2_dyadic_csr3000"] == (0, None), forms


# ---------------------------------------------------------------------------
# 1. the first iteration
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2)
def test_the_first_iteration_is_pcgs(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 5)
    assert X0[1].any()  # a nonzero x0 among them
    for minv in (None, 1.0):
        for max_iter in (0, 1, 2):
            ref = tp.pcg_solve(hp, gpu, M, B, X0, max_iter, minv=minv)
            assert_same(srcg_solve(hp, gpu, M, B, X0, max_iter, minv=minv), ref)
            assert max(r[1] for r in ref) == max(max_iter, 1) - 1
        ref = tp.pcg_solve(hp, gpu, M, B, X0, 3, minv=minv)
        got = srcg_solve(hp, gpu, M, B, X0, 3, minv=minv)
        for c in range(5):
            assert got[c][1] == ref[c][1] and got[c][3].tobytes() == ref[c][3].tobytes(), (minv, c)


# ---------------------------------------------------------------------------
# 2. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2)
def test_columns_are_single_column_calls(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 5)

    def ones(tol):
        return [srcg_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 60, tol)[0] for c in range(5)]

    full = ones(0.0)
    # a tolerance that column 0 meets part-way: just above the smallest residual of its first half
    tr0 = full[0][3]
    half = tr0[:len(tr0) // 2 + 1]
    half = half[np.isfinite(half) & (half > 0.0)]
    tol = float(np.min(half)) * (1.0 + 2.0 ** -10) if len(tr0) > 4 and len(half) else 0.0
    part = ones(tol)
    print(f"{shape}: stops {[r[1] for r in part]} under the tolerance, {[r[1] for r in full]} without")
    if n > 1:
        assert part[0][1] < full[0][1], (part[0][1], full[0][1])
    assert full[2][1] == 0  # (x0 = xexact: frozen since the prologue)
    for t, ref in ((0.0, full), (tol, part)):
        for nrhs, ld in ((5, n), (4, n), (3, n + 3), (2, n), (1, n)):
            assert_same(srcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 60, t, ld=ld), ref[:nrhs])


# ---------------------------------------------------------------------------
# 3. a uniform power-of-two m
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2)
def test_a_uniform_power_of_two_m_is_m_one(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 5)
    ref = srcg_solve(hp, gpu, M, B, X0, 60, minv=1.0)
    assert ref[0][1] > 0 or A.nrow == 1
    for m in (2.0 ** -3, 2.0 ** 5):
        for nrhs in (5, 1):
            assert_same(srcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 60, minv=m), ref[:nrhs])


# ---------------------------------------------------------------------------
# 4. exact scaling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["33c", "16c", "dyadic_csr3000", "dyadic_csr513"])
def test_jacobi_commutes_with_a_power_of_two_scaling(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    Ms, As, s = problem(hp, "p2_" + shape)
    n = A.nrow
    rng = np.random.default_rng(3)
    B = np.stack([A.b, rng.uniform(-1.0, 1.0, n), A.b * 2.0 ** -7, rng.uniform(-1.0, 1.0, n)])
    X0 = np.zeros((4, n))
    for nrhs in (4, 1, 2):
        got = srcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 20)
        gots = srcg_solve(hp, gpu, Ms, B[:nrhs] * s, X0[:nrhs], 20)
        for c in range(nrhs):
            assert got[c][1] == gots[c][1] == 19
            assert (gots[c][0] * s).tobytes() == got[c][0].tobytes(), (nrhs, c, float(np.max(np.abs(gots[c][0] * s - got[c][0]))))
            assert np.all(np.isfinite(got[c][0])) and got[c][0].any()


# ---------------------------------------------------------------------------
# 5. the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P10)
def test_jacobi_follows_the_restatement(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    _, _, _, tr_ref = restated_sr(A, A.b, minv, 200)
    r0 = tr_ref[0]
    # the trace, as far as the restatement is above the rounding floor; converged is normr <= 1e-14 r0
    x, niters, normr, tr = srcg_solve(hp, gpu, M, B, X0, 200, 1e-14 * r0)[0]
    checked = check_trace(tr, tr_ref, RTRANS_RTOL_1GPU)
    print(f"{shape}: {checked} trace points checked, niters {niters}")
    assert checked >= 10, checked
    err = float(np.max(np.abs(x - A.xexact)))
    print(f"{shape}: normr/r0 {normr / r0:.3e} max |x - xexact| {err:.3e}")
    assert normr <= 1e-14 * r0 and niters < 199
    assert err <= 1e-9, err
    # the same run against the classic recurrence on the device
    _, it_pcg, _, tr_pcg = tp.pcg_solve(hp, gpu, M, B, X0, 200, 1e-14 * r0)[0]
    assert check_trace(tr, tr_pcg, RTRANS_RTOL_1GPU) >= 10
    assert niters == it_pcg, (niters, it_pcg)
    # niters under a tolerance between two residuals of the restatement: the
    # widest gap in the middle third of the checked part
    lo, hi = checked // 3, 2 * checked // 3
    k = lo + int(np.argmax(tr_ref[lo:hi] / tr_ref[lo + 1:hi + 1]))
    assert tr_ref[k] > 1.01 * tr_ref[k + 1], (k, tr_ref[k], tr_ref[k + 1])
    tol = float(np.sqrt(tr_ref[k] * tr_ref[k + 1]))
    _, it_ref, nr_ref, _ = restated_sr(A, A.b, minv, 200, tol)
    _, it, nr, _ = srcg_solve(hp, gpu, M, B, X0, 200, tol)[0]
    assert it == it_ref and 0 < it < niters, (it, it_ref, niters)
    assert abs(nr - nr_ref) <= RTRANS_RTOL_1GPU * nr_ref, (nr, nr_ref)


# ---------------------------------------------------------------------------
# 6. host and device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2_33c", "p10_dyadic_csr513", "band600"])
def test_host_solve_and_explicit_jacobi_are_the_device_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    B, X0 = columns(A.b, A.xexact, 3)
    ref = srcg_solve(hp, gpu, M, B, X0, 25)
    X = X0.copy()
    ierr, its, nrs, times = hp.HPCCG_srcg(M, B, X, max_iter=25)
    assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
    assert_same([(X[c], int(its[c]), float(nrs[c]), M.last_trace_srcg(c).copy()) for c in range(3)], ref)
    minv = 1.0 / csr_diagonal(A)
    assert_same(srcg_solve(hp, gpu, M, B, X0, 25, minv=minv), ref)
    X = X0.copy()
    ierr, its, nrs, _ = hp.HPCCG_srcg(M, B, X, max_iter=25, minv=minv)
    assert_same([(X[c], int(its[c]), float(nrs[c]), M.last_trace_srcg(c).copy()) for c in range(3)], ref)
    # one column as a vector, updated in place
    x = X0[1].copy()
    hp.HPCCG_srcg(M, B[1].copy(), x, max_iter=25)
    assert x.tobytes() == ref[1][0].tobytes()


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("base,edit", [("band600", tp._zero_diag), ("dyadic_csr513", tp._negative_diag),
                                       ("band600", tp._missing_diag), ("dyadic_csr3000", tp._missing_diag)],
                         ids=["zero_a", "negative_sell", "missing_a", "missing_sell"])
def test_a_bad_diagonal_is_refused(hp, gpu, base, edit):
    import torch
    A = tp.base_csr(base)
    n = A.nrow
    rp, cols, vals, row = tp._edited(A, edit)
    M = hp.Matrix.from_csr(rp, cols, vals)
    try:
        Bd = torch.ones((2, n), dtype=torch.float64, device=gpu)
        Xd = torch.full((2, n), 0.5, dtype=torch.float64, device=gpu)
        it = (C.c_int * 2)()
        nr = (C.c_double * 2)()
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match=rf"row {row} "):
                hp.HPCCG_srcg(M, Bd, Xd, max_iter=10, device=True)
        assert hp.srcg_lib().hpccg_hip_srcg_solve_device(M.h, 2, Bd.data_ptr(), n, Xd.data_ptr(), n, None, 10, 0.0, it,
                                                         nr, None) == EINVAL
        assert hp.lib().hpccg_hip_last_error().startswith(b"srcg:")
        assert torch.all(Xd == 0.5)
        # a caller's m is taken on the same matrix
        assert hp.HPCCG_srcg(M, Bd, Xd.clone(), max_iter=3, minv=torch.ones(n, dtype=torch.float64, device=gpu),
                             device=True)[0] == 0
    finally:
        M.close()


def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.srcg_lib()
    M, A, _ = problem(hp, "16c")
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = srcg_solve(hp, gpu, M, B, X0, 10)

    def call(h, nrhs=2, ldb=n, ldx=n, minv=None, max_iter=10):
        return L.hpccg_hip_srcg_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, minv, max_iter, 0.0, it,
                                             nr, None)

    members = hp.group_generate(8, 8, 8, nranks=2)
    try:
        for m in members:
            assert call(m.h) == EINVAL
            assert b"group" in hp.lib().hpccg_hip_last_error()
    finally:
        for m in members:
            m.close()
    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        mv = np.ones(n)
        mv[700] = bad
        mv[3000] = bad
        md = torch.from_numpy(mv).to(gpu)
        assert call(M.h, minv=md.data_ptr()) == EINVAL
        assert b"minv[700]" in hp.lib().hpccg_hip_last_error()
        with pytest.raises(hp.HPCCGError, match=r"minv\[700\]"):
            hp.HPCCG_srcg(M, B.copy(), X0.copy(), max_iter=10, minv=mv)
    assert call(M.h, ldb=n - 1) == EINVAL
    assert b"leading dimension" in hp.lib().hpccg_hip_last_error()
    assert call(M.h, ldx=n - 1) == EINVAL
    assert call(M.h, max_iter=-1) == EINVAL
    assert call(M.h, nrhs=0) == EINVAL
    assert call(None) == EINVAL
    assert Xd.cpu().numpy().tobytes() == X0.tobytes()  # nothing was touched
    # ... and a good solve afterwards
    assert_same(srcg_solve(hp, gpu, M, B, X0, 10), ref)


# ---------------------------------------------------------------------------
# 8. degenerate columns
# ---------------------------------------------------------------------------
def same_outcome(got, ref):
    """A bad column against its reference: niters equal, normr equal or both
    NaN, x and trace equal with NaN where the reference's is NaN."""
    assert got[1] == ref[1], ("niters", got[1], ref[1])
    assert got[2] == ref[2] or (math.isnan(got[2]) and math.isnan(ref[2])), ("normr", got[2], ref[2])
    assert np.array_equal(got[0], ref[0], equal_nan=True), "x"
    assert np.array_equal(got[3], ref[3], equal_nan=True), ("trace", got[3], ref[3])


@pytest.mark.parametrize("shape", cc.SHAPES)
def test_degenerate_columns(hp, gpu, shape):
    M, A, _ = (tm if shape in cc.REFINED else tp).problem(hp, shape)
    n = A.nrow
    FB, FX = cc.finite_columns(A.b, A.xexact)
    todo = cc.shape_cases(shape, A)
    by_name = {name: (b, x0) for name, b, x0, _, _ in todo}
    refs = {}

    def one(b, x0, mi, tol):
        key = (b.tobytes(), x0.tobytes(), mi, tol)
        if key not in refs:
            refs[key] = srcg_solve(hp, gpu, M, b.reshape(1, n).copy(), x0.reshape(1, n).copy(), mi, tol)[0]
        return refs[key]

    usual = srcg_solve(hp, gpu, M, FB, FX, cc.MAX_ITER)
    # a bad column alone: the outcome every case comes to, with the classic restatement's niters
    for name, b, x0, mi, tol in todo:
        got = one(b, x0, mi, tol)
        try:
            cc.degenerate(*got, x0)
            _, it, nr, _ = cc.expect_pcg(A, b, x0, mi, tol)
            assert got[1] == it and math.isnan(got[2]) == math.isnan(nr), (got[1:3], it, nr)
        except AssertionError as e:
            raise AssertionError(f"{shape}/{name}: {e}") from None
    # among finite columns
    for label, cols, tol in cc.arrangements([t[0] for t in todo]):
        B, X0 = cc.assemble(cols, FB, FX, by_name)
        got = srcg_solve(hp, gpu, M, B, X0, cc.MAX_ITER, tol)
        for c, col in enumerate(cols):
            try:
                if isinstance(col, int):
                    assert_same([got[c]], [one(FB[col], FX[col], cc.MAX_ITER, tol)])
                    assert np.all(np.isfinite(got[c][0]))
                else:
                    same_outcome(got[c], one(*by_name[col], cc.MAX_ITER, tol))
            except AssertionError as e:
                raise AssertionError(f"{shape} {label} column {c} ({col}): {e}") from None
        # nothing of a bad column stays in the workspace
        if label in ("4/nan_b@0", "5/bad@4", "3/two_bad"):
            assert_same(srcg_solve(hp, gpu, M, FB, FX, cc.MAX_ITER), usual)
    assert_same(srcg_solve(hp, gpu, M, FB, FX, cc.MAX_ITER), usual)


# ---------------------------------------------------------------------------
# 9. both non-temporal arms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tn.SHAPES)
def test_both_nt_arms_give_the_same_bits(hp, gpu, shape):
    """(The nt = 0 forms are held to HPCCG_pcg and the restatement above; a
    chunk whose columns all run takes the arm, one with an ended column the
    general slot loop.)"""
    M, A = tn.problem(hp, shape)
    assert M.get_option("nt") == 0  # (the automatic flag at these sizes)
    sets = (tn.active_columns(A.b, 4), columns(A.b, A.xexact, 4))
    refs = [[srcg_solve(hp, gpu, M, B, X0, 25, minv=m) for m in (None, 1.0)] for B, X0 in sets]
    assert [r[1] for r in refs[0][0]] == [24] * 4 and refs[1][0][2][1] == 0
    try:
        for nt in (1, 0):
            M.set_option("nt", nt)
            assert M.get_option("nt") == nt
            for (B, X0), ref in zip(sets, refs):
                for nrhs in (4, 2, 1):
                    for m, want in zip((None, 1.0), ref):
                        assert_same(srcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 25, minv=m), want[:nrhs])
    finally:
        M.set_option("nt", -1)
    assert M.get_option("nt") == 0
    assert_same(srcg_solve(hp, gpu, M, *sets[0], 25), refs[0][0])  # nothing of the forced runs stays


# ---------------------------------------------------------------------------
# 10., 11. other solves, repeats, the workspace
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
        return single + tp.pcg_solve(hp, gpu, M, B, X0, 40), (Xd.cpu().numpy().tobytes(), its.tobytes(), nrs.tobytes())

    before = others()
    first = srcg_solve(hp, gpu, M, B, X0, 40)
    after = others()
    assert_same(after[0], before[0])
    assert after[1] == before[1]
    for _ in range(3):
        assert_same(srcg_solve(hp, gpu, M, B, X0, 40), first)
    assert M.srcg_workspace_bytes() > 0
    M.batch_release()


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.srcg_live_workspaces()
    prob = hp.generate_matrix(8, 8, 8)
    M = hp.Matrix.from_hpc(prob)
    M2 = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 2)
        first = srcg_solve(hp, gpu, M, B, X0, 10)
        srcg_solve(hp, gpu, M2, B, X0, 10)
        assert hp.srcg_live_workspaces() == base + 2
        assert M2.srcg_workspace_bytes() > 2 * 8 * 512
        M2.srcg_release()
        assert hp.srcg_live_workspaces() == base + 1 and M2.srcg_workspace_bytes() == 0
        assert_same(srcg_solve(hp, gpu, M2, B, X0, 10), first)  # rebuilt on demand, the Jacobi cache too
        small = M2.srcg_workspace_bytes()
        srcg_solve(hp, gpu, M2, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the cache stays
        assert M2.srcg_workspace_bytes() > small
        assert_same(srcg_solve(hp, gpu, M2, B, X0, 10), first)  # (p and s of the larger call are never read)
        M2.srcg_release()
        M2.srcg_release()  # (idempotent)
        assert hp.srcg_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()
        M2.close()
        prob.close()
    assert hp.srcg_live_workspaces() == base
