"""Chebyshev polynomial preconditioned CG over an in-process rank group
(include/hpccg_hip_poly_group.h, lib/libhpccg_hip_poly_group.so): per column
the recurrence of hpccg_hip_poly.h, every member on its own rows, the ghost
planes of z moved after step 0 and after every step but the last and those of p
after the p update (one kernel per member each), the dots summed over the
members in rank order. All members share one device.

  1. degree 0 is the group pcg bit for bit (every member's x, niters, normr,
     every trace);
  2. a group of one is the one-rank solve bit for bit, with its spectrum and
     bound;
  3. column c of a multi-column call is bitwise its single-column call;
  4. exact scaling by powers of two, explicit bounds and the default bound;
  5. the halo kernel against the halo by copies: the same bits;
  6. the bound against NumPy's of the global matrix, its exact values and its
     exact scaling;
  7. on matrices scaled by s_i = 10^u_i: the trace against the NumPy
     restatement and against the one-rank solve of the global matrix (they
     differ in the dots' summation order only), niters under a tolerance, x
     against xexact, degrees 1 to 4;
  8. it does what it is for; 9. degenerate columns; 10. refusals;
  11. the other solves are undisturbed; 12. the workspace's life.

Shapes: those of test_gpu_pcg_group.py with its Case machinery (2 x 8^3: one
slice per member; 8 x 16^3: interior members with both ghost planes;
3 x 33x17x9: unaligned odd planes that start in a slice's padding; 4 x 7x5x1:
ghost planes as large as the member; 2 x 12x10x8 7-pt; csr3: the int32-column
image), their "p2_" / "p10_" forms, and "lap_" forms of the 27-pt stencils:
every diagonal entry 26.0 (weakly diagonally dominant), split into the same
slabs by group_from_csr.

7.: the restatement run on the CPU under three dot orders -- oracle.ddot's
sequential sum, np.dot, and the sequential sums of the members' slabs added in
rank order -- with the bound from test_gpu_poly.numpy_bound and lmin = lmax / 30,
degrees 1 to 4, 200 iterations at most, tolerance 1e-14 r0, on the seven shapes
of 7. and on p10_lap_2x16x16x8: 11 to 43 trace points are kept on every
shape/degree pair, niters is the same under the three orders in every case, and
the worst disagreement of the restatement with itself on rtrans over the points
kept is 3.5e-10 (p10_lap_2x16x16x8, degree 1), 2.9e-11 on p10_lap_3x33x17x9,
9.8e-12 on p10_4x7x5x1 and <= 3.0e-12 everywhere else; its x is within 7.0e-11
of xexact. Every disagreement is at most 1/280 of RTRANS_RTOL_MULTI, so the bar
has room for the members' summation order and for nothing else.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import test_gpu_pcg_group as tpg
import test_gpu_poly as tpo
from conftest import RTRANS_RTOL_MULTI, check_trace
from test_gpu_pcg_group import SHAPES, assert_same, columns, csr_diagonal, dev, finish, rows_of, scale_of, scaled

pytestmark = pytest.mark.gpu

EINVAL, EPLAN = -1, -5
MAX_ITER = 60
EIG_RATIO = 30.0
DEGREES = (1, 2, 3, 4)


# ---------------------------------------------------------------------------
# problems: test_gpu_pcg_group.Case, and the "lap_" forms beside it
# ---------------------------------------------------------------------------
def lap_global(name):
    A0, counts = tpg.global_matrix(name)
    vals = A0.vals.copy()
    vals[rows_of(A0) == A0.cols] = 26.0
    return finish(A0.row_ptr, A0.cols, vals), counts


def make_case(hp, name):
    kind, _, rest = name.partition("_")
    if kind not in ("p2", "p10"):
        kind, rest = None, name
    if not rest.startswith("lap_"):
        return tpg.Case(hp, name)
    A, counts = lap_global(rest[4:])
    cs = object.__new__(tpg.Case)
    cs.s = scale_of(kind, A.nrow) if kind else None
    cs.A = scaled(A, cs.s) if kind else A
    cs.Ms = tpg.members_from_csr(hp, cs.A, counts)
    cs.has_a = 1
    assert [M.get_option("has_a") for M in cs.Ms] == [1] * len(counts), name
    cs.P = len(counts)
    cs.rows, s = [], 0
    for n in counts:
        cs.rows.append(slice(s, s + n))
        s += n
    cs.N = s
    return cs


_cases = {}


def case(hp, name):
    if name not in _cases:
        _cases[name] = make_case(hp, name)
    return _cases[name]


def live(hp):
    return (hp.group_pcg_live_workspaces(), hp.pcg_live_workspaces(), hp.batch_live_workspaces(),
            hp.poly_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _close_cases(hp):
    base = hp.group_poly_live_workspaces()
    others = live(hp)
    yield
    for c in _cases.values():
        c.close()
    _cases.clear()
    assert hp.group_poly_live_workspaces() == base
    assert live(hp) == others


def poly_solve(hp, gpu, cs, B, X0, max_iter, tol=0.0, degree=2, lmin=None, lmax=None, minv=None, pad=0,
               halo_copies=False):
    """[(xs per member, niters, normr, trace)] per column of a group polynomial
    solve; minv: None (Jacobi), a number (that value everywhere) or a global array."""
    import torch
    Bd = [dev(gpu, a, pad) for a in cs.split(B)]
    Xd = [dev(gpu, a, pad) for a in cs.split(X0)]
    minvs = None
    if minv is not None:
        m = np.full(cs.N, 1.0) * np.float64(minv)
        minvs = [torch.from_numpy(m[rw].copy()).to(gpu) for rw in cs.rows]
    its, nrs, times = hp.group_HPCCG_poly(cs.Ms, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, minvs=minvs,
                                          max_iter=max_iter, tolerance=tol, halo_copies=halo_copies)
    assert times[0] > 0.0 and not times[1:].any()
    X = [x.cpu().numpy() for x in Xd]
    if pad:
        for x, rw in zip(X, cs.rows):
            assert np.all(x[:, rw.stop - rw.start:] == 7.5)  # nothing stored between the columns
    return [([x[c, :rw.stop - rw.start].copy() for x, rw in zip(X, cs.rows)], int(its[c]), float(nrs[c]),
             hp.group_last_trace_poly(cs.Ms, c).copy()) for c in range(B.shape[0])]


def one_rank_matrix(hp, cs):
    return hp.Matrix.from_csr(cs.A.row_ptr, cs.A.cols, cs.A.vals)


# ---------------------------------------------------------------------------
# 1. degree 0 is the group pcg
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_degree_0_is_the_group_pcg(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs)
    assert X0[1].any() and X0[3].any()  # nonzero x0 among them
    m_rand = np.random.default_rng(23).uniform(0.25, 4.0, cs.N)
    every = ((1, 0), (2, 3), (3, 0), (4, 0), (5, 3), (7, 0))  # every chunking of the launches, a padded ld
    for minv, counts in ((None, every), (1.0, ((5, 3), (1, 0))), (m_rand, ((7, 0), (2, 3)))):
        ref = tpg.pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, minv=minv)
        assert ref[0][1] > 0
        for nrhs, pad in counts:
            assert_same(poly_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, degree=0, minv=minv, pad=pad),
                        ref[:nrhs])
        if minv is not None:
            continue
        # a tolerance that column 0 meets part-way, one iteration and none at all
        tr0 = ref[0][3]
        tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10)
        for max_iter, t in ((MAX_ITER, tol), (1, 0.0), (0, 0.0)):
            part = tpg.pcg_solve(hp, gpu, cs, B[:4], X0[:4], max_iter, t)
            if t:
                assert part[0][1] < ref[0][1], (part[0][1], ref[0][1])
            assert_same(poly_solve(hp, gpu, cs, B[:4], X0[:4], max_iter, t, degree=0), part)
        # (bounds given with degree 0 are checked, kept and not used)
        assert_same(poly_solve(hp, gpu, cs, B[:2], X0[:2], MAX_ITER, degree=0, lmin=0.5, lmax=3.0), ref[:2])
        assert hp.group_last_spectrum_poly(cs.Ms) == (0.5, 3.0)


# ---------------------------------------------------------------------------
# 2. a group of one
# ---------------------------------------------------------------------------
def test_group_of_one_is_the_one_rank_solve(hp, gpu):
    """nranks == 1 runs the same code on a halo-free matrix: 0.0 + a total is
    the total, so every column is bitwise HPCCG_poly's."""
    M = hp.Matrix.generate(12, 11, 10)
    G1 = hp.group_generate(12, 11, 10, 1)
    try:
        A = oracle.generate(12, 11, 10)
        rng = np.random.default_rng(3)
        B = np.stack([A.b, rng.uniform(-1.0, 1.0, A.nrow), 0.5 * A.b])
        for degree in DEGREES:
            for nrhs in (3, 1):
                Xs = dev(gpu, np.zeros_like(B[:nrhs]))
                _, its1, nrs1, _ = hp.HPCCG_poly(M, dev(gpu, B[:nrhs]), Xs, degree=degree, max_iter=40, device=True)
                tr1 = [M.last_trace_poly(c).copy() for c in range(nrhs)]
                for Ms in ([M], G1):  # a plain one-rank matrix and a one-member group
                    Bd, Xd = dev(gpu, B[:nrhs]), dev(gpu, np.zeros_like(B[:nrhs]))
                    its, nrs, _ = hp.group_HPCCG_poly(Ms, [Bd], [Xd], degree=degree, max_iter=40)
                    assert list(its) == list(its1) and nrs.tobytes() == nrs1.tobytes(), (degree, nrhs)
                    assert Xd.cpu().numpy().tobytes() == Xs.cpu().numpy().tobytes(), (degree, nrhs)
                    for c in range(nrhs):
                        assert hp.group_last_trace_poly(Ms, c).tobytes() == tr1[c].tobytes()
                    assert hp.group_last_spectrum_poly(Ms) == M.last_spectrum_poly()
            assert its1[0] == 39 and np.all(np.isfinite(Xs.cpu().numpy()))
        assert hp.group_poly_bound([M]) == hp.group_poly_bound(G1) == hp.poly_bound(M)
    finally:
        M.close()
        for m in G1:
            m.close()


# ---------------------------------------------------------------------------
# 3. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2_3x33x17x9", "p10_csr3", "2x12x10x8_7pt"])
def test_columns_are_single_column_calls(hp, gpu, shape):
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    rng = np.random.default_rng(9)
    # the same tolerance meets differently scaled residuals at different iterations
    B = np.stack([A.b, A.b * 2.0 ** -20, rng.uniform(-1.0, 1.0, N) * 2.0 ** 10, A.b * 2.0 ** -40, A.b])
    X0 = np.zeros((5, N))
    X0[4] = A.xexact  # (ends before its first iteration)
    tol = 1e-8 * float(np.linalg.norm(A.b))
    one = [poly_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], 150, tol)[0] for c in range(5)]
    stops = [o[1] for o in one]
    print(f"{shape}: stops {stops}")
    assert len(set(stops)) >= 3 and max(stops) < 149 and stops[4] == 0, stops
    for nrhs, pad in ((5, 5), (4, 0), (3, 0), (2, 0)):
        got = poly_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 150, tol, pad=pad)
        assert_same(got, one[:nrhs])
        for g in got[:4]:
            assert len(g[3]) == g[1] + 1 and g[2] == g[3][-1]


# ---------------------------------------------------------------------------
# 4. exact scaling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "csr3"])
def test_chebyshev_commutes_with_a_power_of_two_scaling(hp, gpu, shape):
    cs, css = case(hp, shape), case(hp, "p2_" + shape)
    assert cs.has_a == css.has_a == tpg.HAS_A[shape]
    s, N = css.s, cs.N
    rng = np.random.default_rng(3)
    B = np.stack([cs.A.b, rng.uniform(-1.0, 1.0, N), cs.A.b * 2.0 ** -7, rng.uniform(-1.0, 1.0, N)])
    X0 = np.zeros((4, N))
    # (2.0 bounds the Jacobi-scaled spectrum of these diagonally dominant matrices); then the default bound
    for kw in (dict(lmin=2.0 / EIG_RATIO, lmax=2.0), dict()):
        for nrhs in (4, 1):
            got = poly_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 12, degree=3, **kw)
            gots = poly_solve(hp, gpu, css, B[:nrhs] * s, X0[:nrhs], 12, degree=3, **kw)
            assert hp.group_last_spectrum_poly(cs.Ms) == hp.group_last_spectrum_poly(css.Ms)
            if kw:
                assert hp.group_last_spectrum_poly(cs.Ms) == (2.0 / EIG_RATIO, 2.0)
            for c in range(nrhs):
                assert got[c][1] == gots[c][1] == 11
                for m, rw in enumerate(cs.rows):
                    x, xs = got[c][0][m], gots[c][0][m] * s[rw]
                    assert xs.tobytes() == x.tobytes(), (kw, nrhs, c, m, float(np.max(np.abs(xs - x))))
                    assert np.all(np.isfinite(x)) and x.any()


# ---------------------------------------------------------------------------
# 5. the halo kernel and the halo by copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "4x7x5x1", "p10_csr3"])
def test_the_halo_kernel_equals_the_copies(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs, 5)
    kernel = poly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=3)
    copies = poly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=3, halo_copies=True)
    assert kernel[0][1] > 0 and all(np.all(np.isfinite(x)) and x.any() for x in kernel[0][0])
    assert_same(kernel, copies)
    assert_same(poly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=3), kernel)  # (the switch is the call's own)


# ---------------------------------------------------------------------------
# 6. the bound
# ---------------------------------------------------------------------------
LAP27 = ["lap_2x8c", "lap_8x16c", "lap_3x33x17x9", "lap_4x7x5x1"]


@pytest.mark.parametrize("shape", SHAPES + LAP27)
def test_the_bound_is_numpys_of_the_global_matrix(hp, gpu, shape):
    import torch
    cs = case(hp, shape)
    A = cs.A
    jac = 1.0 / csr_diagonal(A)
    got = hp.group_poly_bound(cs.Ms)
    ref, w = tpo.numpy_bound(A, jac)
    margin = (w + 3) * 2.0 ** -52  # (test_gpu_poly.py: one rounding per added term, the two products and the sqrt)
    print(f"{shape}: group bound {got!r} numpy {ref!r} widest row {w}")
    assert abs(got - ref) <= margin * ref, (got, ref)
    assert hp.group_poly_bound(cs.Ms) == got  # (cached)
    jacs = [torch.from_numpy(jac[rw].copy()).to(gpu) for rw in cs.rows]
    assert hp.group_poly_bound(cs.Ms, jacs) == got  # a caller's m: the same kernels
    m = np.random.default_rng(23).uniform(0.25, 4.0, cs.N)
    rm, _ = tpo.numpy_bound(A, m)
    gm = hp.group_poly_bound(cs.Ms, [torch.from_numpy(m[rw].copy()).to(gpu) for rw in cs.rows])
    assert abs(gm - rm) <= margin * rm, (gm, rm)
    exact = 2.0 if shape in LAP27 else 53.0 / 27.0 if shape in SHAPES[:4] else None
    if exact is not None:  # (the 27-pt stencils: an interior row has 26 neighbours)
        assert abs(got - exact) <= margin * exact, (got, exact)
    # the power-of-two scaling: q_i / s_i, |a_ij| s_i s_j, exact with a correctly rounded sqrt
    gs = hp.group_poly_bound(case(hp, "p2_" + shape).Ms)
    assert np.float64(gs).tobytes() == np.float64(got).tobytes(), (gs, got)
    # against one rank: the slot order of a row may differ between the images, so this is printed only
    M1 = one_rank_matrix(hp, cs)
    try:
        one = hp.poly_bound(M1)
    finally:
        M1.close()
    print(f"{shape}: one-rank bound {one!r}, bitwise equal: {np.float64(one).tobytes() == np.float64(got).tobytes()}")
    assert abs(one - got) <= 2.0 * margin * ref, (one, got)


# ---------------------------------------------------------------------------
# 7. the restatement and one rank
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("shape", ["p10_" + s for s in SHAPES] + ["p10_lap_3x33x17x9"])
def test_the_group_follows_the_restatement_and_one_rank(hp, gpu, shape, degree):
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    xs, niters, normr, tr = poly_solve(hp, gpu, cs, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    lmin, lmax = hp.group_last_spectrum_poly(cs.Ms)
    assert lmax == hp.group_poly_bound(cs.Ms) and lmin == lmax / EIG_RATIO, (lmin, lmax)
    _, _, _, tr_ref = tpo.restated(A, A.b, minv, degree, lmin, lmax, 200)
    assert tr_ref[0] == r0
    checked = check_trace(tr, tr_ref, RTRANS_RTOL_MULTI)
    print(f"{shape} degree {degree}: {checked} trace points checked against the restatement, niters {niters}")
    assert checked >= 10, checked
    M1 = one_rank_matrix(hp, cs)
    try:
        Bd, Xd = dev(gpu, B), dev(gpu, X0)
        _, it1, _, _ = hp.HPCCG_poly(M1, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, device=True, max_iter=200,
                                     tolerance=1e-14 * r0)
        tr1 = M1.last_trace_poly(0).copy()
    finally:
        M1.close()
    checked1 = check_trace(tr, tr1, RTRANS_RTOL_MULTI)
    print(f"{shape} degree {degree}: {checked1} trace points checked against one rank, niters {niters} / {int(it1[0])}")
    assert checked1 >= 10, checked1
    x = np.concatenate(xs)
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
    _, it_ref, nr_ref, _ = tpo.restated(A, A.b, minv, degree, lmin, lmax, 200, tol)
    _, it, nr, _ = poly_solve(hp, gpu, cs, B, X0, 200, tol, degree=degree)[0]
    assert it == it_ref and 0 < it < niters, (it, it_ref, niters)
    assert abs(nr - nr_ref) <= RTRANS_RTOL_MULTI * nr_ref, (nr, nr_ref)


# ---------------------------------------------------------------------------
# 8. it does what it is for
# ---------------------------------------------------------------------------
def test_degree_3_halves_group_jacobis_iterations(hp, gpu):
    cs = case(hp, "p10_lap_3x33x17x9")
    A, N = cs.A, cs.N
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    tol = 1e-10 * r0
    xs, it, nr, _ = poly_solve(hp, gpu, cs, B, X0, 200, tol, degree=3)[0]
    lmin, lmax = hp.group_last_spectrum_poly(cs.Ms)
    _, it_ref, _, _ = tpo.restated(A, A.b, 1.0 / csr_diagonal(A), 3, lmin, lmax, 200, tol)
    jac = tpg.pcg_solve(hp, gpu, cs, B, X0, 200, tol)[0]
    print(f"p10_lap_3x33x17x9: degree 3 {it} iterations (restatement {it_ref}), group Jacobi {jac[1]}; "
          f"normr/r0 {nr / r0:.3e}")
    assert abs(it - it_ref) <= 2, (it, it_ref)
    assert nr <= tol and jac[2] <= tol
    assert 2 * it <= jac[1], (it, jac[1])


# ---------------------------------------------------------------------------
# 9. degenerate columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "p2_csr3", "2x12x10x8_7pt"])
def test_degenerate_columns_beside_ordinary_ones(hp, gpu, shape):
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    minv = 1.0 / csr_diagonal(A)
    rng = np.random.default_rng(41)
    # a NaN well inside member 1, and one on member 0's last row (a plane member 1 reads)
    inside = (cs.rows[1].start + cs.rows[1].stop) // 2
    plane = cs.rows[0].stop - 1
    nan_in, nan_pl = A.b.copy(), A.b.copy()
    nan_in[inside] = np.nan
    nan_pl[plane] = np.nan
    B = np.stack([A.b, np.zeros(N), nan_in, rng.uniform(-1.0, 1.0, N), nan_pl])
    X0 = np.zeros((5, N))  # (column 1: b = 0 and x0 = 0, a residual that is zero in every summation order)
    mi = 25
    alone = {c: poly_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], mi)[0] for c in (0, 3)}
    for copies in (False, True):
        got = poly_solve(hp, gpu, cs, B, X0, mi, halo_copies=copies)
        lmin, lmax = hp.group_last_spectrum_poly(cs.Ms)
        for c in (0, 3):
            assert_same(got[c:c + 1], [alone[c]])
            assert got[c][1] == mi - 1 and all(np.all(np.isfinite(x)) for x in got[c][0])
        for c in (1, 2, 4):
            x, it, nr, tr = tpo.restated(A, B[c], minv, 2, lmin, lmax, mi, x0=X0[c])
            assert got[c][1] == it == 0, (c, got[c][1], it)
            assert math.isnan(got[c][2]) == math.isnan(nr) and (got[c][2] == 0.0) == (nr == 0.0), (c, got[c][2], nr)
            assert len(got[c][3]) == len(tr) == 1
            assert np.concatenate(got[c][0]).tobytes() == X0[c].tobytes()  # x untouched on every member
        assert math.isnan(got[2][2]) and math.isnan(got[4][2]) and got[1][2] == 0.0
        # ... and a following clean call is bitwise the first
        for c in (0, 3):
            assert_same(poly_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], mi), [alone[c]])


# ---------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.poly_group_lib()
    err = hp.lib().hpccg_hip_last_error
    cs = case(hp, "2x8c")
    three = case(hp, "3x33x17x9")
    n = 512
    B, X0 = columns(cs, 2)
    Bd = [dev(gpu, a) for a in cs.split(B)]
    Xd = [dev(gpu, a) for a in cs.split(X0)]
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = poly_solve(hp, gpu, cs, B, X0, 10)

    def call(Ms, ldb=(n, n), ldx=(n, n), nrhs=2, max_iter=10, nranks=2, minv=None, degree=2, lmin=0.0, lmax=0.0):
        hs = (C.c_void_p * len(Ms))(*[M.h for M in Ms])
        bp = (C.c_void_p * 2)(*[t.data_ptr() for t in Bd])
        xp = (C.c_void_p * 2)(*[t.data_ptr() for t in Xd])
        mp = None if minv is None else (C.c_void_p * 2)(*[t.data_ptr() for t in minv])
        return L.hpccg_hip_group_poly_solve_device(hs, nranks, nrhs, bp, (C.c_longlong * 2)(*ldb), xp,
                                                   (C.c_longlong * 2)(*ldx), mp, degree, lmin, lmax, max_iter, 0.0,
                                                   it, nr, None)

    def untouched():
        return all(x.cpu().numpy().tobytes() == a.tobytes() for x, a in zip(Xd, cs.split(X0)))

    dev0 = torch.cuda.current_device()
    other = hp.group_generate(8, 8, 8, 2)
    plain = hp.Matrix.generate(8, 8, 8)
    parts = []
    for r in range(2):  # (the halo mode applies to members made from CSR parts)
        prob = hp.generate_matrix(8, 8, 8, rank=r, size=2)
        parts.append(prob.to_csr() + (r * n,))
        prob.close()
    hp.set_halo_mode(2)
    try:
        gather = hp.group_from_csr(parts, 2 * n)
    finally:
        hp.set_halo_mode(0)
    assert all(M.get_option("halo_mode") == 2 for M in gather)
    try:
        assert call(gather) == EPLAN
        assert b"gather" in err()
        assert untouched()
        assert call(cs.Ms[::-1]) == EINVAL  # a member out of rank order
        assert b"rank" in err()
        assert call(three.Ms[:2]) == EINVAL  # a wrong nranks: a subset of a group
        assert b"rank" in err()
        assert call(cs.Ms, nranks=1) == EINVAL
        assert call([plain, plain]) == EINVAL  # a single-rank matrix in a 2-slot call
        assert call([cs.Ms[0], other[1]]) == EINVAL  # members of two groups
        assert b"another group" in err()
        assert untouched()
        assert call(cs.Ms, ldb=(n, n - 1)) == EINVAL
        assert b"leading dimension" in err()
        assert call(cs.Ms, ldx=(n - 1, n)) == EINVAL
        assert call(cs.Ms, nrhs=0) == EINVAL
        assert call(cs.Ms, max_iter=-1) == EINVAL
        for degree in (-1, 17):
            assert call(cs.Ms, degree=degree) == EINVAL
            assert b"degree" in err()
        # a caller's lmin against the computed lmax
        bound = hp.group_poly_bound(cs.Ms)
        for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (-1.0, 2.0), (float("nan"), 2.0), (0.5, float("inf")),
                           (bound, 0.0), (2.0 * bound, 0.0)):
            assert call(cs.Ms, lmin=lmin, lmax=lmax) == EINVAL, (lmin, lmax)
            assert b"bounds" in err()
        assert untouched()
        # a caller's m with a bad entry on the last member
        for bad in (0.0, float("nan"), -1.0, float("inf")):
            mv = [torch.ones(n, dtype=torch.float64, device=gpu) for _ in range(2)]
            mv[1][300] = bad
            mv[1][411] = bad
            assert call(cs.Ms, minv=mv) == EINVAL
            assert b"member 1's minv[300]" in err(), err()
            with pytest.raises(hp.HPCCGError, match=r"member 1's minv\[300\]"):
                hp.group_HPCCG_poly(cs.Ms, Bd, Xd, max_iter=10, minvs=mv)
            with pytest.raises(hp.HPCCGError, match=r"member 1's minv\[300\]"):
                hp.group_poly_bound(cs.Ms, mv)
            assert untouched()
        with pytest.raises(hp.HPCCGError):
            hp.group_HPCCG_poly(gather, Bd, Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError):
            hp.group_poly_bound(cs.Ms[::-1])
        with pytest.raises(hp.HPCCGError):
            hp.group_last_trace_poly(cs.Ms, 2)  # (the last solve had two columns)
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            hp.group_last_spectrum_poly(other)
        assert untouched()
        assert torch.cuda.current_device() == dev0
        # the one-rank library keeps refusing a member
        for m in cs.Ms:
            assert hp.poly_lib().hpccg_hip_poly_solve_device(m.h, 2, Bd[0].data_ptr(), n, Xd[0].data_ptr(), n, None, 2,
                                                             0.0, 0.0, 10, 0.0, it, nr, None) == EINVAL
            assert b"group" in err()
        assert untouched()
    finally:
        for M in other + gather + [plain]:
            M.close()
    # ... and a good solve afterwards
    assert_same(poly_solve(hp, gpu, cs, B, X0, 10), ref)


@pytest.mark.parametrize("shape", ["csr3", "2x8c"])
@pytest.mark.parametrize("kind", list(tpg.BAD))
def test_a_bad_diagonal_on_one_member_is_refused(hp, gpu, shape, kind):
    import torch
    A0, counts = tpg.global_matrix(shape)
    start1 = counts[0]
    rp, cols, vals = tpg._edited(A0, tpg.BAD[kind])
    A = finish(rp, cols, vals)
    Ms = tpg.members_from_csr(hp, A, counts)
    try:
        Bd = [torch.ones((2, n), dtype=torch.float64, device=gpu) for n in counts]
        Xd = [torch.full((2, n), 0.5, dtype=torch.float64, device=gpu) for n in counts]
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match=rf"\(-1\).*member 1 row {517 - start1} "):
                hp.group_HPCCG_poly(Ms, Bd, Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError, match=rf"member 1 row {517 - start1} "):
            hp.group_poly_bound(Ms)
        assert all(torch.all(x == 0.5) for x in Xd)
        # a caller's m is taken on the same members (NaN entries aside: they reach the bound)
        if kind != "nan":
            ones = [torch.ones(n, dtype=torch.float64, device=gpu) for n in counts]
            its, _, _ = hp.group_HPCCG_poly(Ms, Bd, [x.clone() for x in Xd], max_iter=3, minvs=ones)
            assert list(its) == [2, 2]
    finally:
        for M in Ms:
            M.close()


# ---------------------------------------------------------------------------
# 11. isolation
# ---------------------------------------------------------------------------
def test_other_solves_and_repeats_are_undisturbed(hp, gpu):
    cs = case(hp, "3x33x17x9")
    B, X0 = columns(cs, 4)
    prob = hp.generate_matrix(16, 16, 16)
    M1 = hp.Matrix.from_hpc(prob)
    B1, X1 = np.stack([prob.b, 0.5 * prob.b]), np.zeros((2, len(prob.b)))
    prob.close()

    def others():
        single = tpg.single_solves(hp, gpu, cs, B[:2], X0[:2], 40)
        Bd = [dev(gpu, a) for a in cs.split(B)]
        Xd = [dev(gpu, a) for a in cs.split(X0)]
        its, nrs, _ = hp.group_HPCCG_batch(cs.Ms, Bd, Xd, max_iter=40)
        gp = tpg.pcg_solve(hp, gpu, cs, B, X0, 40)
        b1, x1 = dev(gpu, B1), dev(gpu, X1)
        _, it1, nr1, _ = hp.HPCCG_pcg(M1, b1, x1, max_iter=40, device=True)
        b2, x2 = dev(gpu, B1), dev(gpu, X1)
        _, it2, nr2, _ = hp.HPCCG_poly(M1, b2, x2, max_iter=40, device=True)
        b3, x3 = dev(gpu, B1), dev(gpu, X1)
        _, it3, nr3, _ = hp.HPCCG_batch(M1, b3, x3, max_iter=40, device=True)
        return single + gp, ([x.cpu().numpy().tobytes() for x in Xd], its.tobytes(), nrs.tobytes(),
                             x1.cpu().numpy().tobytes(), it1.tobytes(), nr1.tobytes(),
                             x2.cpu().numpy().tobytes(), it2.tobytes(), nr2.tobytes(),
                             x3.cpu().numpy().tobytes(), it3.tobytes(), nr3.tobytes())

    try:
        before = others()
        counts = live(hp)
        first = poly_solve(hp, gpu, cs, B, X0, 40)
        assert live(hp) == counts
        after = others()
        assert_same(after[0], before[0])
        assert after[1] == before[1]
        for _ in range(3):
            assert_same(poly_solve(hp, gpu, cs, B, X0, 40), first)
        assert all(hp.group_poly_workspace_bytes(M) > 0 for M in cs.Ms)
        assert M1.poly_workspace_bytes() > 0 and hp.group_poly_workspace_bytes(M1) == 0
    finally:
        M1.close()
        for M in cs.Ms:
            M.batch_release()
            hp.group_pcg_release(M)


# ---------------------------------------------------------------------------
# 12. the workspace's life
# ---------------------------------------------------------------------------
def test_workspace_goes_with_the_members(hp, gpu):
    base = hp.group_poly_live_workspaces()
    others = live(hp)
    cs = tpg.Case(hp, "2x8c")
    try:
        B, X0 = columns(cs, 2)
        first = poly_solve(hp, gpu, cs, B, X0, 10)
        assert hp.group_poly_live_workspaces() == base + 2
        assert all(hp.group_poly_workspace_bytes(M) > 2 * 8 * 512 for M in cs.Ms)
        hp.group_poly_release(cs.Ms[1])
        assert hp.group_poly_live_workspaces() == base + 1 and hp.group_poly_workspace_bytes(cs.Ms[1]) == 0
        assert_same(poly_solve(hp, gpu, cs, B, X0, 10), first)  # rebuilt on demand, the caches too
        small = hp.group_poly_workspace_bytes(cs.Ms[1])
        poly_solve(hp, gpu, cs, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the caches stay
        assert hp.group_poly_workspace_bytes(cs.Ms[1]) > small
        assert_same(poly_solve(hp, gpu, cs, B, X0, 10), first)
        for M in cs.Ms:
            hp.group_poly_release(M)
            hp.group_poly_release(M)  # (idempotent)
            assert hp.group_poly_workspace_bytes(M) == 0
        assert hp.group_poly_live_workspaces() == base
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            hp.group_last_spectrum_poly(cs.Ms)
        assert_same(poly_solve(hp, gpu, cs, B, X0, 10), first)
        assert hp.group_poly_live_workspaces() == base + 2  # ... and closing the members without a release frees them
        assert first[0][1] == 9
        assert live(hp) == others
    finally:
        cs.close()
    assert hp.group_poly_live_workspaces() == base
    assert live(hp) == others
