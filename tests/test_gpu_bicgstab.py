"""Right-preconditioned BiCGStab for non-symmetric matrices
(include/hpccg_hip_bicgstab.h, lib/bicgstab/libhpccg_hip_bicgstab.so): per column the
recurrence of the header with M^-1 = diag(m), by default Jacobi m_i = 1 / a_ii;
loop test, niters, normr and trace on the 2-norm of r; a status per column.

  1. parity with the NumPy restatement (bicgstab_cases.restated_bicg) on the
     window on which the restatement agrees with itself (bicgstab_cases.window):
     niters, the r.r history within RTRANS_RTOL_1GPU, x within ten times the
     restatement's own spread under two dot orders (not below 1e-12 max |x|),
     the status; trace[0] bitwise HPCCG_pcg's;
  2. the two exact identities, bitwise: a uniform m = 2^e is m = 1; Jacobi on
     A S, S powers of two, gives s_j x'_j = x of Jacobi on A;
  3. column c of a multi-column call is bitwise its one-column call, also when
     the columns stop at different iterations; host solve = device solve;
     nothing is stored between the columns; explicit 1 / diagonal = the default;
  4. it solves what CG cannot: the 16^3 convective stencil;
  5. degenerate columns: a breakdown, an exact solve, NaN and inf in b;
  6. both nt arms give the same bits;
  7. refusals and the workspace's life.

Shapes (bicgstab_cases): the convective stencils 16^3 (8 slices), 33^3 (71
slices, two dot groups, the x-triple plan), 12x10x16 7-pt (a tail slice),
1x40x3, 1x1x1; a 16^3 stencil of distinct non-symmetric values; the 600-row
band (per-slice widths) and random CSR with 513 and 3000 rows (the int32-column
image; 513: one row in the last slice), each with its columns scaled by powers
of two.
"""
import ctypes as C
import math

import numpy as np
import pytest

import bicgstab_cases as bc
import oracle
import test_gpu_pcg as tp
from bicgstab_cases import restated_bicg
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_mixed import assert_same, columns, dev

pytestmark = pytest.mark.gpu

EINVAL = -1

_problems = {}


def problem(hp, name, A=None):
    """(Matrix, oracle.CSR with b = A 1) of a bicgstab_cases name (A: the CSR of another key)."""
    if name not in _problems:
        A = bc.csr_of(name) if A is None else A
        _problems[name] = (hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals), A)
    return _problems[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems(hp):
    yield
    for M, _ in _problems.values():
        M.close()
    _problems.clear()
    assert hp.bicgstab_live_workspaces() == 0


def bicg_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, minv=None, ld=None):
    """[(x, niters, normr, trace, status)] per column of a device solve; minv:
    None (Jacobi), a number (that value everywhere) or an array."""
    import torch
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    if minv is not None:
        minv = torch.from_numpy(np.full(n, 1.0) * np.float64(minv)).to(gpu)
    ierr, its, nrs, times = hp.HPCCG_bicgstab(M, Bd, Xd, max_iter=max_iter, tolerance=tol, minv=minv, device=True)
    assert ierr == 0 and times[0] > 0.0 and not times[1:].any()
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_bicgstab(c).copy(), M.last_status_bicgstab(c))
            for c in range(B.shape[0])]


def same(got, ref):
    """assert_same, and the statuses."""
    assert_same(got, ref)
    assert [g[4] for g in got] == [r[4] for r in ref]


def kind_minv(kind):
    return 1.0 if kind == "one" else None


def test_every_image_form_is_exercised(hp, gpu):
    forms = {}
    for name in bc.TABLE:
        M, _ = problem(hp, name)
        forms[name] = (M.get_option("has_a"), M.get_option("a_width") if M.get_option("has_a") else None)
    assert forms["33c"] == (1, 27) and forms["16c"] == (1, 27) and forms["dominant16"] == (1, 27), forms
    assert forms["12x10x16_7pt"] == (1, 7) and forms["band600s"] == (1, 0), forms
    assert forms["csr513s"] == (0, None) and forms["csr3000s"] == (0, None), forms


# ---------------------------------------------------------------------------
# 1. parity with the restatement on its window
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bc.MKINDS)
@pytest.mark.parametrize("name", bc.TABLE)
def test_parity_with_the_restatement(hp, gpu, name, kind):
    M, A = problem(hp, name)
    m = bc.minv_of(A, kind)
    B, X0 = columns(A.b, A.xexact, 4)
    # the window every running column has (column 2 starts at the solution and runs nothing)
    wins = [bc.window(name, kind, B[c], X0[c], key=c) for c in range(4)]
    running = [c for c in range(4) if wins[c][2][4][0] != 0.0]
    assert 0 in running and (2 not in running or A.nrow == 1), running
    W = min(wins[c][0] for c in running)
    assert W >= 1
    got = bicg_solve(hp, gpu, M, B, X0, W + 1, minv=kind_minv(kind))
    pcg = tp.pcg_solve(hp, gpu, M, B, X0, 1, minv=kind_minv(kind))
    for c in range(4):
        ref = restated_bicg(A, B[c], m, W + 1, x0=X0[c])
        blk = restated_bicg(A, B[c], m, W + 1, x0=X0[c], dot=bc.blocked_dot)
        x, it, nr, tr, status = got[c]
        assert it == ref[1] and status == ref[5], (c, it, ref[1], status, ref[5])
        assert len(tr) == it + 1 and nr == tr[-1]
        checked = check_trace(tr, ref[3], RTRANS_RTOL_1GPU)
        spread = float(np.max(np.abs(ref[0] - blk[0])))
        bar = max(10.0 * spread, 1e-12 * float(np.max(np.abs(ref[0]))))
        err = float(np.max(np.abs(x - ref[0])))
        print(f"{name}/{kind} column {c}: W {W} niters {it} status {status}, {checked} history points, "
              f"|x - ref| {err:.3e}, the restatement's spread {spread:.3e}")
        assert err <= bar, (c, err, bar)
        assert tr[0].tobytes() == pcg[c][3][0].tobytes(), (c, tr[0], pcg[c][3][0])
    M.pcg_release()


# ---------------------------------------------------------------------------
# 2. the two exact identities
# ---------------------------------------------------------------------------
IDENT = ["16c", "12x10x16_7pt", "band600s", "csr513s"]


@pytest.mark.parametrize("name", IDENT)
def test_a_uniform_power_of_two_m_is_m_one(hp, gpu, name):
    M, A = problem(hp, name)
    B, X0 = columns(A.b, A.xexact, 4)
    # a tolerance that column 0 meets part-way: just above the smallest residual of its first half
    tr0 = bicg_solve(hp, gpu, M, B[:1], X0[:1], 25, minv=1.0)[0][3]
    tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10)
    for max_iter, t in ((25, 0.0), (25, tol), (2, 0.0)):
        ref = bicg_solve(hp, gpu, M, B, X0, max_iter, t, minv=1.0)
        assert ref[0][1] >= 1 and (t == 0.0 or ref[0][1] < 24), ref[0][1]
        for m in (2.0 ** -3, 2.0 ** 5):
            same(bicg_solve(hp, gpu, M, B, X0, max_iter, t, minv=m), ref)
            same(bicg_solve(hp, gpu, M, B[:1], X0[:1], max_iter, t, minv=m), ref[:1])


@pytest.mark.parametrize("name", IDENT)
def test_jacobi_commutes_with_a_power_of_two_column_scaling(hp, gpu, name):
    A0, As, s = bc.scaled_pair(name)
    M0, _ = problem(hp, "pair0_" + name, A0)
    Ms, _ = problem(hp, "pairs_" + name, As)
    n = A0.nrow
    rng = np.random.default_rng(3)
    B = np.stack([A0.b, rng.uniform(-1.0, 1.0, n), A0.b * 2.0 ** -7, rng.uniform(-1.0, 1.0, n)])
    X0 = np.zeros((4, n))
    for nrhs in (4, 1, 2):
        got = bicg_solve(hp, gpu, M0, B[:nrhs], X0[:nrhs], 12)
        gots = bicg_solve(hp, gpu, Ms, B[:nrhs], X0[:nrhs], 12)
        for c in range(nrhs):
            assert got[c][1] == 11 and np.all(np.isfinite(got[c][0])) and got[c][0].any()
            same([(gots[c][0] * s,) + gots[c][1:]], [got[c]])


# ---------------------------------------------------------------------------
# 3. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33c", "csr513s", "12x10x16_7pt"])
def test_columns_are_single_column_calls(hp, gpu, name):
    M, A = problem(hp, name)
    n = A.nrow
    rng = np.random.default_rng(9)
    B = np.stack([A.b, A.b * 2.0 ** -20, rng.uniform(-1.0, 1.0, n) * 2.0 ** 10, A.b * 2.0 ** -40, A.b])
    X0 = np.zeros((5, n))
    X0[4] = A.xexact  # (ends before its first iteration)
    one = [bicg_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 30)[0] for c in range(5)]
    for nrhs, ld in ((5, n + 5), (3, n)):
        same(bicg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 30, ld=ld), one[:nrhs])
    # a tolerance between two consecutive residuals of column 0 (test_gpu_fuzz's rule: never within
    # rounding of either), which the differently scaled columns meet at other iterations
    tr = one[0][3]
    above = int(np.sum(np.minimum.accumulate(tr) >= 1e-9 * tr[0]))
    j = next(j for j in range(max(1, above // 2), len(tr) - 1) if 1e-8 * tr[j] < tr[j + 1] < 0.9 * tr[j])
    tol = float(np.sqrt(tr[j] * tr[j + 1]))
    one = [bicg_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 30, tol)[0] for c in range(5)]
    stops = [o[1] for o in one]
    print(f"{name}: tolerance after residual {j}, stops {stops}")
    assert stops[0] < 29 and len(set(stops)) >= 3 and stops[4] == 0, stops
    for nrhs, ld in ((5, n), (3, n + 3)):
        got = bicg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 30, tol, ld=ld)
        same(got, one[:nrhs])
        for g in got:
            assert len(g[3]) == g[1] + 1 and g[2] == g[3][-1]


@pytest.mark.parametrize("name", ["33c", "csr513s", "band600s"])
def test_host_solve_and_explicit_jacobi_are_the_device_solve(hp, gpu, name):
    M, A = problem(hp, name)
    B, X0 = columns(A.b, A.xexact, 3)
    ref = bicg_solve(hp, gpu, M, B, X0, 15)

    def host(**kw):
        X = X0.copy()
        ierr, its, nrs, times = hp.HPCCG_bicgstab(M, B, X, max_iter=15, **kw)
        assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
        return [(X[c], int(its[c]), float(nrs[c]), M.last_trace_bicgstab(c).copy(), M.last_status_bicgstab(c))
                for c in range(3)]

    same(host(), ref)
    minv = 1.0 / tp.csr_diagonal(A)
    same(bicg_solve(hp, gpu, M, B, X0, 15, minv=minv), ref)
    same(host(minv=minv), ref)
    # one column as a vector, updated in place
    x = X0[1].copy()
    hp.HPCCG_bicgstab(M, B[1].copy(), x, max_iter=15)
    assert x.tobytes() == bicg_solve(hp, gpu, M, B[1:2], X0[1:2], 15)[0][0].tobytes()


# ---------------------------------------------------------------------------
# 4. it solves what CG cannot
# ---------------------------------------------------------------------------
def test_it_solves_the_convective_stencil_cg_cannot(hp, gpu):
    M, A = problem(hp, "16c")
    n = A.nrow
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    x, it, nr, tr, status = bicg_solve(hp, gpu, M, B, X0, 60, 1e-9 * r0)[0]
    res = float(np.linalg.norm(A.b - oracle.sparsemv(A, x)))
    err = float(np.max(np.abs(x - 1.0)))
    px, pit, pnr, ptr = tp.pcg_solve(hp, gpu, M, B, X0, 150)[0]
    print(f"16c convective: BiCGStab {it} iterations, status {status}, |b - A x| / r0 {res / r0:.3e}, "
          f"max |x - 1| {err:.3e}; pcg {pit} iterations, normr / r0 {pnr / r0:.3e}")
    assert status == 0 and it <= 40, (status, it)
    assert res <= 1e-8 * r0 and err <= 1e-8, (res / r0, err)
    assert pit == 149 and pnr > 0.1 * r0, (pit, pnr / r0)
    M.pcg_release()


# ---------------------------------------------------------------------------
# 5. degenerate columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bc.MKINDS)
def test_a_breakdown_freezes_its_column_alone(hp, gpu, kind):
    M, A = problem(hp, "breakdown")
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 4)
    B[2], X0[2] = 0.0, 0.0
    B[2, :2] = (1.0, -1.0)  # rhat.v = 0.0 at k = 1, and the stencil's rows at rest
    got = bicg_solve(hp, gpu, M, B, X0, 20, minv=kind_minv(kind))
    x, it, nr, tr, status = got[2]
    assert (it, status) == (0, 1) and not x.any() and len(tr) == 1 and nr == math.sqrt(2.0), (it, status, nr)
    ref = restated_bicg(A, B[2], bc.minv_of(A, kind), 20)
    assert (ref[1], ref[5]) == (0, 1)
    keep = [0, 1, 3]
    assert [got[c][4] for c in keep] == [0, 0, 0] and [got[c][1] for c in keep] == [19, 19, 19]
    same([got[c] for c in keep], bicg_solve(hp, gpu, M, B[keep], X0[keep], 20, minv=kind_minv(kind)))
    same(got[2:3], bicg_solve(hp, gpu, M, B[2:3], X0[2:3], 20, minv=kind_minv(kind)))


def test_one_row_is_solved_exactly(hp, gpu):
    M, A = problem(hp, "1x1x1")
    for kind in bc.MKINDS:
        ref = restated_bicg(A, A.b, bc.minv_of(A, kind), 500)
        x, it, nr, tr, status = bicg_solve(hp, gpu, M, A.b.reshape(1, 1), np.zeros((1, 1)), 500, minv=kind_minv(kind))[0]
        assert status == 2 == ref[5] and it == ref[1], (status, it, ref[1], ref[5])
        assert x.tobytes() == ref[0].tobytes() and np.isfinite(x).all(), (x, ref[0])  # (one row: every dot is one product)


@pytest.mark.parametrize("name", ["16c", "csr513s"])
def test_non_finite_columns_end_by_the_lagged_test(hp, gpu, name):
    M, A = problem(hp, name)
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 4)
    B[1, n // 2] = np.nan
    B[3, n // 3] = np.inf
    good = [0, 2]
    for kind in bc.MKINDS:
        got = bicg_solve(hp, gpu, M, B, X0, 12, minv=kind_minv(kind))
        for c in (1, 3):
            ref = restated_bicg(A, B[c], bc.minv_of(A, kind), 12, x0=X0[c])
            x, it, nr, tr, status = got[c]
            assert (it, status) == (ref[1], ref[5]) == ((0, 0) if c == 1 else (2, 0)), (c, it, status, ref[1], ref[5])
            assert math.isnan(nr) and math.isnan(ref[2])
            if c == 1:
                assert x.tobytes() == X0[c].tobytes()  # untouched
            else:
                assert np.isnan(x).all()
        same([got[c] for c in good], bicg_solve(hp, gpu, M, B[good], X0[good], 12, minv=kind_minv(kind)))
        # nothing of a bad column stays in the workspace
        same(bicg_solve(hp, gpu, M, B[good], X0[good], 12, minv=kind_minv(kind)), [got[c] for c in good])


# ---------------------------------------------------------------------------
# 6. both nt arms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16c", "12x10x16_7pt"])
def test_both_nt_arms_give_the_same_bits(hp, gpu, name):
    M, A = problem(hp, name)
    n = A.nrow
    rng = np.random.default_rng(6)
    B = rng.uniform(-1.0, 1.0, (5, n))  # every column runs to max_iter: a full chunk takes the nt arm
    B[0] = A.b
    X0 = np.zeros((5, n))
    X0[1] = 0.25 * ((np.arange(n) % 7) - 3)

    def run():
        out = []
        for nrhs, ld in ((5, n), (4, n + 3), (2, n), (1, n)):
            for minv in (None, 1.0):
                out += bicg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 12, minv=minv, ld=ld)
        assert all(o[1] == 11 for o in out)
        return out

    assert M.get_option("nt") == 0
    ref = run()
    try:
        M.set_option("nt", 1)
        assert M.get_option("nt") == 1
        got = run()
    finally:
        M.set_option("nt", -1)
    assert M.get_option("nt") == 0
    same(got, ref)
    same(run(), ref)  # nothing of the forced run stays


# ---------------------------------------------------------------------------
# 7. refusals, the workspace
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
            with pytest.raises(hp.HPCCGError, match=rf"bicgstab: .*row {row} "):
                hp.HPCCG_bicgstab(M, Bd, Xd, max_iter=10, device=True)
        assert torch.all(Xd == 0.5)
        # a caller's m is taken on the same matrix
        assert hp.HPCCG_bicgstab(M, Bd, Xd.clone(), max_iter=3, minv=torch.ones(n, dtype=torch.float64, device=gpu),
                                 device=True)[0] == 0
    finally:
        M.close()


def test_refusals_leave_the_process_working(hp, gpu):
    L = hp.bicgstab_lib()
    M, A = problem(hp, "16c")
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = bicg_solve(hp, gpu, M, B, X0, 10)

    def call(h, nrhs=2, ldb=n, ldx=n, minv=None, max_iter=10):
        return L.hpccg_hip_bicgstab_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, minv, max_iter, 0.0,
                                                 it, nr, None)

    err = hp.lib().hpccg_hip_last_error
    assert call(M.h, ldb=n - 1) == EINVAL
    assert b"leading dimension" in err() and err().startswith(b"bicgstab:")
    assert call(M.h, ldx=n - 1) == EINVAL
    assert call(M.h, max_iter=-1) == EINVAL
    assert call(M.h, nrhs=0) == EINVAL
    assert call(None) == EINVAL
    with pytest.raises(hp.HPCCGError, match=r"bicgstab: minv\[700\]"):
        mv = np.ones(n)
        mv[700] = 0.0
        hp.HPCCG_bicgstab(M, B.copy(), X0.copy(), max_iter=10, minv=mv)
    assert Xd.cpu().numpy().tobytes() == X0.tobytes()  # nothing was touched
    with pytest.raises(hp.HPCCGError, match="no status of column 2"):
        M.last_status_bicgstab(2)
    # max_iter 0 and 1: the prologue only
    for max_iter in (0, 1):
        for x, its, nrm, tr, status in bicg_solve(hp, gpu, M, B, X0, max_iter):
            assert (its, status, len(tr)) == (0, 0, 1) and nrm == tr[0]
        got = bicg_solve(hp, gpu, M, B, X0, max_iter)
        assert got[0][0].tobytes() == X0[0].tobytes() and got[1][0].tobytes() == X0[1].tobytes()
        assert got[0][3][0].tobytes() == ref[0][3][0].tobytes()
    # ... and a good solve afterwards
    same(bicg_solve(hp, gpu, M, B, X0, 10), ref)


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.bicgstab_live_workspaces()
    A = bc.csr_of("12x10x16_7pt")
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    M2 = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    try:
        B, X0 = columns(A.b, A.xexact, 2)
        first = bicg_solve(hp, gpu, M, B, X0, 10)
        bicg_solve(hp, gpu, M2, B, X0, 10)
        assert hp.bicgstab_live_workspaces() == base + 2
        assert M2.bicgstab_workspace_bytes() > 2 * 8 * 8 * A.nrow  # eight vectors per column
        M2.bicgstab_release()
        assert hp.bicgstab_live_workspaces() == base + 1 and M2.bicgstab_workspace_bytes() == 0
        same(bicg_solve(hp, gpu, M2, B, X0, 10), first)  # rebuilt on demand, the Jacobi cache too
        small = M2.bicgstab_workspace_bytes()
        bicg_solve(hp, gpu, M2, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows
        grown = M2.bicgstab_workspace_bytes()
        assert grown > small
        same(bicg_solve(hp, gpu, M2, B, X0, 10), first)
        assert M2.bicgstab_workspace_bytes() == grown  # ... and is kept
        M2.bicgstab_release()
        M2.bicgstab_release()  # (idempotent)
        assert hp.bicgstab_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()
        M2.close()
    assert hp.bicgstab_live_workspaces() == base
