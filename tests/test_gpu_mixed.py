"""Mixed-precision CG (include/hpccg_hip_mixed.h, lib/libhpccg_hip_mixed.so):
the matrix values streamed from an fp32 image, everything else fp64.

  * the SpMM over the fp32 image is bitwise the CPU oracle's SpMV on the CSR
    whose values went through np.float32, on every shape;
  * on a matrix whose values are exact in fp32 the solve is bitwise the fp64
    single solve of each column: x, niters, normr, trace;
  * on any other matrix the refinement reaches the fp64 residual that the fp32
    operator alone cannot (the control), within twice the fp64 solve's
    iterations and 2 to 4 sweeps;
  * every column of a multi-column call is bitwise the single-column call.

Shapes: the stencils of test_gpu_batch.py (16^3, 33^3 with 71 slices and a
partial last one, 12x10x16 7-pt, 1x1x1, 1x40x3), random SPD CSR with n = 1,
513, 3000 in a dyadic (fp32-exact) and a plain (inexact) form (entries in
random order: the int32-column image), a 600-row band with ascending columns
(SELL-512-A with per-slice widths), and 16^3 27-pt / 12x10x16 7-pt with every
entry scaled by a symmetric random factor (SELL-512-A, inexact).
"""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

EINVAL = -1


# ---------------------------------------------------------------------------
# problems: name -> (Matrix, oracle.CSR with b = A xexact, xexact)
# ---------------------------------------------------------------------------
def random_spd(rng, n, per_row, band, dyadic):
    """Symmetric, strictly diagonally dominant (so SPD), the entries of each
    row in random order, b = A 1. dyadic: every off-diagonal and the diagonal's
    extra term are multiples of 2^-10, so every value and b are exact in fp32;
    otherwise uniform values, inexact."""
    def q(v):
        return round(v * 1024.0) / 1024.0 if dyadic else v
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for _ in range(int(rng.integers(0, per_row + 1))):
            j = int(i + rng.integers(-band, band + 1)) if band else int(rng.integers(0, n))
            if 0 <= j < n and j != i:
                v = -q(float(rng.uniform(0.05, 1.0)))
                rows[i][j] = v
                rows[j][i] = v
    row_ptr = np.zeros(n + 1, np.int64)
    cols, vals = [], []
    for i in range(n):
        d = rows[i]
        ent = list(d.items()) + [(i, sum(-v for v in d.values()) + q(float(rng.uniform(0.5, 2.0))))]
        for k in rng.permutation(len(ent)):
            cols.append(ent[k][0])
            vals.append(ent[k][1])
        row_ptr[i + 1] = len(cols)
    return finish(row_ptr, cols, vals)


def finish(row_ptr, cols, vals):
    n = len(row_ptr) - 1
    A = oracle.CSR(np.asarray(row_ptr, np.int64), np.asarray(cols, np.int32), np.asarray(vals, np.float64),
                   np.zeros(n), np.zeros(n), np.ones(n))
    A.b = oracle.sparsemv(A, np.ones(n))
    return A


def band600():
    """600 rows, tridiagonal, with a further +-7 pair among the rows from 512
    on: ascending columns, slice 0 three slots wide and slice 1 five."""
    n = 600
    row_ptr, cols, vals = [0], [], []
    for i in range(n):
        for j, v in ((i - 7, -0.25), (i - 1, -1.0), (i, 4.0), (i + 1, -1.0), (i + 7, -0.25)):
            if 0 <= j < n and (abs(j - i) != 7 or min(i, j) >= 512):
                cols.append(j)
                vals.append(v)
        row_ptr.append(len(cols))
    return finish(row_ptr, cols, vals)


def perturbed(nx, ny, nz, s7, seed):
    """The stencil with every entry scaled by a symmetric random factor in
    [0.5, 1.5) (one factor per unordered index pair)."""
    G = oracle.generate(nx, ny, nz, use_7pt=s7)
    n = G.nrow
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(G.row_ptr))
    c = G.cols.astype(np.int64)
    key = np.minimum(rows, c) * n + np.maximum(rows, c)
    uniq, inv = np.unique(key, return_inverse=True)
    f = np.random.default_rng(seed).uniform(0.5, 1.5, len(uniq))
    return finish(G.row_ptr, G.cols, G.vals * f[inv])


STENCILS = {
    "16c": (16, 16, 16, False),
    "33c": (33, 33, 33, False),
    "12x10x16_7pt": (12, 10, 16, True),
    "1x1x1": (1, 1, 1, False),
    "1x40x3": (1, 40, 3, False),
}
CSRS = {"csr1": (1, 0, 0, 11), "csr513": (513, 6, 40, 12), "csr3000": (3000, 9, 0, 13)}
DYADIC = ["dyadic_" + k for k in CSRS]
PLAIN = ["plain_" + k for k in CSRS]
EXACT = list(STENCILS) + DYADIC + ["band600"]
INEXACT = ["plain_csr513", "plain_csr3000", "pert_16c", "pert_12x10x16_7pt"]
ALL = EXACT + ["plain_csr1"] + INEXACT

_problems = {}


def problem(hp, name):
    if name not in _problems:
        if name in STENCILS:
            nx, ny, nz, s7 = STENCILS[name]
            A = oracle.generate(nx, ny, nz, use_7pt=s7)
            prob = hp.generate_matrix(nx, ny, nz, use_7pt=s7)
            M = hp.Matrix.from_hpc(prob)
            prob.close()
        else:
            if name == "band600":
                A = band600()
            elif name.startswith("pert_"):
                nx, ny, nz, s7 = STENCILS[name[5:]]
                A = perturbed(nx, ny, nz, s7, 31)
            else:
                form, key = name.split("_")
                n, per_row, band, seed = CSRS[key]
                A = random_spd(np.random.default_rng(seed), n, per_row, band, form == "dyadic")
            M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
        _problems[name] = (M, A, A.xexact.copy())
    return _problems[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems(hp):
    yield
    for M, _, _ in _problems.values():
        M.close()
    _problems.clear()
    assert hp.mixed_live_workspaces() == 0


def columns(b, xexact, nrhs, seed=5):
    """The right-hand sides and initial guesses of test_gpu_batch.columns:
    the generated b; a scaled b with a nonzero x0; x0 = xexact (an exactly zero
    residual); random columns."""
    n = len(b)
    g = np.arange(n)
    rng = np.random.default_rng(seed)
    B = np.zeros((nrhs, n))
    X0 = np.zeros((nrhs, n))
    for c in range(nrhs):
        if c == 0:
            B[c] = b
        elif c == 1:
            B[c] = b * 2.0 ** -3
            X0[c] = 0.25 * ((g % 7) - 3)
        elif c == 2:
            B[c] = b
            X0[c] = xexact
        else:
            B[c] = rng.uniform(-1.0, 1.0, n)
    return B, X0


def dev(gpu, a, ld=None):
    """(nrhs, n) host columns on the device with leading dimension ld."""
    import torch
    nrhs, n = a.shape
    t = torch.full((nrhs, max(ld or n, 1)), 7.5, dtype=torch.float64, device=gpu)
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t


def single_solves(hp, gpu, M, B, X0, max_iter, tol=0.0):
    """The fp64 reference: every column solved alone on the device."""
    import torch
    out = []
    for c in range(B.shape[0]):
        b = torch.from_numpy(B[c].copy()).to(gpu)
        x = torch.from_numpy(X0[c].copy()).to(gpu)
        ierr, it, nr, _ = hp.HPCCG(M, b, x, max_iter=max_iter, tolerance=tol, device=True)
        assert ierr == 0
        out.append((x.cpu().numpy(), it, nr, M.last_trace().copy()))
    return out


def mixed_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, ld=None, **kw):
    """[(x, niters, normr, trace, (sweep iters, sweep residuals))] per column."""
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    ierr, its, nrs, times = hp.HPCCG_mixed(M, Bd, Xd, max_iter=max_iter, tolerance=tol, device=True, **kw)
    assert ierr == 0
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_mixed(c).copy(), M.last_sweeps_mixed(c))
            for c in range(B.shape[0])]


def assert_same(got, ref, sweeps=False):
    assert len(got) == len(ref)
    for c, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == r[1], (c, g[1], r[1])
        assert np.float64(g[2]).tobytes() == np.float64(r[2]).tobytes(), (c, g[2], r[2])
        assert g[3].tobytes() == r[3].tobytes(), (c, "trace")
        assert g[0].tobytes() == r[0].tobytes(), (c, "x", float(np.max(np.abs(g[0] - r[0]))))
        if sweeps:
            assert g[4][0].tobytes() == r[4][0].tobytes() and g[4][1].tobytes() == r[4][1].tobytes(), (c, g[4], r[4])


def test_every_image_form_is_exercised(hp, gpu):
    """Widths 27, 7, per-slice (0) of SELL-512-A and the SELL-512 form."""
    forms = {}
    for name in ALL:
        M, _, _ = problem(hp, name)
        forms[name] = (M.get_option("has_a"), M.get_option("a_width") if M.get_option("has_a") else None)
    assert forms["33c"] == (1, 27) and forms["pert_16c"] == (1, 27), forms
    assert forms["12x10x16_7pt"] == (1, 7) and forms["pert_12x10x16_7pt"] == (1, 7), forms
    assert forms["band600"] == (1, 0), forms
    for name in DYADIC[1:] + PLAIN[1:]:
        assert forms[name] == (0, None), forms
    for name in EXACT:
        assert problem(hp, name)[0].mixed_info()["exact"] == 1, name
    for name in INEXACT:
        info = problem(hp, name)[0].mixed_info()
        assert info["exact"] == 0 and info["inexact_values"] > 0, (name, info)


# ---------------------------------------------------------------------------
# 1. SpMV
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3], ids=["ld_n", "ld_n3"])
@pytest.mark.parametrize("shape", ALL)
def test_spmm_is_the_oracle_on_the_fp32_values(hp, gpu, shape, pad):
    import torch
    M, A, _ = problem(hp, shape)
    n = A.nrow
    A32 = oracle.CSR(A.row_ptr, A.cols, A.vals.astype(np.float32).astype(np.float64), None, None, None)
    exact = bool(np.all(A32.vals == A.vals))
    assert exact == (shape in EXACT)
    rng = np.random.default_rng(21)
    V = rng.uniform(-1.0, 1.0, (5, n))
    ref = [oracle.sparsemv(A32, V[c]) for c in range(5)]
    for nrhs in (1, 2, 3, 5):
        Xd = dev(gpu, V[:nrhs], n + pad)
        Yd = torch.full((nrhs, n + pad), -3.0, dtype=torch.float64, device=gpu)
        hp.HPC_sparsemv_mixed(M, Xd, Yd)
        Y = Yd.cpu().numpy()
        for c in range(nrhs):
            assert Y[c, :n].tobytes() == ref[c].tobytes(), (nrhs, c, float(np.max(np.abs(Y[c, :n] - ref[c]))))
        assert np.all(Y[:, n:] == -3.0)
    if exact:
        for c in range(2):
            y = torch.zeros(n, dtype=torch.float64, device=gpu)
            hp.HPC_sparsemv(M, torch.from_numpy(V[c].copy()).to(gpu), y)
            assert y.cpu().numpy().tobytes() == ref[c].tobytes(), c


# ---------------------------------------------------------------------------
# 2. an exact matrix: the fp64 solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EXACT)
def test_exact_solve_is_the_fp64_single_solve(hp, gpu, shape):
    M, A, xexact = problem(hp, shape)
    n = A.nrow
    B, X0 = columns(A.b, xexact, 5)
    assert M.mixed_info()["exact"] == 1
    for max_iter in (0, 1, 2, 60):
        ref = single_solves(hp, gpu, M, B, X0, max_iter)
        assert ref[2][1] == 0  # column 2 ends before its first iteration
        if max_iter > 1 and n > 1:
            assert ref[0][1] > 0  # ... while the others run
        for nrhs, ld in ((5, n), (3, n + 3), (2, n), (1, n)):
            # (max_sweeps and inner_rtol are ignored)
            got = mixed_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], max_iter, ld=ld, max_sweeps=1 + nrhs % 2,
                              inner_rtol=0.5 if nrhs == 2 else -1.0)
            assert_same(got, ref[:nrhs])
            for c in range(nrhs):
                its, res = got[c][4]
                assert list(its) == [got[c][1]] and len(res) == 2  # one sweep
                assert res[1] == got[c][2] and res[0] == got[c][3][0]


def test_exact_columns_stop_at_their_own_iteration(hp, gpu):
    M, A, _ = problem(hp, "16c")
    n = A.nrow
    rng = np.random.default_rng(9)
    # the same tolerance meets differently scaled residuals at different iterations
    B = np.stack([A.b, A.b * 2.0 ** -20, rng.uniform(-1.0, 1.0, n) * 2.0 ** 10, A.b * 2.0 ** -40])
    X0 = np.zeros((4, n))
    tol = 1e-6
    ref = single_solves(hp, gpu, M, B, X0, 150, tol)
    stops = [r[1] for r in ref]
    assert len(set(stops)) >= 2 and min(stops) < 149, stops
    for nrhs in (4, 3, 1):
        assert_same(mixed_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 150, tol), ref[:nrhs])


def test_one_column_as_a_vector(hp, gpu):
    """1-D b and x are one column, x updated in place (device and host)."""
    import torch
    M, A, _ = problem(hp, "16c")
    n = A.nrow
    ref = single_solves(hp, gpu, M, A.b.reshape(1, n), np.zeros((1, n)), 30)[0]
    x = torch.zeros(n, dtype=torch.float64, device=gpu)
    ierr, its, nrs, _ = hp.HPCCG_mixed(M, torch.from_numpy(A.b.copy()).to(gpu), x, max_iter=30, device=True)
    assert ierr == 0 and int(its[0]) == ref[1] and x.cpu().numpy().tobytes() == ref[0].tobytes()
    xh = np.zeros(n)
    hp.HPCCG_mixed(M, A.b.copy(), xh, max_iter=30)
    assert xh.tobytes() == ref[0].tobytes()
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_mixed(M, A.b.copy(), np.zeros(2 * n)[::2], max_iter=30)


@pytest.mark.parametrize("shape", ["33c", "plain_csr513"])
def test_host_solve_is_device_solve(hp, gpu, shape):
    M, A, xexact = problem(hp, shape)
    B, X0 = columns(A.b, xexact, 3)
    tol = 0.0 if shape in EXACT else 1e-12 * float(np.linalg.norm(A.b))
    ref = mixed_solve(hp, gpu, M, B, X0, 25 if shape in EXACT else 4000, tol)
    X = X0.copy()
    ierr, its, nrs, times = hp.HPCCG_mixed(M, B, X, max_iter=25 if shape in EXACT else 4000, tolerance=tol)
    assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
    got = [(X[c], int(its[c]), float(nrs[c]), M.last_trace_mixed(c).copy(), M.last_sweeps_mixed(c)) for c in range(3)]
    assert_same(got, ref, sweeps=True)


# ---------------------------------------------------------------------------
# 3. any other matrix: the refinement reaches the fp64 residual
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", INEXACT)
def test_refinement_reaches_the_fp64_residual(hp, gpu, shape):
    """Bounds from the issue's CPU restatement of the algorithm on matrices of
    these families: 2 sweeps, final residuals 1-4e-13 ||b||, inner iterations
    within 1.43x of the fp64 solve's; the fp32 operator alone stalls at 3e-8 to
    1.2e-7 ||b||."""
    M, A, xexact = problem(hp, shape)
    n = A.nrow
    bnorm = float(np.linalg.norm(A.b))
    tol = 1e-12 * bnorm
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    assert M.mixed_info()["exact"] == 0
    fp64 = single_solves(hp, gpu, M, B, X0, 4000, tol)[0]
    x, niters, normr, trace, (its, res) = mixed_solve(hp, gpu, M, B, X0, 4000, tol)[0]
    host_res = float(np.linalg.norm(A.b - oracle.sparsemv(A, x)))
    print(f"{shape}: sweeps {list(its)} residuals {[float(r) / bnorm for r in res]} niters {niters} "
          f"(fp64 {fp64[1]}) host residual {host_res / bnorm:.3e}")
    assert normr <= tol, (normr, tol)
    assert host_res <= 2.0 * tol, (host_res, tol)
    assert 2 <= len(its) <= 4, its
    assert niters <= 2 * fp64[1], (niters, fp64[1])
    # the sweeps' record is consistent
    assert int(its.sum()) == niters and len(res) == len(its) + 1
    assert np.all(res[1:] < res[:-1]), res
    assert np.float64(res[-1]).tobytes() == np.float64(normr).tobytes()
    assert len(trace) == niters + len(its)
    # control: without the fp64 residual steps the fp32 operator does not get there
    _, nit1, normr1, _, (its1, res1) = mixed_solve(hp, gpu, M, B, X0, 4000, tol, max_sweeps=1, inner_rtol=0.0)[0]
    print(f"{shape}: control normr {normr1 / bnorm:.3e} after {nit1}")
    assert len(its1) == 1 and normr1 > 1e-9 * bnorm, (normr1, bnorm)


# ---------------------------------------------------------------------------
# 4. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["plain_csr3000", "pert_16c"])
def test_refined_columns_are_single_column_calls(hp, gpu, shape):
    M, A, xexact = problem(hp, shape)
    n = A.nrow
    tol = 1e-12 * float(np.linalg.norm(A.b))
    # zero sweeps (x0 = xexact: b = A 1 is the SpMV's own sum) | the full solve |
    # a b so small that the first sweep's inner target is the tolerance itself
    B = np.stack([A.b, A.b, A.b * 2.0 ** -30])
    X0 = np.stack([xexact, np.zeros(n), np.zeros(n)])
    got = mixed_solve(hp, gpu, M, B, X0, 4000, tol, ld=n + 5)
    sweeps = [len(g[4][0]) for g in got]
    assert sweeps[0] == 0 and got[0][1] == 0 and got[0][2] == 0.0 and len(got[0][3]) == 0, got[0][1:]
    assert sweeps[1] >= 2 and len(set(sweeps)) >= 2, sweeps
    assert got[2][1] < got[1][1]
    for c in range(3):
        assert got[c][2] <= tol
        assert_same(got[c:c + 1], mixed_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 4000, tol), sweeps=True)
    # ... and whatever the budget: columns that run out of iterations or sweeps
    for kw in (dict(max_iter=20), dict(max_iter=4000, max_sweeps=1), dict(max_iter=1)):
        it = kw.pop("max_iter")
        got = mixed_solve(hp, gpu, M, B, X0, it, tol, **kw)
        assert all(g[1] <= max(it, 1) - 1 for g in got)
        for c in range(3):
            assert_same(got[c:c + 1], mixed_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], it, tol, **kw), sweeps=True)


# ---------------------------------------------------------------------------
# 5. values outside fp32 range
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
        Yd = torch.full((2, 3), -3.0, dtype=torch.float64, device=gpu)
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match="fp32 range"):
                hp.HPCCG_mixed(M, Bd, Xd, max_iter=10, device=True)
            with pytest.raises(hp.HPCCGError, match="fp32 range"):
                hp.HPC_sparsemv_mixed(M, Xd, Yd)
            with pytest.raises(hp.HPCCGError, match="fp32 range"):
                M.mixed_info()
        it = (C.c_int * 2)()
        nr = (C.c_double * 2)()
        assert hp.mixed_lib().hpccg_hip_mixed_solve_device(M.h, 2, Bd.data_ptr(), 3, Xd.data_ptr(), 3, 10, 0.0, 8, -1.0,
                                                           it, nr, None) == EINVAL
        assert torch.all(Xd == 0.5) and torch.all(Yd == -3.0)
        # the fp64 solve takes the matrix as it is
        assert hp.HPCCG(M, Bd[0], Xd[0].clone(), max_iter=5, device=True)[0] == 0
    finally:
        M.close()
    # ... and a good matrix afterwards
    G, A, xexact = problem(hp, "16c")
    B, X0 = columns(A.b, xexact, 2)
    assert_same(mixed_solve(hp, gpu, G, B, X0, 10), single_solves(hp, gpu, G, B, X0, 10))


# ---------------------------------------------------------------------------
# 6. lifecycle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["33c", "pert_16c"])
def test_other_solves_and_repeats_are_undisturbed(hp, gpu, shape):
    M, A, xexact = problem(hp, shape)
    B, X0 = columns(A.b, xexact, 3)
    tol = 1e-12 * float(np.linalg.norm(A.b))

    def others():
        single = single_solves(hp, gpu, M, B[:2], X0[:2], 40)
        Bd, Xd = dev(gpu, B), dev(gpu, X0)
        ierr, its, nrs, _ = hp.HPCCG_batch(M, Bd, Xd, max_iter=40, device=True)
        assert ierr == 0
        return single, (Xd.cpu().numpy().tobytes(), its.tobytes(), nrs.tobytes())

    before = others()
    first = mixed_solve(hp, gpu, M, B, X0, 400, tol)
    after = others()
    assert_same(after[0], before[0])
    assert after[1] == before[1]
    for _ in range(3):
        assert_same(mixed_solve(hp, gpu, M, B, X0, 400, tol), first, sweeps=True)
    assert M.mixed_workspace_bytes() > 0


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.mixed_live_workspaces()
    prob = hp.generate_matrix(8, 8, 8)
    M = hp.Matrix.from_hpc(prob)
    M2 = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 2)
        first = mixed_solve(hp, gpu, M, B, X0, 10)
        mixed_solve(hp, gpu, M2, B, X0, 10)
        assert hp.mixed_live_workspaces() == base + 2
        info = M2.mixed_info()
        assert info["image_bytes"] == 4 * 512 * 27 and info["workspace_bytes"] > 0
        assert M2.mixed_workspace_bytes() == info["image_bytes"] + info["workspace_bytes"]
        M2.mixed_release()
        assert hp.mixed_live_workspaces() == base + 1 and M2.mixed_workspace_bytes() == 0
        assert_same(mixed_solve(hp, gpu, M2, B, X0, 10), first)  # rebuilt on demand
        M2.mixed_release()
        M2.mixed_release()  # (idempotent)
        assert hp.mixed_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()
        M2.close()
        prob.close()
    assert hp.mixed_live_workspaces() == base


def test_refusals_leave_the_process_working(hp, gpu):
    L = hp.mixed_lib()
    M, A, xexact = problem(hp, "16c")
    n = A.nrow
    B, X0 = columns(A.b, xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()

    def call(h, nrhs=2, ldb=n, ldx=n, max_iter=10, sweeps=8, rtol=-1.0):
        return L.hpccg_hip_mixed_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, max_iter, 0.0, sweeps,
                                              rtol, it, nr, None)

    members = hp.group_generate(8, 8, 8, nranks=2)
    try:
        for m in members:
            assert call(m.h) == EINVAL
            assert b"group" in hp.lib().hpccg_hip_last_error()
            with pytest.raises(hp.HPCCGError):
                hp.HPC_sparsemv_mixed(m, Xd, Bd)
            with pytest.raises(hp.HPCCGError):
                m.mixed_info()
    finally:
        for m in members:
            m.close()
    assert call(M.h, ldb=n - 1) == EINVAL
    assert call(M.h, ldx=n - 1) == EINVAL
    assert call(M.h, max_iter=-1) == EINVAL
    assert call(M.h, nrhs=0) == EINVAL
    assert call(M.h, sweeps=0) == EINVAL
    assert call(M.h, rtol=1.0) == EINVAL
    assert call(None) == EINVAL
    assert Xd.cpu().numpy().tobytes() == X0.tobytes()  # nothing was touched
    with pytest.raises(hp.HPCCGError):
        hp.HPCCG_mixed(M, Bd, Xd, max_iter=-1, device=True)
    # ... and a good solve afterwards
    assert_same(mixed_solve(hp, gpu, M, B, X0, 10), single_solves(hp, gpu, M, B, X0, 10))
