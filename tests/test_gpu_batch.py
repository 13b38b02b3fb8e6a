"""Batched multi-right-hand-side CG (include/hpccg_hip_batch.h,
lib/libhpccg_hip_batch.so): every column of a batch is bitwise the single
solve of that column -- x, niters, normr and the whole residual trace -- and
every column of the batched SpMM is bitwise HPC_sparsemv of that column. The
single solve is the reference; one case checks the batch against the CPU
oracle as well, to catch a bug the two GPU paths could share.

Shapes: 16^3 (8 slices, one group of the dot), 33^3 (71 slices, a 97-row tail
slice, two groups), 12x10x16 7-pt, 1x1x1 and 1x40x3 (degenerate axes, fewer
than 512 rows), random SPD CSR with n = 1, 513, 3000 (entries in random order:
no SELL-512-A image, the int32-column SpMM), 7-pt 256x256x130 (260 groups:
past the first 256 of the dot's top level).
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import RTRANS_RTOL_1GPU, check_trace

pytestmark = pytest.mark.gpu

EINVAL = -1


# ---------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------
def random_spd(rng, n, per_row, band):
    """Symmetric, strictly diagonally dominant (so SPD), entries of each row in
    random order; b = A 1 (the generator of test_gpu_random_csr.py)."""
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for _ in range(int(rng.integers(0, per_row + 1))):
            j = int(i + rng.integers(-band, band + 1)) if band else int(rng.integers(0, n))
            if 0 <= j < n and j != i:
                v = -float(rng.uniform(0.05, 1.0))
                rows[i][j] = v
                rows[j][i] = v
    row_ptr = np.zeros(n + 1, np.int64)
    cols, vals = [], []
    for i in range(n):
        d = rows[i]
        ent = list(d.items()) + [(i, sum(-v for v in d.values()) + float(rng.uniform(0.5, 2.0)))]
        order = rng.permutation(len(ent))
        for k in order:
            cols.append(ent[k][0])
            vals.append(ent[k][1])
        row_ptr[i + 1] = len(cols)
    A = oracle.CSR(row_ptr, np.asarray(cols, np.int32), np.asarray(vals, np.float64), np.zeros(n), np.zeros(n),
                   np.ones(n))
    A.b = oracle.sparsemv(A, np.ones(n))
    return A


STENCILS = {
    "16c": (16, 16, 16, False),
    "33c": (33, 33, 33, False),
    "12x10x16_7pt": (12, 10, 16, True),
    "1x1x1": (1, 1, 1, False),
    "1x40x3": (1, 40, 3, False),
}
CSRS = {"csr1": (1, 0, 0, 11), "csr513": (513, 6, 40, 12), "csr3000": (3000, 9, 0, 13)}
SHAPES = list(STENCILS) + list(CSRS)

_problems = {}


def problem(hp, name):
    """(Matrix, b, xexact) of a shape, built once for the module."""
    if name not in _problems:
        if name in STENCILS:
            nx, ny, nz, s7 = STENCILS[name]
            prob = hp.generate_matrix(nx, ny, nz, use_7pt=s7)
            _problems[name] = (hp.Matrix.from_hpc(prob), prob.b, prob.xexact)
            prob.close()
        else:
            n, per_row, band, seed = CSRS[name]
            A = random_spd(np.random.default_rng(seed), n, per_row, band)
            _problems[name] = (hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals), A.b.copy(), np.ones(n))
    return _problems[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems(hp):
    yield
    for M, _, _ in _problems.values():
        M.close()
    _problems.clear()
    assert hp.batch_live_workspaces() == 0


def columns(b, xexact, nrhs, seed=5):
    """The test's right-hand sides and initial guesses, (nrhs, n) each."""
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
            X0[c] = xexact  # b = A 1 sums small integers: an exactly zero residual
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
    """The reference: every column solved alone on the device."""
    import torch
    out = []
    for c in range(B.shape[0]):
        b = torch.from_numpy(B[c].copy()).to(gpu)
        x = torch.from_numpy(X0[c].copy()).to(gpu)
        if len(B[c]) == 0:
            continue
        ierr, it, nr, _ = hp.HPCCG(M, b, x, max_iter=max_iter, tolerance=tol, device=True)
        assert ierr == 0
        out.append((x.cpu().numpy(), it, nr, M.last_trace().copy()))
    return out


def batch_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, ld=None):
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    ierr, its, nrs, times = hp.HPCCG_batch(M, Bd, Xd, max_iter=max_iter, tolerance=tol, device=True)
    assert ierr == 0
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_batch(c).copy()) for c in range(B.shape[0])]


def assert_same(got, ref):
    assert len(got) == len(ref)
    for c, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == r[1], (c, g[1], r[1])
        assert np.float64(g[2]).tobytes() == np.float64(r[2]).tobytes(), (c, g[2], r[2])
        assert g[3].tobytes() == r[3].tobytes(), (c, "trace")
        assert g[0].tobytes() == r[0].tobytes(), (c, "x", float(np.max(np.abs(g[0] - r[0]))))


# ---------------------------------------------------------------------------
# 1. SpMM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3], ids=["ld_n", "ld_n3"])
@pytest.mark.parametrize("shape", SHAPES)
def test_spmm_columns_are_sparsemv(hp, gpu, shape, pad):
    import torch
    M, b, _ = problem(hp, shape)
    n = len(b)
    rng = np.random.default_rng(21)
    V = rng.uniform(-1.0, 1.0, (9, n))
    ref = []
    for c in range(9):
        y = torch.zeros(n, dtype=torch.float64, device=gpu)
        hp.HPC_sparsemv(M, torch.from_numpy(V[c].copy()).to(gpu), y)
        ref.append(y.cpu().numpy())
    for nrhs in (1, 2, 3, 4, 5, 9):
        Xd = dev(gpu, V[:nrhs], n + pad)
        Yd = torch.full((nrhs, n + pad), -3.0, dtype=torch.float64, device=gpu)
        hp.HPC_sparsemv_batch(M, Xd, Yd)
        Y = Yd.cpu().numpy()
        for c in range(nrhs):
            assert Y[c, :n].tobytes() == ref[c].tobytes(), (nrhs, c)
        assert np.all(Y[:, n:] == -3.0)


# ---------------------------------------------------------------------------
# 2. solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_solve_columns_are_single_solves(hp, gpu, shape):
    M, b, xexact = problem(hp, shape)
    n = len(b)
    B, X0 = columns(b, xexact, 5)
    for max_iter in (1, 2, 30, 150):
        ref = single_solves(hp, gpu, M, B, X0, max_iter)
        assert ref[2][1] == 0  # column 2 ends before its first iteration
        if max_iter > 1 and n > 1:
            assert ref[0][1] > 0  # ... while the others run
        for nrhs, ld in ((5, n), (4, n + 3), (3, n), (2, n), (1, n)):
            got = batch_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], max_iter, ld=ld)
            assert_same(got, ref[:nrhs])


def test_host_solve_is_device_solve(hp, gpu):
    M, b, xexact = problem(hp, "33c")
    B, X0 = columns(b, xexact, 4)
    ref = batch_solve(hp, gpu, M, B, X0, 25)
    X = X0.copy()
    ierr, its, nrs, times = hp.HPCCG_batch(M, B, X, max_iter=25)
    assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
    got = [(X[c], int(its[c]), float(nrs[c]), M.last_trace_batch(c).copy()) for c in range(4)]
    assert_same(got, ref)


# ---------------------------------------------------------------------------
# 3. staggered stops
# ---------------------------------------------------------------------------
def test_columns_stop_at_their_own_iteration(hp, gpu):
    M, b, xexact = problem(hp, "16c")
    n = len(b)
    rng = np.random.default_rng(9)
    # the same tolerance meets differently scaled residuals at different iterations
    B = np.stack([b, b * 2.0 ** -20, rng.uniform(-1.0, 1.0, n) * 2.0 ** 10, b * 2.0 ** -40])
    X0 = np.zeros((4, n))
    tol = 1e-6
    ref = single_solves(hp, gpu, M, B, X0, 150, tol)
    stops = [r[1] for r in ref]
    assert len(set(stops)) >= 2, stops  # the reference itself staggers
    assert min(stops) < 149
    assert_same(batch_solve(hp, gpu, M, B, X0, 150, tol), ref)


# ---------------------------------------------------------------------------
# 4. independent check against the CPU oracle
# ---------------------------------------------------------------------------
def test_batch_against_cpu_oracle(hp, gpu):
    nx = 20
    prob = hp.generate_matrix(nx, nx, nx)
    M = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 4)
        got = batch_solve(hp, gpu, M, B, X0, 60)
    finally:
        M.close()
        prob.close()
    A = oracle.generate(nx, nx, nx)
    for c in (0, 1, 3):  # (column 2's residual is exactly zero: nothing to compare against)
        ref = oracle.hpccg(A, b=B[c].copy(), x=X0[c].copy(), max_iter=60)
        assert got[c][1] == ref["niters"]
        assert check_trace(got[c][3], ref["trace"], RTRANS_RTOL_1GPU) >= 10, c
        assert float(np.max(np.abs(got[c][0] - ref["x"]))) <= 1e-9 * max(1.0, float(np.max(np.abs(ref["x"]))))
    assert got[2][1] == 0 and got[2][2] == 0.0


# ---------------------------------------------------------------------------
# 5. wide top level
# ---------------------------------------------------------------------------
def test_wide_top_level(hp, gpu):
    import torch
    M = hp.Matrix.generate(256, 256, 130, use_7pt=True)
    try:
        n = int(M.info()["nrow"])
        assert (n + 511) // 512 > 64 * 256  # more than 256 groups
        b = torch.zeros(n, dtype=torch.float64, device=gpu)
        hp.HPC_sparsemv(M, torch.ones(n, dtype=torch.float64, device=gpu), b)  # b = A 1, exact
        g = torch.arange(n, dtype=torch.float64, device=gpu)
        Bd = torch.stack([b, b * 2.0 ** -3])
        X0 = torch.stack([torch.zeros_like(b), 0.25 * (torch.remainder(g, 7) - 3)])
        ref = []
        for c in range(2):
            x = X0[c].clone()
            ierr, it, nr, _ = hp.HPCCG(M, Bd[c], x, max_iter=4, device=True)
            ref.append((x, it, nr, M.last_trace().copy()))
        Xd = X0.clone()
        ierr, its, nrs, _ = hp.HPCCG_batch(M, Bd, Xd, max_iter=4, device=True)
        assert ierr == 0
        for c in range(2):
            assert int(its[c]) == ref[c][1] == 3
            assert np.float64(nrs[c]).tobytes() == np.float64(ref[c][2]).tobytes()
            assert M.last_trace_batch(c).tobytes() == ref[c][3].tobytes()
            assert torch.equal(Xd[c], ref[c][0])
    finally:
        M.close()


# ---------------------------------------------------------------------------
# 6. state
# ---------------------------------------------------------------------------
def test_repeats_and_single_solves_do_not_disturb_each_other(hp, gpu):
    M, b, xexact = problem(hp, "33c")
    B, X0 = columns(b, xexact, 4)
    before = single_solves(hp, gpu, M, B[:2], X0[:2], 40)
    first = batch_solve(hp, gpu, M, B, X0, 40)
    after = single_solves(hp, gpu, M, B[:2], X0[:2], 40)
    assert_same(after, before)
    for _ in range(19):
        assert_same(batch_solve(hp, gpu, M, B, X0, 40), first)
    assert_same(first[:2], before)
    assert M.batch_workspace_bytes() > 0


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.batch_live_workspaces()
    prob = hp.generate_matrix(8, 8, 8)
    M = hp.Matrix.from_hpc(prob)
    M2 = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 2)
        batch_solve(hp, gpu, M, B, X0, 10)
        batch_solve(hp, gpu, M2, B, X0, 10)
        assert hp.batch_live_workspaces() == base + 2
        M2.batch_release()
        assert hp.batch_live_workspaces() == base + 1 and M2.batch_workspace_bytes() == 0
        first = batch_solve(hp, gpu, M2, B, X0, 10)  # rebuilt on demand
        M2.batch_release()
        M2.batch_release()  # (idempotent)
        assert hp.batch_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()
        M2.close()
        prob.close()
    assert hp.batch_live_workspaces() == base


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_the_process_working(hp, gpu):
    L = hp.batch_lib()
    M, b, xexact = problem(hp, "16c")
    n = len(b)
    B, X0 = columns(b, xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()

    def call(h, nrhs=2, ldb=n, ldx=n, max_iter=10):
        return L.hpccg_hip_batch_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, max_iter, 0.0, it, nr,
                                              None)

    members = hp.group_generate(8, 8, 8, nranks=2)
    try:
        for m in members:
            assert call(m.h, ldb=n, ldx=n) == EINVAL
            assert b"batch" in hp.lib().hpccg_hip_last_error()
            with pytest.raises(hp.HPCCGError):
                hp.HPC_sparsemv_batch(m, Xd, Bd)
    finally:
        for m in members:
            m.close()
    assert call(M.h, ldb=n - 1) == EINVAL
    assert call(M.h, ldx=n - 1) == EINVAL
    assert call(M.h, max_iter=-1) == EINVAL
    assert call(M.h, nrhs=0) == EINVAL
    assert call(None) == EINVAL
    assert Xd.cpu().numpy().tobytes() == X0.tobytes()  # nothing was touched
    with pytest.raises(hp.HPCCGError):
        hp.HPCCG_batch(M, Bd, Xd, max_iter=-1, device=True)
    # ... and a good batch afterwards
    assert_same(batch_solve(hp, gpu, M, B, X0, 10), single_solves(hp, gpu, M, B, X0, 10))
