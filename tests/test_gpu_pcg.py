"""Diagonally preconditioned CG (include/hpccg_hip_pcg.h,
lib/libhpccg_hip_pcg.so): per column the recurrence of the header with
M^-1 = diag(m), by default Jacobi m_i = 1 / a_ii; loop test, niters, normr and
trace on the 2-norm of r.

  1. m = 1: every column is bitwise the single solve (x, niters, normr, trace);
  2. m = 2^-3 and m = 2^5 everywhere: the same bits (every quantity scales exactly);
  3. Jacobi on S A S with S b, S powers of two: s_i x'_i is bitwise the x of
     Jacobi on A with b (the per-row m, the division, both SpMM forms);
  4. on matrices scaled by s_i = 10^u_i: the NumPy restatement below (trace,
     niters under a tolerance, x against xexact);
  5. it pays: on scaled 16^3 Jacobi converges where the plain solve does not;
  6. column c of a multi-column call is bitwise the single-column call;
  7. host solve = device solve, explicit 1 / diagonal = the default, the
     diagonal read from the image = the CSR's;
  8. refusals and the workspace's life.

Shapes (the smallest that reach every path; those of test_gpu_mixed.py): 16^3
(8 slices), 33^3 (71 slices: two dot groups), 12x10x16 7-pt (a tail slice),
1x1x1, 1x40x3, a 600-row band (per-slice widths), random dyadic SPD CSR with
513 and 3000 rows (entries in random order: the int32-column image; 513: one
row in the last slice) -- and each of them with every entry a_ij s_i s_j,
s_i = 2^e_i, e_i random in [-6, 6] ("p2_"), or s_i = 10^u_i, u_i uniform in
[-1.5, 1.5] ("p10_").
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_mixed import CSRS, STENCILS, assert_same, band600, columns, dev, finish, random_spd, single_solves

pytestmark = pytest.mark.gpu

EINVAL = -1

BASE = list(STENCILS) + ["band600", "dyadic_csr513", "dyadic_csr3000"]
P2 = ["p2_" + k for k in BASE]
# 4.: the restatement run with two dot orders (a sequential sum and numpy's
# blocked one) agrees with itself on the checked part of the rtrans trace to
# 7.7e-11 (16c), 4.9e-12 (33c), 3.5e-14 (7pt), 1.2e-13 (band600), 1.1e-14
# (csr513): within a tenth of RTRANS_RTOL_1GPU. (p10_dyadic_csr3000: 1.5e-9, left out.)
P10 = ["p10_" + k for k in ("16c", "33c", "12x10x16_7pt", "band600", "dyadic_csr513")]


# ---------------------------------------------------------------------------
# problems: name -> (Matrix, oracle.CSR with b = A 1, scale s or None)
# ---------------------------------------------------------------------------
def rows_of(A):
    return np.repeat(np.arange(A.nrow, dtype=np.int64), np.diff(A.row_ptr))


def scaled(A, s):
    """Every entry a_ij s_i s_j, b = A' 1."""
    return finish(A.row_ptr, A.cols, (A.vals * s[rows_of(A)]) * s[A.cols.astype(np.int64)])


def csr_diagonal(A):
    rows = rows_of(A)
    d = np.zeros(A.nrow)
    sel = rows == A.cols
    d[rows[sel]] = A.vals[sel]
    return d


def base_csr(name):
    if name in STENCILS:
        nx, ny, nz, s7 = STENCILS[name]
        return oracle.generate(nx, ny, nz, use_7pt=s7)
    if name == "band600":
        return band600()
    n, per_row, band, seed = CSRS[name.split("_")[1]]
    return random_spd(np.random.default_rng(seed), n, per_row, band, True)


def scale_of(kind, n):
    rng = np.random.default_rng(77)
    return 2.0 ** rng.integers(-6, 7, n) if kind == "p2" else 10.0 ** rng.uniform(-1.5, 1.5, n)


_problems = {}


def problem(hp, name):
    if name not in _problems:
        kind, _, rest = name.partition("_")
        if kind in ("p2", "p10"):
            A0 = base_csr(rest)
            s = scale_of(kind, A0.nrow)
            A = scaled(A0, s)
            M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
        elif name in STENCILS:
            nx, ny, nz, s7 = STENCILS[name]
            A, s = base_csr(name), None
            prob = hp.generate_matrix(nx, ny, nz, use_7pt=s7)
            M = hp.Matrix.from_hpc(prob)
            prob.close()
        else:
            A, s = base_csr(name), None
            M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
        _problems[name] = (M, A, s)
    return _problems[name]


@pytest.fixture(scope="module", autouse=True)
def _close_problems(hp):
    yield
    for M, _, _ in _problems.values():
        M.close()
    _problems.clear()
    assert hp.pcg_live_workspaces() == 0


def pcg_solve(hp, gpu, M, B, X0, max_iter, tol=0.0, minv=None, ld=None):
    """[(x, niters, normr, trace)] per column of a device solve; minv: None
    (Jacobi), a number (that value everywhere) or an array."""
    import torch
    n = B.shape[1]
    Bd, Xd = dev(gpu, B, ld), dev(gpu, X0, ld)
    if minv is not None:
        minv = torch.from_numpy(np.full(n, 1.0) * np.float64(minv)).to(gpu)
    ierr, its, nrs, times = hp.HPCCG_pcg(M, Bd, Xd, max_iter=max_iter, tolerance=tol, minv=minv, device=True)
    assert ierr == 0 and times[0] > 0.0 and not times[1:].any()
    X = Xd.cpu().numpy()
    if ld and ld > n:
        assert np.all(X[:, n:] == 7.5)  # nothing stored between the columns
    return [(X[c, :n].copy(), int(its[c]), float(nrs[c]), M.last_trace_pcg(c).copy()) for c in range(B.shape[0])]


# ---------------------------------------------------------------------------
# The recurrence of include/hpccg_hip_pcg.h restated: oracle.sparsemv and a
# fixed-order (sequential) float64 dot by default (dot: another order, for the
# restatement's own error). trace[k] is the normr iteration k
# reports, sqrt(rr_{k-1}) (HPCCG.cpp:358), as in every solver here.
# ---------------------------------------------------------------------------
def restated(A, b, minv, max_iter, tol=0.0, x0=None, dot=oracle.ddot):
    with np.errstate(all="ignore"):
        x = np.zeros(A.nrow) if x0 is None else np.array(x0, np.float64)
        p = x + 0.0 * x
        Ap = oracle.sparsemv(A, p)
        r = b + (-1.0) * Ap
        rz = np.float64(dot(r, minv * r))
        oldrz = rz
        hist = [np.float64(dot(r, r))]
        normr = np.sqrt(hist[0])
        trace = [normr]
        k = 1
        while k < max_iter and normr > tol:
            z = minv * r
            p = z + 0.0 * z if k == 1 else z + (rz / oldrz) * p
            normr = np.sqrt(hist[k - 1])
            trace.append(normr)
            Ap = oracle.sparsemv(A, p)
            alpha = rz / np.float64(dot(p, Ap))
            x = x + alpha * p
            r = r + (-alpha) * Ap
            oldrz = rz
            rz = np.float64(dot(r, minv * r))
            hist.append(np.float64(dot(r, r)))
            k += 1
    return x, k - 1, float(normr), np.array(trace)


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
# 1., 2. a uniform m: the single solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2)
def test_uniform_m_is_the_single_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 5)
    assert X0[1].any()  # a nonzero x0 among them
    full = single_solves(hp, gpu, M, B, X0, 60)
    # a tolerance that column 0 meets part-way: just above the smallest residual of its first half
    tr0 = full[0][3]
    tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10) if len(tr0) > 4 else 0.0
    part = single_solves(hp, gpu, M, B, X0, 60, tol)
    print(f"{shape}: stops {[r[1] for r in part]} under the tolerance, {[r[1] for r in full]} without")
    if n > 1:
        assert part[0][1] < full[0][1], (part[0][1], full[0][1])
    for max_iter, t, ref in ((60, 0.0, full), (60, tol, part), (1, 0.0, None), (0, 0.0, None)):
        if ref is None:
            ref = single_solves(hp, gpu, M, B, X0, max_iter, t)
        for nrhs, ld in ((5, n), (4, n), (3, n + 3), (2, n), (1, n)):
            assert_same(pcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], max_iter, t, minv=1.0, ld=ld), ref[:nrhs])
        for m in (2.0 ** -3, 2.0 ** 5):
            for nrhs in (5, 1):
                assert_same(pcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], max_iter, t, minv=m), ref[:nrhs])


# ---------------------------------------------------------------------------
# 3. exact scaling
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
        got = pcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 20)
        gots = pcg_solve(hp, gpu, Ms, B[:nrhs] * s, X0[:nrhs], 20)
        for c in range(nrhs):
            assert got[c][1] == gots[c][1] == 19
            assert (gots[c][0] * s).tobytes() == got[c][0].tobytes(), (nrhs, c, float(np.max(np.abs(gots[c][0] * s - got[c][0]))))
            assert np.all(np.isfinite(got[c][0])) and got[c][0].any()


# ---------------------------------------------------------------------------
# 4. the restatement
# ---------------------------------------------------------------------------
_restated = {}


def restated_full(hp, name, max_iter=200):
    if name not in _restated:
        _, A, _ = problem(hp, name)
        _restated[name] = restated(A, A.b, 1.0 / csr_diagonal(A), max_iter)
    return _restated[name]


@pytest.mark.parametrize("shape", P10)
def test_jacobi_follows_the_restatement(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    _, _, _, tr_ref = restated_full(hp, shape)
    r0 = tr_ref[0]
    # the trace, as far as the restatement is above the rounding floor; converged
    # is normr <= 1e-14 r0, where the restatement's own x is within 3.9e-11 of
    # xexact on these matrices (1e-12 r0: up to 3.6e-9)
    x, niters, normr, tr = pcg_solve(hp, gpu, M, B, X0, 200, 1e-14 * r0)[0]
    checked = check_trace(tr, tr_ref, RTRANS_RTOL_1GPU)
    print(f"{shape}: {checked} trace points checked, niters {niters}")
    assert checked >= 10, checked
    # converged: x against xexact
    err = float(np.max(np.abs(x - A.xexact)))
    print(f"{shape}: normr/r0 {normr / r0:.3e} max |x - xexact| {err:.3e}")
    assert normr <= 1e-14 * r0 and niters < 199
    assert err <= 1e-9, err
    # niters under a tolerance between two residuals of the restatement: the
    # widest gap in the middle third of the checked part
    lo, hi = checked // 3, 2 * checked // 3
    k = lo + int(np.argmax(tr_ref[lo:hi] / tr_ref[lo + 1:hi + 1]))
    assert tr_ref[k] > 1.01 * tr_ref[k + 1], (k, tr_ref[k], tr_ref[k + 1])
    tol = float(np.sqrt(tr_ref[k] * tr_ref[k + 1]))
    _, it_ref, nr_ref, _ = restated(A, A.b, minv, 200, tol)
    _, it, nr, _ = pcg_solve(hp, gpu, M, B, X0, 200, tol)[0]
    assert it == it_ref and 0 < it < niters, (it, it_ref, niters)
    assert abs(nr - nr_ref) <= RTRANS_RTOL_1GPU * nr_ref, (nr, nr_ref)


# ---------------------------------------------------------------------------
# 5. it pays
# ---------------------------------------------------------------------------
def test_jacobi_converges_where_the_plain_solve_does_not(hp, gpu):
    M, A, _ = problem(hp, "p2_16c")
    n = A.nrow
    B, X0 = A.b.reshape(1, n).copy(), np.zeros((1, n))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    tol = 1e-10 * r0
    _, it_ref, _, _ = restated(A, A.b, 1.0 / csr_diagonal(A), 200, tol)
    x, it, nr, tr = pcg_solve(hp, gpu, M, B, X0, 200, tol)[0]
    plain = single_solves(hp, gpu, M, B, X0, 200, tol)[0]
    print(f"p2_16c: Jacobi {it} iterations (restatement {it_ref}), normr/r0 {nr / r0:.3e}; plain {plain[1]} iterations, "
          f"normr/r0 {plain[2] / r0:.3e}")
    assert it <= it_ref + 2 and it < 100, (it, it_ref)
    assert nr <= tol
    assert plain[1] == 199 and plain[2] > tol, plain[1:3]


# ---------------------------------------------------------------------------
# 6. columns are independent
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
    one = [pcg_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], 150, tol)[0] for c in range(5)]
    stops = [o[1] for o in one]
    assert len(set(stops)) >= 3 and max(stops) < 149 and stops[4] == 0, stops
    for nrhs, ld in ((5, n + 5), (4, n), (3, n), (2, n)):
        got = pcg_solve(hp, gpu, M, B[:nrhs], X0[:nrhs], 150, tol, ld=ld)
        assert_same(got, one[:nrhs])
        for g in got[:4]:
            assert len(g[3]) == g[1] + 1 and g[2] == g[3][-1]
    # ... and when the iterations run out first
    for max_iter in (2, 7):
        got = pcg_solve(hp, gpu, M, B, X0, max_iter, tol)
        assert max(g[1] for g in got) == max_iter - 1 and got[4][1] == 0
        assert_same(got, [pcg_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], max_iter, tol)[0] for c in range(5)])


# ---------------------------------------------------------------------------
# 7. host and device, the diagonal
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE + P2 + P10)
def test_the_diagonal_is_the_csr_diagonal(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    assert M.diagonal_pcg().tobytes() == csr_diagonal(A).tobytes()


@pytest.mark.parametrize("shape", ["p2_33c", "p10_dyadic_csr513", "band600"])
def test_host_solve_and_explicit_jacobi_are_the_device_solve(hp, gpu, shape):
    M, A, _ = problem(hp, shape)
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 3)
    ref = pcg_solve(hp, gpu, M, B, X0, 25)
    X = X0.copy()
    ierr, its, nrs, times = hp.HPCCG_pcg(M, B, X, max_iter=25)
    assert ierr == 0 and times[0] > 0.0 and times[6] > 0.0 and not times[1:6].any()
    assert_same([(X[c], int(its[c]), float(nrs[c]), M.last_trace_pcg(c).copy()) for c in range(3)], ref)
    minv = 1.0 / M.diagonal_pcg()
    assert_same(pcg_solve(hp, gpu, M, B, X0, 25, minv=minv), ref)
    X = X0.copy()
    ierr, its, nrs, _ = hp.HPCCG_pcg(M, B, X, max_iter=25, minv=minv)
    assert_same([(X[c], int(its[c]), float(nrs[c]), M.last_trace_pcg(c).copy()) for c in range(3)], ref)
    # one column as a vector, updated in place
    x = X0[1].copy()
    hp.HPCCG_pcg(M, B[1].copy(), x, max_iter=25)
    assert x.tobytes() == pcg_solve(hp, gpu, M, B[1:2], X0[1:2], 25)[0][0].tobytes()


# ---------------------------------------------------------------------------
# 8. refusals, the workspace
# ---------------------------------------------------------------------------
def _edited(A, edit):
    rp, cols, vals = A.row_ptr.copy(), A.cols.copy(), A.vals.copy()
    return edit(rp, cols, vals, rows_of(A))


def _zero_diag(rp, cols, vals, rows):
    vals[(rows == 517) & (cols == 517)] = 0.0
    return rp, cols, vals, 517


def _negative_diag(rp, cols, vals, rows):
    vals[(rows == 512) & (cols == 512)] *= -1.0
    return rp, cols, vals, 512


def _missing_diag(rp, cols, vals, rows):
    keep = ~((rows == cols) & ((rows == 5) | (rows == 300)))
    lens = np.bincount(rows[keep], minlength=len(rp) - 1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), cols[keep], vals[keep], 5


@pytest.mark.parametrize("base,edit", [("band600", _zero_diag), ("dyadic_csr513", _negative_diag),
                                       ("band600", _missing_diag), ("dyadic_csr3000", _missing_diag)],
                         ids=["zero_a", "negative_sell", "missing_a", "missing_sell"])
def test_a_bad_diagonal_is_refused(hp, gpu, base, edit):
    import torch
    A = base_csr(base)
    n = A.nrow
    rp, cols, vals, row = _edited(A, edit)
    M = hp.Matrix.from_csr(rp, cols, vals)
    try:
        d = M.diagonal_pcg()
        if edit is _missing_diag:
            assert d[5] == 0.0 and d[300] == 0.0 and np.all(np.delete(d, [5, 300]) > 0.0)
        Bd = torch.ones((2, n), dtype=torch.float64, device=gpu)
        Xd = torch.full((2, n), 0.5, dtype=torch.float64, device=gpu)
        it = (C.c_int * 2)()
        nr = (C.c_double * 2)()
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match=rf"row {row} "):
                hp.HPCCG_pcg(M, Bd, Xd, max_iter=10, device=True)
        assert hp.pcg_lib().hpccg_hip_pcg_solve_device(M.h, 2, Bd.data_ptr(), n, Xd.data_ptr(), n, None, 10, 0.0, it, nr,
                                                       None) == EINVAL
        assert torch.all(Xd == 0.5)
        # a caller's m is taken on the same matrix
        assert hp.HPCCG_pcg(M, Bd, Xd.clone(), max_iter=3, minv=torch.ones(n, dtype=torch.float64, device=gpu),
                            device=True)[0] == 0
    finally:
        M.close()


def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.pcg_lib()
    M, A, _ = problem(hp, "16c")
    n = A.nrow
    B, X0 = columns(A.b, A.xexact, 2)
    Bd, Xd = dev(gpu, B), dev(gpu, X0)
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = pcg_solve(hp, gpu, M, B, X0, 10)

    def call(h, nrhs=2, ldb=n, ldx=n, minv=None, max_iter=10):
        return L.hpccg_hip_pcg_solve_device(h, nrhs, Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, minv, max_iter, 0.0, it, nr,
                                            None)

    members = hp.group_generate(8, 8, 8, nranks=2)
    try:
        for m in members:
            assert call(m.h) == EINVAL
            assert b"group" in hp.lib().hpccg_hip_last_error()
            with pytest.raises(hp.HPCCGError):
                m.diagonal_pcg()
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
            hp.HPCCG_pcg(M, B.copy(), X0.copy(), max_iter=10, minv=mv)
    assert call(M.h, ldb=n - 1) == EINVAL
    assert b"leading dimension" in hp.lib().hpccg_hip_last_error()
    assert call(M.h, ldx=n - 1) == EINVAL
    assert call(M.h, max_iter=-1) == EINVAL
    assert call(M.h, nrhs=0) == EINVAL
    assert call(None) == EINVAL
    assert Xd.cpu().numpy().tobytes() == X0.tobytes()  # nothing was touched
    # ... and a good solve afterwards
    assert_same(pcg_solve(hp, gpu, M, B, X0, 10), ref)


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
        return single, (Xd.cpu().numpy().tobytes(), its.tobytes(), nrs.tobytes(), Xm.cpu().numpy().tobytes(),
                        itm.tobytes(), nrm.tobytes())

    before = others()
    first = pcg_solve(hp, gpu, M, B, X0, 40)
    after = others()
    assert_same(after[0], before[0])
    assert after[1] == before[1]
    for _ in range(3):
        assert_same(pcg_solve(hp, gpu, M, B, X0, 40), first)
    assert M.pcg_workspace_bytes() > 0
    M.batch_release()
    M.mixed_release()


def test_workspace_goes_with_the_matrix(hp, gpu):
    base = hp.pcg_live_workspaces()
    prob = hp.generate_matrix(8, 8, 8)
    M = hp.Matrix.from_hpc(prob)
    M2 = hp.Matrix.from_hpc(prob)
    try:
        B, X0 = columns(prob.b, prob.xexact, 2)
        first = pcg_solve(hp, gpu, M, B, X0, 10)
        pcg_solve(hp, gpu, M2, B, X0, 10)
        assert hp.pcg_live_workspaces() == base + 2
        assert M2.pcg_workspace_bytes() > 2 * 8 * 512
        M2.pcg_release()
        assert hp.pcg_live_workspaces() == base + 1 and M2.pcg_workspace_bytes() == 0
        assert_same(pcg_solve(hp, gpu, M2, B, X0, 10), first)  # rebuilt on demand, the Jacobi cache too
        small = M2.pcg_workspace_bytes()
        pcg_solve(hp, gpu, M2, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the cache stays
        assert M2.pcg_workspace_bytes() > small
        assert_same(pcg_solve(hp, gpu, M2, B, X0, 10), first)
        M2.pcg_release()
        M2.pcg_release()  # (idempotent)
        assert hp.pcg_live_workspaces() == base + 1
        assert first[0][1] == 9
    finally:
        M.close()
        M2.close()
        prob.close()
    assert hp.pcg_live_workspaces() == base
