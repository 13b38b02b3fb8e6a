"""Single-reduction CG with the Chebyshev polynomial preconditioner over an
in-process rank group (include/hpccg_hip_srpoly_group.h,
lib/libhpccg_hip_srpoly_group.so): per column the recurrence of
hpccg_hip_srpoly.h, every member on its own rows, the ghost planes of z moved
after step 0 and after every step (the last: u), the three dots summed over the
members in rank order at one point. All members share one device.

  1. degree 0 is the group srcg bit for bit (every member's x, niters, normr,
     every trace);
  2. max_iter <= 2 is the group poly bit for bit, the trace still at 3;
  3. a group of one is the one-rank solve bit for bit, on every image form, with
     its spectrum and bound;
  4. column c of a multi-column call is bitwise its single-column call;
  5. the halo kernel against the halo by copies: the same bits;
  6. on matrices scaled by s_i = 10^u_i, degrees 1 to 4: the trace against the
     NumPy restatement of the global matrix within test_gpu_poly_group.py's bar,
     niters equal to group_HPCCG_poly's, x against xexact;
  7. the bound is the group poly's; 8. refusals (a bad diagonal on one member,
     the gather plan); 9. degenerate columns; 10. both non-temporal arms;
  11. other solves and repeats undisturbed; 12. the workspace's life.

Shapes and helpers: those of test_gpu_poly_group.py (its cases, "lap_" forms
included) and test_gpu_srcg_group.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import test_gpu_nt as tn
import test_gpu_pcg_group as tpg
import test_gpu_poly_group as tgp
import test_gpu_srcg_group as tgs
from conftest import RTRANS_RTOL_MULTI, check_trace
from test_gpu_pcg_group import SHAPES, assert_same, columns, csr_diagonal, dev, finish
from test_gpu_poly_group import DEGREES, EIG_RATIO, MAX_ITER, case
from test_gpu_srpoly import restated_srpoly

pytestmark = pytest.mark.gpu

EINVAL, EPLAN = -1, -5


def live(hp):
    return (hp.group_pcg_live_workspaces(), hp.group_poly_live_workspaces(), hp.group_srcg_live_workspaces(),
            hp.srpoly_live_workspaces(), hp.poly_live_workspaces(), hp.batch_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _close_cases(hp):
    base = hp.group_srpoly_live_workspaces()
    others = live(hp)
    yield
    for cache in (tgp._cases, tgs._cases):
        for c in cache.values():
            c.close()
        cache.clear()
    assert hp.group_srpoly_live_workspaces() == base
    assert live(hp) == others


def srpoly_solve(hp, gpu, cs, B, X0, max_iter, tol=0.0, degree=2, lmin=None, lmax=None, minv=None, pad=0,
                 halo_copies=False):
    """[(xs per member, niters, normr, trace)] per column of a group solve;
    minv: None (Jacobi), a number (that value everywhere) or a global array."""
    import torch
    Bd = [dev(gpu, a, pad) for a in cs.split(B)]
    Xd = [dev(gpu, a, pad) for a in cs.split(X0)]
    minvs = None
    if minv is not None:
        m = np.full(cs.N, 1.0) * np.float64(minv)
        minvs = [torch.from_numpy(m[rw].copy()).to(gpu) for rw in cs.rows]
    its, nrs, times = hp.group_HPCCG_srpoly(cs.Ms, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, minvs=minvs,
                                            max_iter=max_iter, tolerance=tol, halo_copies=halo_copies)
    assert times[0] > 0.0 and not times[1:].any()
    X = [x.cpu().numpy() for x in Xd]
    if pad:
        for x, rw in zip(X, cs.rows):
            assert np.all(x[:, rw.stop - rw.start:] == 7.5)  # nothing stored between the columns
    return [([x[c, :rw.stop - rw.start].copy() for x, rw in zip(X, cs.rows)], int(its[c]), float(nrs[c]),
             hp.group_last_trace_srpoly(cs.Ms, c).copy()) for c in range(B.shape[0])]


# ---------------------------------------------------------------------------
# 1. degree 0 is the group srcg
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_degree_0_is_the_group_srcg(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs)
    assert X0[1].any() and X0[3].any()  # nonzero x0 among them
    m_rand = np.random.default_rng(23).uniform(0.25, 4.0, cs.N)
    every = ((1, 0), (2, 3), (3, 0), (4, 0), (5, 3), (7, 0))  # every chunking of the launches, a padded ld
    for minv, counts in ((None, every), (1.0, ((5, 3), (1, 0))), (m_rand, ((7, 0), (2, 3)))):
        ref = tgs.srcg_solve(hp, gpu, cs, B, X0, MAX_ITER, minv=minv)
        assert ref[0][1] > 0
        for nrhs, pad in counts:
            assert_same(srpoly_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, degree=0, minv=minv, pad=pad),
                        ref[:nrhs])
        if minv is not None:
            continue
        # a tolerance that column 0 meets part-way, one iteration and none at all
        tr0 = ref[0][3]
        tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10)
        for max_iter, t in ((MAX_ITER, tol), (1, 0.0), (0, 0.0)):
            part = tgs.srcg_solve(hp, gpu, cs, B[:4], X0[:4], max_iter, t)
            if t:
                assert part[0][1] < ref[0][1], (part[0][1], ref[0][1])
            assert_same(srpoly_solve(hp, gpu, cs, B[:4], X0[:4], max_iter, t, degree=0), part)
        # (bounds given with degree 0 are checked, kept and not used)
        assert_same(srpoly_solve(hp, gpu, cs, B[:2], X0[:2], MAX_ITER, degree=0, lmin=0.5, lmax=3.0), ref[:2])
        assert hp.group_last_spectrum_srpoly(cs.Ms) == (0.5, 3.0)


# ---------------------------------------------------------------------------
# 2. the first iteration
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + ["p2_3x33x17x9", "p10_csr3", "lap_8x16c"])
def test_the_first_iteration_is_group_polys(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs)
    assert B.shape[0] == 7 and X0[1].any() and X0[3].any()  # nonzero x0 among them
    for degree in DEGREES:
        for max_iter in (0, 1, 2):
            ref = tgp.poly_solve(hp, gpu, cs, B, X0, max_iter, degree=degree)
            assert_same(srpoly_solve(hp, gpu, cs, B, X0, max_iter, degree=degree), ref)
            assert hp.group_last_spectrum_srpoly(cs.Ms) == hp.group_last_spectrum_poly(cs.Ms)
            assert max(r[1] for r in ref) == max(max_iter, 1) - 1
        ref = tgp.poly_solve(hp, gpu, cs, B, X0, 3, degree=degree)
        got = srpoly_solve(hp, gpu, cs, B, X0, 3, degree=degree)
        for c in range(7):
            assert got[c][1] == ref[c][1] and got[c][3].tobytes() == ref[c][3].tobytes(), (degree, c)
    # a caller's m, two columns
    m_rand = np.random.default_rng(23).uniform(0.25, 4.0, cs.N)
    assert_same(srpoly_solve(hp, gpu, cs, B[:2], X0[:2], 2, degree=3, minv=m_rand, pad=3),
                tgp.poly_solve(hp, gpu, cs, B[:2], X0[:2], 2, degree=3, minv=m_rand, pad=3))


# ---------------------------------------------------------------------------
# 3. a group of one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["a_image", "a_image_7pt", "sell"])
def test_group_of_one_is_the_one_rank_solve(hp, gpu, form):
    """nranks == 1 runs the same code on a halo-free matrix: 0.0 + a total is
    the total, so every column is bitwise HPCCG_srpoly's."""
    G1 = None
    if form == "sell":
        A = tpg.random_spd(np.random.default_rng(11), 1300, 6, 40)
        M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    else:
        s7 = form == "a_image_7pt"
        A = oracle.generate(12, 11, 10, use_7pt=s7)
        M = hp.Matrix.generate(12, 11, 10, use_7pt=s7)
        G1 = hp.group_generate(12, 11, 10, 1, use_7pt=s7)
    try:
        assert M.get_option("has_a") == int(form != "sell")
        rng = np.random.default_rng(3)
        B = np.stack([A.b, rng.uniform(-1.0, 1.0, A.nrow), 0.5 * A.b])
        for degree in (0,) + tuple(DEGREES):
            for nrhs in (3, 1):
                Xs = dev(gpu, np.zeros_like(B[:nrhs]))
                _, its1, nrs1, _ = hp.HPCCG_srpoly(M, dev(gpu, B[:nrhs]), Xs, degree=degree, max_iter=40, device=True)
                tr1 = [M.last_trace_srpoly(c).copy() for c in range(nrhs)]
                for Ms in ([M],) + ((G1,) if G1 else ()):  # a plain one-rank matrix and a one-member group
                    Bd, Xd = dev(gpu, B[:nrhs]), dev(gpu, np.zeros_like(B[:nrhs]))
                    its, nrs, _ = hp.group_HPCCG_srpoly(Ms, [Bd], [Xd], degree=degree, max_iter=40)
                    assert list(its) == list(its1) and nrs.tobytes() == nrs1.tobytes(), (degree, nrhs)
                    assert Xd.cpu().numpy().tobytes() == Xs.cpu().numpy().tobytes(), (degree, nrhs)
                    for c in range(nrhs):
                        assert hp.group_last_trace_srpoly(Ms, c).tobytes() == tr1[c].tobytes()
                    assert hp.group_last_spectrum_srpoly(Ms) == M.last_spectrum_srpoly()
            assert its1[0] == 39 and np.all(np.isfinite(Xs.cpu().numpy()))
        assert hp.group_srpoly_bound([M]) == hp.srpoly_bound(M)
        if G1:
            assert hp.group_srpoly_bound(G1) == hp.srpoly_bound(M)
    finally:
        M.close()
        for m in G1 or ():
            m.close()


# ---------------------------------------------------------------------------
# 4. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2_3x33x17x9", "p10_csr3", "2x12x10x8_7pt", "4x7x5x1"])
def test_columns_are_single_column_calls(hp, gpu, shape):
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    rng = np.random.default_rng(9)
    # the same tolerance meets differently scaled residuals at different iterations
    B = np.stack([A.b, A.b * 2.0 ** -20, rng.uniform(-1.0, 1.0, N) * 2.0 ** 10, A.b * 2.0 ** -40, A.b])
    X0 = np.zeros((5, N))
    X0[4] = A.xexact  # (ends before its first iteration)
    tol = 1e-8 * float(np.linalg.norm(A.b))
    for degree in (2, 3):
        one = [srpoly_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], 150, tol, degree=degree)[0] for c in range(5)]
        stops = [o[1] for o in one]
        print(f"{shape} degree {degree}: stops {stops}")
        assert len(set(stops)) >= 3 and max(stops) < 149 and stops[4] == 0, stops
        for nrhs, pad in ((5, 5), (4, 0), (3, 0), (2, 0)):
            got = srpoly_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 150, tol, degree=degree, pad=pad)
            assert_same(got, one[:nrhs])
            for g in got[:4]:
                assert len(g[3]) == g[1] + 1 and g[2] == g[3][-1]


# ---------------------------------------------------------------------------
# 5. the halo kernel and the halo by copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "4x7x5x1", "p10_csr3"])
def test_the_halo_kernel_equals_the_copies(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs, 5)
    for degree in (3, 2, 0):
        kernel = srpoly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=degree)
        copies = srpoly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=degree, halo_copies=True)
        assert kernel[0][1] > 0 and all(np.all(np.isfinite(x)) and x.any() for x in kernel[0][0])
        assert_same(kernel, copies)
        assert_same(srpoly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=degree), kernel)  # (the switch is the call's own)


# ---------------------------------------------------------------------------
# 6. the restatement and the group poly
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("shape", ["p10_" + s for s in SHAPES] + ["p10_lap_3x33x17x9"])
def test_the_group_follows_the_restatement_and_the_group_poly(hp, gpu, shape, degree):
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    xs, niters, normr, tr = srpoly_solve(hp, gpu, cs, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    lmin, lmax = hp.group_last_spectrum_srpoly(cs.Ms)
    assert lmax == hp.group_srpoly_bound(cs.Ms) and lmin == lmax / EIG_RATIO, (lmin, lmax)
    _, _, _, tr_ref = restated_srpoly(A, A.b, minv, degree, lmin, lmax, 200)
    assert tr_ref[0] == r0
    checked = check_trace(tr, tr_ref, RTRANS_RTOL_MULTI)
    print(f"{shape} degree {degree}: {checked} trace points checked against the restatement, niters {niters}")
    assert checked >= 10, checked
    _, it_poly, _, tr_poly = tgp.poly_solve(hp, gpu, cs, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    assert check_trace(tr, tr_poly, RTRANS_RTOL_MULTI) >= 10
    assert niters == it_poly, (niters, it_poly)
    x = np.concatenate(xs)
    err = float(np.max(np.abs(x - A.xexact)))
    print(f"{shape} degree {degree}: normr/r0 {normr / r0:.3e} max |x - xexact| {err:.3e}")
    assert normr <= 1e-14 * r0 and niters < 199
    assert err <= 1e-9, err


# ---------------------------------------------------------------------------
# 7. the bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + ["lap_3x33x17x9", "p10_csr3"])
def test_the_bound_is_the_group_polys(hp, gpu, shape):
    import torch
    cs = case(hp, shape)
    ref = hp.group_poly_bound(cs.Ms)
    assert np.float64(hp.group_srpoly_bound(cs.Ms)).tobytes() == np.float64(ref).tobytes()
    assert hp.group_srpoly_bound(cs.Ms) == ref  # (cached)
    m = np.random.default_rng(23).uniform(0.25, 4.0, cs.N)
    ms = [torch.from_numpy(m[rw].copy()).to(gpu) for rw in cs.rows]
    assert np.float64(hp.group_srpoly_bound(cs.Ms, ms)).tobytes() == np.float64(hp.group_poly_bound(cs.Ms, ms)).tobytes()


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["csr3", "2x8c"])
@pytest.mark.parametrize("kind", ["zero", "missing"])
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
                hp.group_HPCCG_srpoly(Ms, Bd, Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError, match=rf"member 1 row {517 - start1} "):
            hp.group_srpoly_bound(Ms)
        assert hp.lib().hpccg_hip_last_error().startswith(b"group srpoly:")
        assert all(torch.all(x == 0.5) for x in Xd)
        # a caller's m is taken on the same members
        ones = [torch.ones(n, dtype=torch.float64, device=gpu) for n in counts]
        its, _, _ = hp.group_HPCCG_srpoly(Ms, Bd, [x.clone() for x in Xd], max_iter=3, minvs=ones)
        assert list(its) == [2, 2]
    finally:
        for M in Ms:
            M.close()


def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.srpoly_group_lib()
    err = hp.lib().hpccg_hip_last_error
    cs = case(hp, "2x8c")
    three = case(hp, "3x33x17x9")
    n = 512
    B, X0 = columns(cs, 2)
    Bd = [dev(gpu, a) for a in cs.split(B)]
    Xd = [dev(gpu, a) for a in cs.split(X0)]
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = srpoly_solve(hp, gpu, cs, B, X0, 10)

    def call(Ms, ldb=(n, n), ldx=(n, n), nrhs=2, max_iter=10, nranks=2, minv=None, degree=2, lmin=0.0, lmax=0.0):
        hs = (C.c_void_p * len(Ms))(*[M.h for M in Ms])
        bp = (C.c_void_p * 2)(*[t.data_ptr() for t in Bd])
        xp = (C.c_void_p * 2)(*[t.data_ptr() for t in Xd])
        mp = None if minv is None else (C.c_void_p * 2)(*[t.data_ptr() for t in minv])
        return L.hpccg_hip_group_srpoly_solve_device(hs, nranks, nrhs, bp, (C.c_longlong * 2)(*ldb), xp,
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
        assert b"gather" in err() and err().startswith(b"group srpoly:")
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
        bound = hp.group_srpoly_bound(cs.Ms)
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
                hp.group_HPCCG_srpoly(cs.Ms, Bd, Xd, max_iter=10, minvs=mv)
            with pytest.raises(hp.HPCCGError, match=r"member 1's minv\[300\]"):
                hp.group_srpoly_bound(cs.Ms, mv)
            assert untouched()
        with pytest.raises(hp.HPCCGError):
            hp.group_HPCCG_srpoly(gather, Bd, Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError):
            hp.group_srpoly_bound(cs.Ms[::-1])
        with pytest.raises(hp.HPCCGError):
            hp.group_last_trace_srpoly(cs.Ms, 2)  # (the last solve had two columns)
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            hp.group_last_spectrum_srpoly(other)
        assert untouched()
        assert torch.cuda.current_device() == dev0
        # the one-rank library keeps refusing a member
        for m in cs.Ms:
            assert hp.srpoly_lib().hpccg_hip_srpoly_solve_device(m.h, 2, Bd[0].data_ptr(), n, Xd[0].data_ptr(), n, None,
                                                                 2, 0.0, 0.0, 10, 0.0, it, nr, None) == EINVAL
            assert b"group" in err()
        assert untouched()
    finally:
        for M in other + gather + [plain]:
            M.close()
    # ... and a good solve afterwards
    assert_same(srpoly_solve(hp, gpu, cs, B, X0, 10), ref)


# ---------------------------------------------------------------------------
# 9. degenerate columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (0, 2))
@pytest.mark.parametrize("shape", ["2x8c", "csr3"])
def test_degenerate_columns(hp, gpu, shape, degree):
    """b = A x0 (a zero initial residual), a NaN in b and an infinite x0 entry,
    the latter two on a plane a neighbour reads: each ends with the classic
    group solve's niters and normr (group_HPCCG_srcg at degree 0, else
    group_HPCCG_poly), the finite columns keep their bits and nothing stays in
    the workspaces."""
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    FB, FX = columns(cs, 5)
    edge = cs.rows[1].start  # member 1's first row: in member 0's upper ghost plane
    e = np.zeros(N)
    e[edge - 1] = 2.0  # (one nonzero: A e is exact in any summation order)
    bad = {"exact": (oracle.sparsemv(A, e), e), "nan_b": (FB[1].copy(), FX[1].copy()),
           "inf_x0": (FB[0].copy(), np.zeros(N))}
    bad["nan_b"][0][edge] = np.nan
    bad["inf_x0"][1][edge - 1] = np.inf
    usual = srpoly_solve(hp, gpu, cs, FB, FX, 20, degree=degree)
    assert usual[0][1] == 19
    alone = {c: srpoly_solve(hp, gpu, cs, FB[c:c + 1], FX[c:c + 1], 20, degree=degree)[0] for c in (0, 3)}
    for halo_copies in (False, True):
        for cols in (("exact", 0, "nan_b", 3, "inf_x0"), ("inf_x0", "nan_b", 0, "exact"), ("nan_b",)):
            B = np.stack([FB[c] if isinstance(c, int) else bad[c][0] for c in cols])
            X0 = np.stack([FX[c] if isinstance(c, int) else bad[c][1] for c in cols])
            got = srpoly_solve(hp, gpu, cs, B, X0, 20, degree=degree, halo_copies=halo_copies)
            if degree == 0:
                ref = tgs.srcg_solve(hp, gpu, cs, B, X0, 20, halo_copies=halo_copies)
            else:
                ref = tgp.poly_solve(hp, gpu, cs, B, X0, 20, degree=degree, halo_copies=halo_copies)
            for c, col in enumerate(cols):
                where = (shape, cols, c, col)
                if isinstance(col, int):
                    assert_same([got[c]], [alone[col]])
                    continue
                assert got[c][1] == ref[c][1] == 0, (where, got[c][1], ref[c][1])
                assert tgs.nan_equal(got[c][2], ref[c][2]), (where, got[c][2], ref[c][2])
                assert math.isnan(got[c][2]) == (col != "exact") and (col != "exact" or got[c][2] == 0.0), where
                for m, rw in enumerate(cs.rows):  # x untouched
                    assert np.array_equal(got[c][0][m], X0[c, rw], equal_nan=True), (where, m)
            assert_same(srpoly_solve(hp, gpu, cs, FB, FX, 20, degree=degree), usual)  # nothing of a bad column stays


# ---------------------------------------------------------------------------
# 10. both non-temporal arms
# ---------------------------------------------------------------------------
# (test_gpu_nt.SHAPES holds one-rank shapes only: the group shapes are test_gpu_srcg_group.py's)
@pytest.mark.parametrize("shape", ["2x8c", "csr3", "2x12x10x8_7pt"])
def test_both_nt_arms_give_the_same_bits(hp, gpu, shape):
    """A chunk whose columns all run takes the arm, one with an ended column
    the general slot loop: both sets of columns, every chunking; degree 3 (u in
    z buffer 1) and degree 2 (u in buffer 0)."""
    cs = case(hp, shape)
    assert [M.get_option("nt") for M in cs.Ms] == [0] * cs.P  # (the automatic flag at these sizes)
    sets = (tn.active_columns(cs.A.b, 4), columns(cs, 4))
    sets[1][1][2] = 0.0  # column 2 starts at its solution (one nonzero: A x0 is exact) and ends in the prologue
    sets[1][1][2, cs.N // 2] = 2.0
    sets[1][0][2] = oracle.sparsemv(cs.A, sets[1][1][2])
    degrees = (3, 2)
    refs = [[srpoly_solve(hp, gpu, cs, B, X0, 25, degree=d) for d in degrees] for B, X0 in sets]
    assert [r[1] for r in refs[0][0]] == [24] * 4 and refs[1][0][2][1] == 0
    try:
        for nt in (1, 0):
            for M in cs.Ms:
                M.set_option("nt", nt)
                assert M.get_option("nt") == nt
            for (B, X0), ref in zip(sets, refs):
                for nrhs in (4, 2, 1):
                    for d, want in zip(degrees, ref):
                        assert_same(srpoly_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 25, degree=d, pad=3), want[:nrhs])
        cs.Ms[0].set_option("nt", 1)  # member 0 alone: members run their own kernels
        assert_same(srpoly_solve(hp, gpu, cs, *sets[0], 25, degree=3), refs[0][0])
    finally:
        for M in cs.Ms:
            M.set_option("nt", -1)
    assert [M.get_option("nt") for M in cs.Ms] == [0] * cs.P
    assert_same(srpoly_solve(hp, gpu, cs, *sets[0], 25, degree=3), refs[0][0])  # nothing of the forced runs stays


# ---------------------------------------------------------------------------
# 11. isolation
# ---------------------------------------------------------------------------
def test_other_solves_and_repeats_are_undisturbed(hp, gpu):
    cs = case(hp, "3x33x17x9")
    B, X0 = columns(cs, 4)

    def others():
        single = tpg.single_solves(hp, gpu, cs, B[:2], X0[:2], 40)
        Bd = [dev(gpu, a) for a in cs.split(B)]
        Xd = [dev(gpu, a) for a in cs.split(X0)]
        its, nrs, _ = hp.group_HPCCG_batch(cs.Ms, Bd, Xd, max_iter=40)
        rest = tpg.pcg_solve(hp, gpu, cs, B, X0, 40) + tgs.srcg_solve(hp, gpu, cs, B, X0, 40) + \
            tgp.poly_solve(hp, gpu, cs, B, X0, 40)
        return single + rest, ([x.cpu().numpy().tobytes() for x in Xd], its.tobytes(), nrs.tobytes())

    try:
        before = others()
        counts = live(hp)
        first = srpoly_solve(hp, gpu, cs, B, X0, 40)
        assert live(hp) == counts
        after = others()
        assert_same(after[0], before[0])
        assert after[1] == before[1]
        for _ in range(3):
            assert_same(srpoly_solve(hp, gpu, cs, B, X0, 40), first)
        # a solve of another degree between two leaves nothing behind (u moves between the z buffers)
        srpoly_solve(hp, gpu, cs, B, X0, 40, degree=3)
        srpoly_solve(hp, gpu, cs, B, X0, 40, degree=0)
        assert_same(srpoly_solve(hp, gpu, cs, B, X0, 40), first)
        assert all(hp.group_srpoly_workspace_bytes(M) > 0 for M in cs.Ms)
    finally:
        for M in cs.Ms:
            M.batch_release()
            hp.group_pcg_release(M)
            hp.group_srcg_release(M)
            hp.group_poly_release(M)


# ---------------------------------------------------------------------------
# 12. the workspace's life
# ---------------------------------------------------------------------------
def test_workspace_goes_with_the_members(hp, gpu):
    base = hp.group_srpoly_live_workspaces()
    others = live(hp)
    cs = tpg.Case(hp, "2x8c")
    try:
        B, X0 = columns(cs, 2)
        first = srpoly_solve(hp, gpu, cs, B, X0, 10)
        assert hp.group_srpoly_live_workspaces() == base + 2
        assert all(hp.group_srpoly_workspace_bytes(M) > 2 * 8 * 512 for M in cs.Ms)
        hp.group_srpoly_release(cs.Ms[1])
        assert hp.group_srpoly_live_workspaces() == base + 1 and hp.group_srpoly_workspace_bytes(cs.Ms[1]) == 0
        assert_same(srpoly_solve(hp, gpu, cs, B, X0, 10), first)  # rebuilt on demand, the caches too
        small = hp.group_srpoly_workspace_bytes(cs.Ms[1])
        srpoly_solve(hp, gpu, cs, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the caches stay
        assert hp.group_srpoly_workspace_bytes(cs.Ms[1]) > small
        assert_same(srpoly_solve(hp, gpu, cs, B, X0, 10), first)
        for M in cs.Ms:
            hp.group_srpoly_release(M)
            hp.group_srpoly_release(M)  # (idempotent)
            assert hp.group_srpoly_workspace_bytes(M) == 0
        assert hp.group_srpoly_live_workspaces() == base
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            hp.group_last_spectrum_srpoly(cs.Ms)
        assert_same(srpoly_solve(hp, gpu, cs, B, X0, 10), first)
        assert hp.group_srpoly_live_workspaces() == base + 2  # ... and closing the members without a release frees them
        assert first[0][1] == 9
        assert live(hp) == others
    finally:
        cs.close()
    assert hp.group_srpoly_live_workspaces() == base
    assert live(hp) == others
