"""Single-reduction preconditioned CG over an in-process rank group
(include/hpccg_hip_srcg_group.h, lib/libhpccg_hip_srcg_group.so): per column
the recurrence of hpccg_hip_srcg.h, every member on its own rows, the ghost
planes of u moved by one kernel per member, the three dots summed over the
members in rank order by one kernel per iteration. All members share one
device.

  1. the first iteration is group_HPCCG_pcg's bit for bit (max_iter 0, 1, 2;
     the trace still at max_iter 3), Jacobi and m = 1: the rank-order sums and
     both halos (of t and of u);
  2. a group of one is bitwise HPCCG_srcg, both image forms;
  3. column c of a multi-column call is bitwise the one-column call, under a
     tolerance that freezes columns part-way too;
  4. m = 2^-3 and m = 2^5 everywhere: the bits of m = 1; Jacobi commutes
     bitwise with a power-of-two scaling;
  5. the halo kernel against the halo by copies: the same bits;
  6. on matrices scaled by s_i = 10^u_i: the trace against one-rank HPCCG_srcg
     of the global matrix and the rank-order restatement; niters and the stop
     under a tolerance against group_HPCCG_pcg and the one-rank solve;
  7. degenerate columns; 8. refusals; 9. both non-temporal arms; 10. the other
     solves are undisturbed and the workspace goes with the members.

Shapes, Case, columns, dev and assert_same: those of test_gpu_pcg_group.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import test_gpu_nt as tn
import test_gpu_pcg_group as tpg
from conftest import RTRANS_RTOL_MULTI, check_trace
from test_gpu_pcg_group import HAS_A, MAX_ITER, SHAPES, Case, assert_same, columns, csr_diagonal, dev, pcg_solve
from test_gpu_poly32_group import rank_dot
from test_gpu_srcg import restated_sr

pytestmark = pytest.mark.gpu

EINVAL, EPLAN = -1, -5

_cases = {}


def case(hp, name):
    if name not in _cases:
        _cases[name] = Case(hp, name)
    return _cases[name]


def live(hp):
    return (hp.group_pcg_live_workspaces(), hp.pcg_live_workspaces(), hp.srcg_live_workspaces(),
            hp.batch_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _close_cases(hp):
    base = hp.group_srcg_live_workspaces()
    others = live(hp)
    yield
    for c in _cases.values():
        c.close()
    _cases.clear()
    assert hp.group_srcg_live_workspaces() == base
    assert live(hp) == others


def srcg_solve(hp, gpu, cs, B, X0, max_iter, tol=0.0, minv=None, pad=0, halo_copies=False):
    """[(xs per member, niters, normr, trace)] per column of a group
    single-reduction solve; minv: None (Jacobi), a number (that value
    everywhere) or a global array (test_gpu_pcg_group.pcg_solve's result)."""
    import torch
    Bd = [dev(gpu, a, pad) for a in cs.split(B)]
    Xd = [dev(gpu, a, pad) for a in cs.split(X0)]
    minvs = None
    if minv is not None:
        m = np.full(cs.N, 1.0) * np.float64(minv)
        minvs = [torch.from_numpy(m[rw].copy()).to(gpu) for rw in cs.rows]
    its, nrs, times = hp.group_HPCCG_srcg(cs.Ms, Bd, Xd, max_iter=max_iter, tolerance=tol, minvs=minvs,
                                          halo_copies=halo_copies)
    assert times[0] > 0.0 and not times[1:].any()
    X = [x.cpu().numpy() for x in Xd]
    if pad:
        for x, rw in zip(X, cs.rows):
            assert np.all(x[:, rw.stop - rw.start:] == 7.5)  # nothing stored between the columns
    return [([x[c, :rw.stop - rw.start].copy() for x, rw in zip(X, cs.rows)], int(its[c]), float(nrs[c]),
             hp.group_last_trace_srcg(cs.Ms, c).copy()) for c in range(B.shape[0])]


# ---------------------------------------------------------------------------
# 1. the first iteration
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + ["p2_3x33x17x9", "p2_csr3", "p10_4x7x5x1", "p10_2x12x10x8_7pt"])
def test_the_first_iteration_is_group_pcgs(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs)
    assert B.shape[0] == 7 and X0[1].any() and X0[3].any()  # nonzero x0 among them
    for minv in (None, 1.0):
        for max_iter in (0, 1, 2):
            ref = pcg_solve(hp, gpu, cs, B, X0, max_iter, minv=minv)
            assert_same(srcg_solve(hp, gpu, cs, B, X0, max_iter, minv=minv), ref)
            assert max(r[1] for r in ref) == max(max_iter, 1) - 1
        ref = pcg_solve(hp, gpu, cs, B, X0, 3, minv=minv)
        got = srcg_solve(hp, gpu, cs, B, X0, 3, minv=minv)
        for c in range(7):
            assert got[c][1] == ref[c][1] == 2 and got[c][3].tobytes() == ref[c][3].tobytes(), (minv, c)


# ---------------------------------------------------------------------------
# 2. a group of one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["a_image", "sell"])
def test_group_of_one_is_the_one_rank_solve(hp, gpu, form):
    """nranks == 1 runs the same code on a halo-free matrix: 0.0 + a total is
    the total, so every column is bitwise HPCCG_srcg's."""
    if form == "a_image":
        A = oracle.generate(12, 11, 10)
        M = hp.Matrix.generate(12, 11, 10)
    else:
        A = tpg.random_spd(np.random.default_rng(11), 1300, 6, 40)
        M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    try:
        assert M.get_option("has_a") == int(form == "a_image")
        rng = np.random.default_rng(3)
        B = np.stack([A.b, rng.uniform(-1.0, 1.0, A.nrow), 0.5 * A.b])
        for nrhs in (3, 1):
            Bd, Xd = dev(gpu, B[:nrhs]), dev(gpu, np.zeros_like(B[:nrhs]))
            its, nrs, _ = hp.group_HPCCG_srcg([M], [Bd], [Xd], max_iter=MAX_ITER)
            Xs = dev(gpu, np.zeros_like(B[:nrhs]))
            _, its1, nrs1, _ = hp.HPCCG_srcg(M, Bd, Xs, max_iter=MAX_ITER, device=True)
            assert list(its) == list(its1) and max(its) == MAX_ITER - 1 and nrs.tobytes() == nrs1.tobytes()
            assert Xd.cpu().numpy().tobytes() == Xs.cpu().numpy().tobytes()
            for c in range(nrhs):
                assert hp.group_last_trace_srcg([M], c).tobytes() == M.last_trace_srcg(c).tobytes()
    finally:
        M.close()


# ---------------------------------------------------------------------------
# 3. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_columns_are_single_column_calls(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs)

    def ones(tol):
        return [srcg_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], MAX_ITER, tol)[0] for c in range(7)]

    full = ones(0.0)
    assert full[0][1] > 0 and all(np.all(np.isfinite(x)) for x in full[0][0])
    # a tolerance that column 0 meets part-way: just above the smallest residual of its first half
    tr0 = full[0][3]
    tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10)
    part = ones(tol)
    print(f"{shape}: stops {[r[1] for r in part]} under the tolerance, {[r[1] for r in full]} without")
    assert part[0][1] < full[0][1], (part[0][1], full[0][1])
    for t, ref in ((0.0, full), (tol, part)):
        for nrhs, pad in ((7, 0), (5, 0), (4, 0), (3, 3), (2, 0), (1, 0)):
            assert_same(srcg_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, t, pad=pad), ref[:nrhs])


# ---------------------------------------------------------------------------
# 4. exact scaling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "2x12x10x8_7pt", "csr3"])
def test_a_uniform_power_of_two_m_is_m_one(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs, 5)
    ref = srcg_solve(hp, gpu, cs, B, X0, MAX_ITER, minv=1.0)
    assert ref[0][1] > 0
    for m in (2.0 ** -3, 2.0 ** 5):
        for nrhs in (5, 1):
            assert_same(srcg_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, minv=m), ref[:nrhs])


@pytest.mark.parametrize("shape", ["3x33x17x9", "csr3"])
def test_jacobi_commutes_with_a_power_of_two_scaling(hp, gpu, shape):
    cs, css = case(hp, shape), case(hp, "p2_" + shape)
    assert cs.has_a == css.has_a == HAS_A[shape]
    s, N = css.s, cs.N
    rng = np.random.default_rng(3)
    B = np.stack([cs.A.b, rng.uniform(-1.0, 1.0, N), cs.A.b * 2.0 ** -7, rng.uniform(-1.0, 1.0, N)])
    X0 = np.zeros((4, N))
    for nrhs in (4, 1, 2):
        got = srcg_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 20)
        gots = srcg_solve(hp, gpu, css, B[:nrhs] * s, X0[:nrhs], 20)
        for c in range(nrhs):
            assert got[c][1] == gots[c][1] == 19
            for m, rw in enumerate(cs.rows):
                x, xs = got[c][0][m], gots[c][0][m] * s[rw]
                assert xs.tobytes() == x.tobytes(), (nrhs, c, m, float(np.max(np.abs(xs - x))))
                assert np.all(np.isfinite(x)) and x.any()


# ---------------------------------------------------------------------------
# 5. the halo kernel and the halo by copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "4x7x5x1", "p10_csr3"])
def test_the_halo_kernel_equals_the_copies(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs, 5)
    kernel = srcg_solve(hp, gpu, cs, B, X0, MAX_ITER)
    copies = srcg_solve(hp, gpu, cs, B, X0, MAX_ITER, halo_copies=True)
    assert kernel[0][1] > 0 and all(np.all(np.isfinite(x)) for x in kernel[0][0])
    assert_same(kernel, copies)
    assert_same(srcg_solve(hp, gpu, cs, B, X0, MAX_ITER), kernel)  # (the switch is the call's own)


# ---------------------------------------------------------------------------
# 6. the group against one rank, the restatement and the group pcg
# ---------------------------------------------------------------------------
# The restatement with the members' sequential dots added in rank order agrees
# with the classic one and with itself under the sequential dot to 8.2e-11 at
# worst on the checked part (tests/test_srcg_group_cpu.py): a thousandth of
# RTRANS_RTOL_MULTI, so the bound has room for what the dots' summation shapes
# cost and for nothing else.
@pytest.mark.parametrize("shape", SHAPES)
def test_group_srcg_follows_one_rank_the_restatement_and_group_pcg(hp, gpu, shape):
    cs = case(hp, "p10_" + shape)
    A, N = cs.A, cs.N
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    M1 = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    try:
        def one_rank(tol, max_iter=MAX_ITER):
            Bd, Xd = dev(gpu, B), dev(gpu, X0)
            _, its, nrs, _ = hp.HPCCG_srcg(M1, Bd, Xd, max_iter=max_iter, tolerance=tol, device=True)
            return Xd.cpu().numpy()[0], int(its[0]), float(nrs[0]), M1.last_trace_srcg(0).copy()

        x1, it1, nr1, tr1 = one_rank(0.0)
        xs, it, nr, tr = srcg_solve(hp, gpu, cs, B, X0, MAX_ITER)[0]
        checked = check_trace(tr, tr1, RTRANS_RTOL_MULTI)
        _, _, _, tr_ref = restated_sr(A, A.b, 1.0 / csr_diagonal(A), MAX_ITER, dot=rank_dot(cs.rows))
        checked_ref = check_trace(tr, tr_ref, RTRANS_RTOL_MULTI)
        print(f"{shape}: {checked} trace points checked against one rank, {checked_ref} against the restatement, "
              f"niters {it} / {it1}")
        assert checked >= 10 and checked_ref >= 10, (checked, checked_ref)
        # converged is normr <= 1e-10 r0: group_HPCCG_pcg's count
        r0 = float(tr1[0])
        _, itc, nrc, _ = srcg_solve(hp, gpu, cs, B, X0, 200, 1e-10 * r0)[0]
        _, itp, nrp, _ = pcg_solve(hp, gpu, cs, B, X0, 200, 1e-10 * r0)[0]
        print(f"{shape}: {itc} iterations to 1e-10 r0 (group pcg {itp}), normr/r0 {nrc / r0:.3e} ({nrp / r0:.3e})")
        assert itc == itp and 0 < itc < 199 and nrc <= 1e-10 * r0, (itc, itp, nrc / r0)
        # a tolerance between two residuals of the one-rank solve (the widest
        # gap in the middle third of the checked part): the same stop
        lo, hi = checked // 3, 2 * checked // 3
        k = lo + int(np.argmax(tr1[lo:hi] / tr1[lo + 1:hi + 1]))
        assert tr1[k] > 1.01 * tr1[k + 1], (k, tr1[k], tr1[k + 1])
        tol = float(np.sqrt(tr1[k] * tr1[k + 1]))
        _, it1t, nr1t, _ = one_rank(tol)
        _, itt, nrt, _ = srcg_solve(hp, gpu, cs, B, X0, MAX_ITER, tol)[0]
        _, itpt, nrpt, _ = pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, tol)[0]
        assert itt == it1t == itpt and 0 < itt < it, (itt, it1t, itpt, it)
        assert abs(nrt - nr1t) <= RTRANS_RTOL_MULTI * nr1t, (nrt, nr1t)
        assert abs(nrt - nrpt) <= RTRANS_RTOL_MULTI * nrpt, (nrt, nrpt)
    finally:
        M1.close()


# ---------------------------------------------------------------------------
# 7. degenerate columns
# ---------------------------------------------------------------------------
def nan_equal(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("shape", ["2x8c", "csr3"])
def test_degenerate_columns(hp, gpu, shape):
    """b = A x0 (a zero initial residual), a NaN in b and an infinite x0 entry,
    the latter two on a plane a neighbour reads: each ends with
    group_HPCCG_pcg's niters and normr, the finite columns keep their bits and
    nothing stays in the workspaces."""
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
    usual = srcg_solve(hp, gpu, cs, FB, FX, 20)
    assert usual[0][1] == 19
    alone = {c: srcg_solve(hp, gpu, cs, FB[c:c + 1], FX[c:c + 1], 20)[0] for c in (0, 3)}
    for halo_copies in (False, True):
        for cols in (("exact", 0, "nan_b", 3, "inf_x0"), ("inf_x0", "nan_b", 0, "exact"), ("nan_b",)):
            B = np.stack([FB[c] if isinstance(c, int) else bad[c][0] for c in cols])
            X0 = np.stack([FX[c] if isinstance(c, int) else bad[c][1] for c in cols])
            got = srcg_solve(hp, gpu, cs, B, X0, 20, halo_copies=halo_copies)
            ref = pcg_solve(hp, gpu, cs, B, X0, 20, halo_copies=halo_copies)
            for c, col in enumerate(cols):
                where = (shape, cols, c, col)
                if isinstance(col, int):
                    assert_same([got[c]], [alone[col]])
                    continue
                assert got[c][1] == ref[c][1] == 0, (where, got[c][1], ref[c][1])
                assert nan_equal(got[c][2], ref[c][2]), (where, got[c][2], ref[c][2])
                assert math.isnan(got[c][2]) == (col != "exact") and (col != "exact" or got[c][2] == 0.0), where
                for m, rw in enumerate(cs.rows):  # x untouched
                    assert np.array_equal(got[c][0][m], X0[c, rw], equal_nan=True), (where, m)
            assert_same(srcg_solve(hp, gpu, cs, FB, FX, 20), usual)  # nothing of a bad column stays


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["csr3", "2x8c"])
@pytest.mark.parametrize("kind", ["zero", "missing"])
def test_a_bad_diagonal_on_one_member_is_refused(hp, gpu, shape, kind):
    import torch
    A0, counts = tpg.global_matrix(shape)
    start1 = counts[0]
    A = tpg.finish(*tpg._edited(A0, tpg.BAD[kind]))
    Ms = tpg.members_from_csr(hp, A, counts)
    try:
        Bd = [torch.ones((2, n), dtype=torch.float64, device=gpu) for n in counts]
        Xd = [torch.full((2, n), 0.5, dtype=torch.float64, device=gpu) for n in counts]
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match=rf"\(-1\): group srcg:.*member 1 row {517 - start1} "):
                hp.group_HPCCG_srcg(Ms, Bd, Xd, max_iter=10)
        assert all(torch.all(x == 0.5) for x in Xd)
        # a caller's m is taken on the same members
        ones = [torch.ones(n, dtype=torch.float64, device=gpu) for n in counts]
        its, _, _ = hp.group_HPCCG_srcg(Ms, Bd, [x.clone() for x in Xd], max_iter=3, minvs=ones)
        assert list(its) == [2, 2]
    finally:
        for M in Ms:
            M.close()


def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.srcg_group_lib()
    err = hp.lib().hpccg_hip_last_error
    cs = case(hp, "2x8c")
    three = case(hp, "3x33x17x9")
    n = 512
    B, X0 = columns(cs, 2)
    Bd = [dev(gpu, a) for a in cs.split(B)]
    Xd = [dev(gpu, a) for a in cs.split(X0)]
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = srcg_solve(hp, gpu, cs, B, X0, 10)

    def call(Ms, ldb=(n, n), ldx=(n, n), nrhs=2, max_iter=10, nranks=2, minv=None):
        hs = (C.c_void_p * len(Ms))(*[M.h for M in Ms])
        bp = (C.c_void_p * 2)(*[t.data_ptr() for t in Bd])
        xp = (C.c_void_p * 2)(*[t.data_ptr() for t in Xd])
        mp = None if minv is None else (C.c_void_p * 2)(*[t.data_ptr() for t in minv])
        return L.hpccg_hip_group_srcg_solve_device(hs, nranks, nrhs, bp, (C.c_longlong * 2)(*ldb), xp,
                                                   (C.c_longlong * 2)(*ldx), mp, max_iter, 0.0, it, nr, None)

    def untouched():
        return all(x.cpu().numpy().tobytes() == a.tobytes() for x, a in zip(Xd, cs.split(X0)))

    def still_the_first():
        assert untouched()
        assert_same(srcg_solve(hp, gpu, cs, B, X0, 10), ref)

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
        assert call(cs.Ms[::-1]) == EINVAL  # the wrong order
        assert b"rank" in err() and err().startswith(b"group srcg:")
        assert call(three.Ms[:2]) == EINVAL  # a wrong nranks: a subset of a group
        assert call(cs.Ms, nranks=1) == EINVAL
        assert call([plain, plain]) == EINVAL  # a single-rank matrix in a 2-slot call
        assert call([cs.Ms[0], other[1]]) == EINVAL  # members of two groups
        assert b"another group" in err()
        still_the_first()
        assert call(gather) == EPLAN
        assert b"gather" in err() and err().startswith(b"group srcg:")
        with pytest.raises(hp.HPCCGError, match="gather"):
            hp.group_HPCCG_srcg(gather, Bd, Xd, max_iter=10)
        still_the_first()
        assert call(cs.Ms, ldb=(n, n - 1)) == EINVAL
        assert b"leading dimension" in err()
        assert call(cs.Ms, ldx=(n - 1, n)) == EINVAL
        assert call(cs.Ms, nrhs=0) == EINVAL
        assert call(cs.Ms, max_iter=-1) == EINVAL
        still_the_first()
        # a caller's m with a bad entry on the last member
        for bad in (0.0, float("nan"), -1.0, float("inf")):
            mv = [torch.ones(n, dtype=torch.float64, device=gpu) for _ in range(2)]
            mv[1][300] = bad
            mv[1][411] = bad
            assert call(cs.Ms, minv=mv) == EINVAL
            assert b"group srcg: member 1's minv[300]" in err(), err()
            with pytest.raises(hp.HPCCGError, match=r"member 1's minv\[300\]"):
                hp.group_HPCCG_srcg(cs.Ms, Bd, Xd, max_iter=10, minvs=mv)
            assert untouched()
        still_the_first()
        # mismatched column counts
        with pytest.raises(hp.HPCCGError, match="columns"):
            hp.group_HPCCG_srcg(cs.Ms, Bd, [x[:1] for x in Xd], max_iter=10)
        with pytest.raises(hp.HPCCGError, match="column sets"):
            hp.group_HPCCG_srcg(cs.Ms, Bd[:1], Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError):
            hp.group_last_trace_srcg(cs.Ms, 2)  # (the last solve had two columns)
        still_the_first()
        assert torch.cuda.current_device() == dev0
        # the one-rank library keeps refusing a member
        for m in cs.Ms:
            assert hp.srcg_lib().hpccg_hip_srcg_solve_device(m.h, 2, Bd[0].data_ptr(), n, Xd[0].data_ptr(), n, None, 10,
                                                             0.0, it, nr, None) == EINVAL
            assert b"group" in err()
        assert untouched()
    finally:
        for M in other + gather + [plain]:
            M.close()
    # ... and a good solve afterwards
    assert_same(srcg_solve(hp, gpu, cs, B, X0, 10), ref)


# ---------------------------------------------------------------------------
# 9. both non-temporal arms
# ---------------------------------------------------------------------------
# (test_gpu_nt.SHAPES holds one-rank shapes only: the group shapes are these)
@pytest.mark.parametrize("shape", ["2x8c", "csr3", "2x12x10x8_7pt"])
def test_both_nt_arms_give_the_same_bits(hp, gpu, shape):
    """A chunk whose columns all run takes the arm, one with an ended column
    the general slot loop: both sets of columns, every chunking."""
    cs = case(hp, shape)
    assert [M.get_option("nt") for M in cs.Ms] == [0] * cs.P  # (the automatic flag at these sizes)
    sets = (tn.active_columns(cs.A.b, 4), columns(cs, 4))
    sets[1][1][2] = 0.0  # column 2 starts at its solution (one nonzero: A x0 is exact) and ends in the prologue
    sets[1][1][2, cs.N // 2] = 2.0
    sets[1][0][2] = oracle.sparsemv(cs.A, sets[1][1][2])
    refs = [[srcg_solve(hp, gpu, cs, B, X0, 25, minv=m) for m in (None, 1.0)] for B, X0 in sets]
    assert [r[1] for r in refs[0][0]] == [24] * 4 and refs[1][0][2][1] == 0
    try:
        for nt in (1, 0):
            for M in cs.Ms:
                M.set_option("nt", nt)
                assert M.get_option("nt") == nt
            for (B, X0), ref in zip(sets, refs):
                for nrhs in (4, 2, 1):
                    for m, want in zip((None, 1.0), ref):
                        assert_same(srcg_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 25, minv=m, pad=3), want[:nrhs])
        cs.Ms[0].set_option("nt", 1)  # member 0 alone: members run their own kernels
        assert_same(srcg_solve(hp, gpu, cs, *sets[0], 25), refs[0][0])
    finally:
        for M in cs.Ms:
            M.set_option("nt", -1)
    assert [M.get_option("nt") for M in cs.Ms] == [0] * cs.P
    assert_same(srcg_solve(hp, gpu, cs, *sets[0], 25), refs[0][0])  # nothing of the forced runs stays


# ---------------------------------------------------------------------------
# 10. other solves and the workspace's life
# ---------------------------------------------------------------------------
def test_other_solves_and_repeats_are_undisturbed(hp, gpu):
    cs = case(hp, "3x33x17x9")
    B, X0 = columns(cs, 4)
    prob = hp.generate_matrix(16, 16, 16)
    M1 = hp.Matrix.from_hpc(prob)
    B1, X1 = np.stack([prob.b, 0.5 * prob.b]), np.zeros((2, len(prob.b)))
    prob.close()

    def others():
        group_pcg = pcg_solve(hp, gpu, cs, B, X0, 40)
        Bd = [dev(gpu, a) for a in cs.split(B)]
        Xd = [dev(gpu, a) for a in cs.split(X0)]
        its, nrs, _ = hp.group_HPCCG_batch(cs.Ms, Bd, Xd, max_iter=40)
        b1, x1 = dev(gpu, B1), dev(gpu, X1)
        _, it1, nr1, _ = hp.HPCCG_srcg(M1, b1, x1, max_iter=40, device=True)
        return group_pcg, ([x.cpu().numpy().tobytes() for x in Xd], its.tobytes(), nrs.tobytes(),
                           x1.cpu().numpy().tobytes(), it1.tobytes(), nr1.tobytes())

    try:
        before = others()
        counts = live(hp)
        first = srcg_solve(hp, gpu, cs, B, X0, 40)
        assert live(hp) == counts
        after = others()
        assert_same(after[0], before[0])
        assert after[1] == before[1]
        for _ in range(3):
            assert_same(srcg_solve(hp, gpu, cs, B, X0, 40), first)
        assert all(hp.group_srcg_workspace_bytes(M) > 0 for M in cs.Ms)
        assert M1.srcg_workspace_bytes() > 0 and hp.group_srcg_workspace_bytes(M1) == 0
    finally:
        M1.close()
        for M in cs.Ms:
            M.batch_release()
            hp.group_pcg_release(M)


def test_workspace_goes_with_the_members(hp, gpu):
    base = hp.group_srcg_live_workspaces()
    others = live(hp)
    cs = Case(hp, "2x8c")
    try:
        B, X0 = columns(cs, 2)
        first = srcg_solve(hp, gpu, cs, B, X0, 10)
        assert hp.group_srcg_live_workspaces() == base + 2
        assert all(hp.group_srcg_workspace_bytes(M) > 2 * 8 * 512 for M in cs.Ms)
        hp.group_srcg_release(cs.Ms[1])
        assert hp.group_srcg_live_workspaces() == base + 1 and hp.group_srcg_workspace_bytes(cs.Ms[1]) == 0
        assert_same(srcg_solve(hp, gpu, cs, B, X0, 10), first)  # rebuilt on demand, the Jacobi cache too
        small = hp.group_srcg_workspace_bytes(cs.Ms[1])
        srcg_solve(hp, gpu, cs, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the cache stays
        assert hp.group_srcg_workspace_bytes(cs.Ms[1]) > small
        assert_same(srcg_solve(hp, gpu, cs, B, X0, 10), first)  # (p and s of the larger call are never read)
        for M in cs.Ms:
            hp.group_srcg_release(M)
            hp.group_srcg_release(M)  # (idempotent)
            assert hp.group_srcg_workspace_bytes(M) == 0
        assert hp.group_srcg_live_workspaces() == base
        assert_same(srcg_solve(hp, gpu, cs, B, X0, 10), first)
        assert hp.group_srcg_live_workspaces() == base + 2
        assert first[0][1] == 9
        assert live(hp) == others
    finally:
        cs.close()
    assert hp.group_srcg_live_workspaces() == base
    assert live(hp) == others
