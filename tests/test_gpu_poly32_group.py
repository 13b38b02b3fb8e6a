"""Chebyshev polynomial preconditioned CG over an in-process rank group whose
polynomial steps stream every member's fp32 image
(include/hpccg_hip_poly32_group.h, lib/libhpccg_hip_poly32_group.so): the
recurrence of hpccg_hip_poly_group.h with A~ = fl32(A) inside the polynomial on
every member, the outer SpMM of a member from its fp32 image only where that
image is the member's rows. All members share one device.

  1. group_poly32_info's verdict, count and bytes per member are NumPy's;
  2. where every member's image is exact every column is group_HPCCG_poly bit
     for bit, degrees 0 to 4;
  3. degree 0 is the group pcg bit for bit on every inexact image;
  4. a group of one is HPCCG_poly32 bit for bit, exact and inexact, with its
     spectrum and bound;
  5. column c of a multi-column call is bitwise its single-column call;
  6. the halo kernel against the halo by copies: the same bits;
  7. the option "nt" forced to 0 and to 1: the same bits;
  8. members that differ in exactness;
  9. on inexact images: the NumPy restatement with A~ inside P under the
     rank-order dot, the one-rank HPCCG_poly32 of the global matrix, niters
     under a tolerance, x against xexact, degrees 1 to 4; not group_HPCCG_poly;
 10. it keeps what the polynomial is for; 11. degenerate columns;
 12. refusals; 13. the other solves are undisturbed, the workspace's life.

Shapes and helpers: those of test_gpu_pcg_group.py (Case, SHAPES),
test_gpu_poly_group.py (make_case with the "lap_" forms, poly_solve) and
test_gpu_poly32.py (restated32, fl32). csr3's entries are random doubles, so
its image and its "p2_" form's are inexact (NumPy says so, and info agrees):
they stand with the inexact shapes in 1. and 3., and the exact int32-column
image of 2. is "dyadic_csr3", csr3 with every entry rounded to a multiple of
2^-8, plain and in its "p2_" form.

9.: the bar is RTRANS_RTOL_1GPU (1e-8) on rtrans with at least 10 points
checked, on the 28 shape/degree pairs. Measured on the CPU for these pairs: the
restatement agrees with itself under three dot orders (oracle.ddot, np.dot, the
members' slabs summed sequentially and added in rank order) to 1.7e-11 or
better, 1/580 of the bar, and keeps 11 to 43 points with equal niters; the
fp64-stepped restatement (test_gpu_poly.restated) differs from it at its worst
kept point by 3.9e-8 to 1.7e-5, at least 3.9 times the bar on every pair
(smallest at p10_8x16c, degree 4), so a build that streamed fp64 values in the
steps misses the bar on all 28 pairs. No pair has been moved to
RTRANS_RTOL_MULTI.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
import test_gpu_pcg_group as tpg
import test_gpu_poly_group as tpolyg
from conftest import RTRANS_RTOL_1GPU, RTRANS_RTOL_MULTI, check_trace
from test_gpu_pcg_group import SHAPES, assert_same, columns, csr_diagonal, dev, finish, scaled
from test_gpu_poly32 import fl32, restated32

pytestmark = pytest.mark.gpu

EINVAL, EPLAN = -1, -5
MAX_ITER = 60
EIG_RATIO = 30.0
DEGREES = (1, 2, 3, 4)
LAP27 = ["lap_2x8c", "lap_8x16c", "lap_3x33x17x9", "lap_4x7x5x1"]
# csr3's entries are uniform random doubles, so its image (and its "p2_" form's) is inexact; the exact int32-column
# image is "dyadic_csr3": csr3 with every entry rounded to a multiple of 2^-8 (still symmetric and strictly
# diagonally dominant: the diagonal's margin is at least 0.5, six neighbours move by 2^-9 at most each)
STENCIL_SHAPES = [s for s in SHAPES if s != "csr3"]
DYADIC = "dyadic_csr3"
EXACT = STENCIL_SHAPES + [DYADIC] + ["p2_" + s for s in STENCIL_SHAPES + [DYADIC]] + LAP27
P10 = ["p10_" + s for s in SHAPES]
INEXACT = P10 + ["p10_lap_3x33x17x9"]
MIXED = "mixed_2x8c"


# ---------------------------------------------------------------------------
# problems: test_gpu_poly_group.make_case, and 2 x 8^3 with member 0 exact and
# member 1 not
# ---------------------------------------------------------------------------
def mixed_case(hp):
    """2x8c scaled symmetrically by s_i = 2^e_i on all of slab 0 and the first
    plane of slab 1 (every row a row of member 0 touches) and s_i = 10^u_i on
    the remaining rows: member 0's rows hold float-exact values only, member
    1's do not."""
    A0, counts = tpg.global_matrix("2x8c")
    N = A0.nrow
    rng = np.random.default_rng(77)
    s = np.where(np.arange(N) < 512 + 64, 2.0 ** rng.integers(-6, 7, N), 10.0 ** rng.uniform(-1.5, 1.5, N))
    cs = object.__new__(tpg.Case)
    cs.s = s
    cs.A = scaled(A0, s)
    cs.Ms = tpg.members_from_csr(hp, cs.A, counts)
    cs.has_a = 1
    assert [M.get_option("has_a") for M in cs.Ms] == [1, 1]
    cs.P = 2
    cs.rows = [slice(0, 512), slice(512, 1024)]
    cs.N = N
    return cs


def dyadic_case(hp, name):
    """csr3 in its slabs with every entry a multiple of 2^-8 (float-exact), and its "p2_" form."""
    A0, counts = tpg.global_matrix("csr3")
    A = finish(A0.row_ptr, A0.cols, np.round(A0.vals * 256.0) / 256.0)
    cs = object.__new__(tpg.Case)
    cs.s = tpg.scale_of("p2", A.nrow) if name.startswith("p2_") else None
    cs.A = scaled(A, cs.s) if cs.s is not None else A
    cs.Ms = tpg.members_from_csr(hp, cs.A, counts)
    cs.has_a = 0
    assert [M.get_option("has_a") for M in cs.Ms] == [0] * len(counts), name  # the int32-column image
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
        if name == MIXED:
            _cases[name] = mixed_case(hp)
        elif name.endswith(DYADIC):
            _cases[name] = dyadic_case(hp, name)
        else:
            _cases[name] = tpolyg.make_case(hp, name)
    return _cases[name]


def live(hp):
    return (hp.group_poly_live_workspaces(), hp.group_pcg_live_workspaces(), hp.pcg_live_workspaces(),
            hp.batch_live_workspaces(), hp.poly_live_workspaces(), hp.poly32_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _close_cases(hp):
    base = hp.group_poly32_live_workspaces()
    others = live(hp)
    yield
    for c in _cases.values():
        c.close()
    _cases.clear()
    assert hp.group_poly32_live_workspaces() == base
    assert live(hp) == others


def poly32_solve(hp, gpu, cs, B, X0, max_iter, tol=0.0, degree=2, lmin=None, lmax=None, minv=None, pad=0,
                 halo_copies=False):
    """[(xs per member, niters, normr, trace)] per column of a group poly32
    solve; minv: None (Jacobi), a number (that value everywhere) or a global array."""
    import torch
    Bd = [dev(gpu, a, pad) for a in cs.split(B)]
    Xd = [dev(gpu, a, pad) for a in cs.split(X0)]
    minvs = None
    if minv is not None:
        m = np.full(cs.N, 1.0) * np.float64(minv)
        minvs = [torch.from_numpy(m[rw].copy()).to(gpu) for rw in cs.rows]
    its, nrs, times = hp.group_HPCCG_poly32(cs.Ms, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, minvs=minvs,
                                            max_iter=max_iter, tolerance=tol, halo_copies=halo_copies)
    assert times[0] > 0.0 and not times[1:].any()
    X = [x.cpu().numpy() for x in Xd]
    if pad:
        for x, rw in zip(X, cs.rows):
            assert np.all(x[:, rw.stop - rw.start:] == 7.5)  # nothing stored between the columns
    return [([x[c, :rw.stop - rw.start].copy() for x, rw in zip(X, cs.rows)], int(its[c]), float(nrs[c]),
             hp.group_last_trace_poly32(cs.Ms, c).copy()) for c in range(B.shape[0])]


def inexact_counts(cs):
    """Per member: NumPy's count of the stored values of its rows that do not
    survive double -> float -> double."""
    A = cs.A
    bad = fl32(A).vals != A.vals
    return [int(np.count_nonzero(bad[int(A.row_ptr[rw.start]):int(A.row_ptr[rw.stop])])) for rw in cs.rows]


def rank_dot(rows):
    """The group's dot on the CPU: the sequential sums of the members' slabs added in rank order from 0.0."""
    def dot(x, y):
        v = np.float64(0.0)
        for rw in rows:
            v = v + np.float64(oracle.ddot(x[rw], y[rw]))
        return v
    return dot


# ---------------------------------------------------------------------------
# 1. info
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EXACT + INEXACT + ["csr3", "p2_csr3", "p10_lap_2x8c"])
def test_info_is_numpys_per_member(hp, gpu, shape):
    cs = case(hp, shape)
    info = hp.group_poly32_info(cs.Ms)
    want = inexact_counts(cs)
    assert len(info) == cs.P
    for r, (i, w, M) in enumerate(zip(info, want, cs.Ms)):
        assert i["inexact_values"] == w, (shape, r, i, w)
        assert i["exact"] == (1 if shape in EXACT else 0), (shape, r, i)
        # 4 bytes per stored slot of the image the member holds: whole slices of 512 rows
        assert i["image_bytes"] % (4 * 512) == 0, (shape, r, i)
        nnz = int(cs.A.row_ptr[cs.rows[r].stop] - cs.A.row_ptr[cs.rows[r].start])
        assert i["image_bytes"] >= 4 * nnz
        if M.get_option("has_a") and M.get_option("a_width") > 0:
            nslices = (M.info()["nrow"] + 511) // 512
            assert i["image_bytes"] == 4 * M.get_option("a_width") * nslices * 512, (shape, r, i)
        assert hp.group_poly32_workspace_bytes(M) >= i["image_bytes"]
    if shape not in EXACT:
        assert all(w > 0 for w in want), (shape, want)
    assert hp.group_poly32_info(cs.Ms) == info  # (built once)


# ---------------------------------------------------------------------------
# 2. exact images: the fp64 group polynomial, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EXACT)
def test_exact_images_are_the_fp64_group_polynomial(hp, gpu, shape):
    cs = case(hp, shape)
    assert all(i["exact"] == 1 for i in hp.group_poly32_info(cs.Ms))
    B, X0 = columns(cs, 5)
    assert X0[1].any() and X0[3].any()  # nonzero x0 among them
    for degree in range(5):
        ref = tpolyg.poly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=degree, pad=3)
        spectrum = hp.group_last_spectrum_poly(cs.Ms)
        assert ref[0][1] > 0
        assert_same(poly32_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=degree, pad=3), ref)
        assert hp.group_last_spectrum_poly32(cs.Ms) == spectrum
        if degree not in (0, 3):
            continue
        # a tolerance that column 0 meets part-way, one iteration and none at all
        tr0 = ref[0][3]
        tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10)
        for max_iter, t in ((MAX_ITER, tol), (1, 0.0), (0, 0.0)):
            part = tpolyg.poly_solve(hp, gpu, cs, B, X0, max_iter, t, degree=degree, pad=3)
            if t:
                assert part[0][1] < ref[0][1], (part[0][1], ref[0][1])
            assert_same(poly32_solve(hp, gpu, cs, B, X0, max_iter, t, degree=degree, pad=3), part)
    # a caller's m, one column
    m = np.random.default_rng(23).uniform(0.25, 4.0, cs.N)
    assert_same(poly32_solve(hp, gpu, cs, B[:1], X0[:1], 20, degree=2, minv=m),
                tpolyg.poly_solve(hp, gpu, cs, B[:1], X0[:1], 20, degree=2, minv=m))
    assert hp.group_poly32_bound(cs.Ms) == hp.group_poly_bound(cs.Ms)


# ---------------------------------------------------------------------------
# 3. degree 0 is the group pcg, whatever the images
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P10 + ["csr3", "p2_csr3"])
def test_degree_0_is_the_group_pcg_on_inexact_images(hp, gpu, shape):
    """... so a member's outer SpMM streams the fp64 values where its image is not its rows."""
    cs = case(hp, shape)
    assert all(i["exact"] == 0 for i in hp.group_poly32_info(cs.Ms))
    B, X0 = columns(cs, 5)
    for minv in (None, 1.0):
        ref = tpg.pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, minv=minv)
        assert ref[0][1] > 0
        for nrhs, pad in ((5, 3), (4, 0), (2, 0), (1, 0)):
            assert_same(poly32_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, degree=0, minv=minv, pad=pad),
                        ref[:nrhs])
    assert_same(poly32_solve(hp, gpu, cs, B, X0, 1, degree=0), tpg.pcg_solve(hp, gpu, cs, B, X0, 1))


# ---------------------------------------------------------------------------
# 4. a group of one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "p10"])
def test_group_of_one_is_the_one_rank_poly32(hp, gpu, kind):
    """nranks == 1 runs the same code on a halo-free matrix: 0.0 + a total is
    the total, so every column is bitwise HPCCG_poly32's."""
    A = oracle.generate(8, 8, 16)  # (2x8c's global matrix)
    if kind == "exact":
        M = hp.Matrix.generate(8, 8, 16)
        groups = [[M], hp.group_generate(8, 8, 16, 1)]
    else:
        A = scaled(A, tpg.scale_of("p10", A.nrow))
        M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
        groups = [[M], hp.group_from_csr([(A.row_ptr, A.cols, A.vals, 0)], A.nrow)]
    try:
        assert hp.poly32_info(M)["exact"] == (1 if kind == "exact" else 0)
        rng = np.random.default_rng(3)
        B = np.stack([A.b, rng.uniform(-1.0, 1.0, A.nrow), 0.5 * A.b])
        for degree in (0, 3):
            for nrhs in (3, 1):
                Xs = dev(gpu, np.zeros_like(B[:nrhs]))
                _, its1, nrs1, _ = hp.HPCCG_poly32(M, dev(gpu, B[:nrhs]), Xs, degree=degree, max_iter=40, device=True)
                tr1 = [M.last_trace_poly32(c).copy() for c in range(nrhs)]
                for Ms in groups:
                    Bd, Xd = dev(gpu, B[:nrhs]), dev(gpu, np.zeros_like(B[:nrhs]))
                    its, nrs, _ = hp.group_HPCCG_poly32(Ms, [Bd], [Xd], degree=degree, max_iter=40)
                    assert list(its) == list(its1) and nrs.tobytes() == nrs1.tobytes(), (degree, nrhs)
                    assert Xd.cpu().numpy().tobytes() == Xs.cpu().numpy().tobytes(), (degree, nrhs)
                    for c in range(nrhs):
                        assert hp.group_last_trace_poly32(Ms, c).tobytes() == tr1[c].tobytes()
                    assert hp.group_last_spectrum_poly32(Ms) == M.last_spectrum_poly32()
            assert its1[0] == 39 and np.all(np.isfinite(Xs.cpu().numpy()))
        for Ms in groups:
            assert hp.group_poly32_bound(Ms) == hp.poly32_bound(M)
            info = hp.group_poly32_info(Ms)
            assert len(info) == 1 and info[0] == hp.poly32_info(M)
    finally:
        for Ms in groups:
            for m in Ms:
                m.close()


# ---------------------------------------------------------------------------
# 5. columns are independent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["p2_3x33x17x9", "p10_csr3"], ids=["exact", "inexact"])
def test_columns_are_single_column_calls(hp, gpu, shape):
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    rng = np.random.default_rng(9)
    # the same tolerance meets differently scaled residuals at different iterations
    B = np.stack([A.b, A.b * 2.0 ** -20, rng.uniform(-1.0, 1.0, N) * 2.0 ** 10, A.b * 2.0 ** -40, A.b])
    X0 = np.zeros((5, N))
    X0[4] = A.xexact  # (ends before its first iteration)
    tol = 1e-8 * float(np.linalg.norm(A.b))
    one = [poly32_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], 150, tol)[0] for c in range(5)]
    stops = [o[1] for o in one]
    print(f"{shape}: stops {stops}")
    assert len(set(stops)) >= 3 and max(stops) < 149 and stops[4] == 0, stops
    for nrhs, pad in ((5, 5), (4, 0), (3, 0), (2, 0)):
        got = poly32_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 150, tol, pad=pad)
        assert_same(got, one[:nrhs])
        for g in got[:4]:
            assert len(g[3]) == g[1] + 1 and g[2] == g[3][-1]


# ---------------------------------------------------------------------------
# 6. the halo kernel and the halo by copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + INEXACT)
def test_the_halo_kernel_equals_the_copies(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs, 4)
    kernel = poly32_solve(hp, gpu, cs, B, X0, 30, degree=3)
    copies = poly32_solve(hp, gpu, cs, B, X0, 30, degree=3, halo_copies=True)
    assert kernel[0][1] > 0 and all(np.all(np.isfinite(x)) and x.any() for x in kernel[0][0])
    assert_same(kernel, copies)
    assert_same(poly32_solve(hp, gpu, cs, B, X0, 30, degree=3), kernel)  # (the switch is the call's own)


# ---------------------------------------------------------------------------
# 7. the plain and the non-temporal value loads
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["2x8c", "p10_3x33x17x9", "p10_2x12x10x8_7pt", "p10_csr3"])
def test_forced_nt_0_and_1_give_the_same_bits(hp, gpu, shape):
    """The kNT = false and kNT = true forms of the steps and of the exact
    members' SpMM, and the fp64 outer forms' two arms; with four columns the
    27-wide shapes take the x-triple plan on their interior slices under both."""
    cs = case(hp, shape)
    B, X0 = columns(cs, 4)
    assert [M.get_option("nt") for M in cs.Ms] == [0] * cs.P
    if shape in ("2x8c", "p10_3x33x17x9"):
        assert all(M.get_option("has_a") == 1 and M.get_option("a_width") == 27 for M in cs.Ms)
    got = {}
    try:
        for flag in (0, 1):
            for M in cs.Ms:
                M.set_option("nt", flag)
                assert M.get_option("nt") == flag
            got[flag] = [poly32_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 30, degree=2, pad=3) for nrhs in (1, 4)]
    finally:
        for M in cs.Ms:
            M.set_option("nt", -1)
    assert [M.get_option("nt") for M in cs.Ms] == [0] * cs.P
    for a, b in zip(got[0], got[1]):
        assert a[0][1] == 29 and all(np.all(np.isfinite(x)) and x.any() for x in a[0][0])
        assert_same(b, a)
    # nothing of the forced runs stays
    assert_same(poly32_solve(hp, gpu, cs, B, X0, 30, degree=2, pad=3), got[0][1])


# ---------------------------------------------------------------------------
# 9. (and 8.) inexact images: the restatement with A~ inside P
# ---------------------------------------------------------------------------
def follows_the_restatement(hp, gpu, cs, name, degree):
    A, N = cs.A, cs.N
    At = fl32(A)
    minv = 1.0 / csr_diagonal(A)
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    dot = rank_dot(cs.rows)
    xs, niters, normr, tr = poly32_solve(hp, gpu, cs, B, X0, 200, 1e-14 * r0, degree=degree)[0]
    lmin, lmax = hp.group_last_spectrum_poly32(cs.Ms)
    # the interval is the fp64 image's
    assert lmax == hp.group_poly32_bound(cs.Ms) == hp.group_poly_bound(cs.Ms) and lmin == lmax / EIG_RATIO
    _, _, _, tr_ref = restated32(A, At, A.b, minv, degree, lmin, lmax, 200, dot=dot)
    checked = check_trace(tr, tr_ref, RTRANS_RTOL_1GPU)
    print(f"{name} degree {degree}: {checked} trace points checked against the restatement, niters {niters}")
    assert checked >= 10, checked
    x = np.concatenate(xs)
    err = float(np.max(np.abs(x - A.xexact)))
    print(f"{name} degree {degree}: normr/r0 {normr / r0:.3e} max |x - xexact| {err:.3e}")
    assert normr <= 1e-14 * r0 and niters <= 198
    assert err <= 1e-9, err
    # the one-rank poly32 solve of the global matrix: the dots' order only
    M1 = tpolyg.one_rank_matrix(hp, cs)
    try:
        Bd, Xd = dev(gpu, B), dev(gpu, X0)
        _, it1, _, _ = hp.HPCCG_poly32(M1, Bd, Xd, degree=degree, lmin=lmin, lmax=lmax, device=True, max_iter=200,
                                       tolerance=1e-14 * r0)
        tr1 = M1.last_trace_poly32(0).copy()
    finally:
        M1.close()
    checked1 = check_trace(tr, tr1, RTRANS_RTOL_MULTI)
    print(f"{name} degree {degree}: {checked1} trace points checked against one rank, niters {niters} / {int(it1[0])}")
    assert checked1 >= 10, checked1
    # niters under a tolerance between two residuals of the restatement: the
    # widest gap in the middle third of the checked part
    lo, hi = checked // 3, 2 * checked // 3
    k = lo + int(np.argmax(tr_ref[lo:hi] / tr_ref[lo + 1:hi + 1]))
    assert tr_ref[k] > 1.01 * tr_ref[k + 1], (k, tr_ref[k], tr_ref[k + 1])
    tol = float(np.sqrt(tr_ref[k] * tr_ref[k + 1]))
    _, it_ref, nr_ref, _ = restated32(A, At, A.b, minv, degree, lmin, lmax, 200, tol, dot=dot)
    _, it, nr, _ = poly32_solve(hp, gpu, cs, B, X0, 200, tol, degree=degree)[0]
    assert it == it_ref and 0 < it < niters, (it, it_ref, niters)
    assert abs(nr - nr_ref) <= RTRANS_RTOL_1GPU * nr_ref, (nr, nr_ref)
    # ... and these are not the fp64 polynomial's iterates
    x64 = tpolyg.poly_solve(hp, gpu, cs, B, X0, 200, 1e-14 * r0, degree=degree)[0][0]
    assert np.concatenate(x64).tobytes() != x.tobytes()


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("shape", INEXACT)
def test_inexact_images_follow_the_restatement(hp, gpu, shape, degree):
    follows_the_restatement(hp, gpu, case(hp, shape), shape, degree)


def test_members_may_differ_in_exactness(hp, gpu):
    cs = case(hp, MIXED)
    A = cs.A
    bad = fl32(A).vals != A.vals
    lo, mid, hi = int(A.row_ptr[0]), int(A.row_ptr[512]), int(A.row_ptr[1024])
    assert not bad[lo:mid].any() and bad[mid:hi].any()
    info = hp.group_poly32_info(cs.Ms)
    assert [i["exact"] for i in info] == [1, 0], info
    assert [i["inexact_values"] for i in info] == [0, int(np.count_nonzero(bad[mid:hi]))], info
    B, X0 = columns(cs, 5)
    for minv in (None, 1.0):
        assert_same(poly32_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=0, minv=minv, pad=3),
                    tpg.pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, minv=minv))
    follows_the_restatement(hp, gpu, cs, MIXED, 3)


# ---------------------------------------------------------------------------
# 10. it keeps what the polynomial is for
# ---------------------------------------------------------------------------
def test_degree_3_keeps_the_fp64_group_polynomials_iterations(hp, gpu):
    cs = case(hp, "p10_lap_3x33x17x9")
    A, N = cs.A, cs.N
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    tol = 1e-10 * r0
    _, it, nr, _ = poly32_solve(hp, gpu, cs, B, X0, 200, tol, degree=3)[0]
    _, it64, nr64, _ = tpolyg.poly_solve(hp, gpu, cs, B, X0, 200, tol, degree=3)[0]
    jac = tpg.pcg_solve(hp, gpu, cs, B, X0, 200, tol)[0]
    print(f"p10_lap_3x33x17x9: degree 3 {it} iterations (fp64 group polynomial {it64}), group Jacobi {jac[1]}; "
          f"normr/r0 {nr / r0:.3e}")
    assert abs(it - it64) <= 1, (it, it64)
    assert nr <= tol and nr64 <= tol and jac[2] <= tol
    assert 2 * it < jac[1], (it, jac[1])


# ---------------------------------------------------------------------------
# 11. degenerate columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "p10_csr3", "p10_2x12x10x8_7pt"])
def test_degenerate_columns_beside_ordinary_ones(hp, gpu, shape):
    cs = case(hp, shape)
    A, N = cs.A, cs.N
    At = fl32(A)
    minv = 1.0 / csr_diagonal(A)
    rng = np.random.default_rng(41)
    # a NaN on member 0's last row: a plane member 1 reads
    plane = cs.rows[0].stop - 1
    nan_pl = A.b.copy()
    nan_pl[plane] = np.nan
    B = np.stack([A.b, np.zeros(N), nan_pl, rng.uniform(-1.0, 1.0, N)])
    X0 = np.zeros((4, N))  # (column 1: b = 0 and x0 = 0, a residual that is zero in every summation order)
    mi = 25
    alone = {c: poly32_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], mi)[0] for c in (0, 3)}
    poly32_solve(hp, gpu, cs, np.tile(A.b, (4, 1)), X0, mi)  # four finite columns: the workspaces at this call's size
    sizes = [hp.group_poly32_workspace_bytes(M) for M in cs.Ms]
    for copies in (False, True):
        got = poly32_solve(hp, gpu, cs, B, X0, mi, halo_copies=copies)
        lmin, lmax = hp.group_last_spectrum_poly32(cs.Ms)
        for c in (0, 3):
            assert_same(got[c:c + 1], [alone[c]])
            assert got[c][1] == mi - 1 and all(np.all(np.isfinite(x)) for x in got[c][0])
        for c in (1, 2):
            x, it, nr, tr = restated32(A, At, B[c], minv, 2, lmin, lmax, mi, x0=X0[c])
            assert got[c][1] == it == 0, (c, got[c][1], it)
            assert math.isnan(got[c][2]) == math.isnan(nr) and (got[c][2] == 0.0) == (nr == 0.0), (c, got[c][2], nr)
            assert len(got[c][3]) == len(tr) == 1
            assert np.concatenate(got[c][0]).tobytes() == X0[c].tobytes()  # x untouched on every member
        assert math.isnan(got[2][2]) and got[1][2] == 0.0
        # ... and nothing of them stays: a following clean call is bitwise the first
        for c in (0, 3):
            assert_same(poly32_solve(hp, gpu, cs, B[c:c + 1], X0[c:c + 1], mi), [alone[c]])
    assert [hp.group_poly32_workspace_bytes(M) for M in cs.Ms] == sizes


# ---------------------------------------------------------------------------
# 12. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [1e300, 1e-40], ids=["overflow", "underflow"])
def test_a_member_outside_fp32_range_refuses_the_call(hp, gpu, bad):
    import torch
    A0, counts = tpg.global_matrix("2x8c")
    vals = A0.vals.copy()
    # one off-diagonal value of a row inside member 1
    row = 512 + 300
    k = int(A0.row_ptr[row])
    if A0.cols[k] == row:
        k += 1
    vals[k] = bad
    A = finish(A0.row_ptr, A0.cols, vals)
    Ms = tpg.members_from_csr(hp, A, counts)
    try:
        Bd = [torch.ones((2, n), dtype=torch.float64, device=gpu) for n in counts]
        Xd = [torch.full((2, n), 0.5, dtype=torch.float64, device=gpu) for n in counts]
        for _ in range(2):  # (the verdict is kept)
            for degree in (2, 0):
                with pytest.raises(hp.HPCCGError, match=r"\(-1\).*member 1: the matrix is outside fp32 range"):
                    hp.group_HPCCG_poly32(Ms, Bd, Xd, degree=degree, max_iter=10)
            with pytest.raises(hp.HPCCGError, match="member 1: the matrix is outside fp32 range"):
                hp.group_poly32_info(Ms)
            with pytest.raises(hp.HPCCGError, match="member 1: the matrix is outside fp32 range"):
                hp.group_poly32_bound(Ms)
        assert all(torch.all(x == 0.5) for x in Xd)
        # the fp64 group polynomial takes the members as they are
        its, _, _ = hp.group_HPCCG_poly(Ms, Bd, [x.clone() for x in Xd], max_iter=3)
        assert list(its) == [2, 2]
    finally:
        for M in Ms:
            M.close()
    # ... and a good group afterwards
    cs = case(hp, "2x8c")
    B, X0 = columns(cs, 2)
    assert_same(poly32_solve(hp, gpu, cs, B, X0, 10), tpolyg.poly_solve(hp, gpu, cs, B, X0, 10))


def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.poly32_group_lib()
    err = hp.lib().hpccg_hip_last_error
    cs = case(hp, "2x8c")
    three = case(hp, "3x33x17x9")
    n = 512
    B, X0 = columns(cs, 2)
    Bd = [dev(gpu, a) for a in cs.split(B)]
    Xd = [dev(gpu, a) for a in cs.split(X0)]
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = poly32_solve(hp, gpu, cs, B, X0, 10)

    def call(Ms, ldb=(n, n), ldx=(n, n), nrhs=2, max_iter=10, nranks=2, minv=None, degree=2, lmin=0.0, lmax=0.0):
        hs = (C.c_void_p * len(Ms))(*[M.h for M in Ms])
        bp = (C.c_void_p * 2)(*[t.data_ptr() for t in Bd])
        xp = (C.c_void_p * 2)(*[t.data_ptr() for t in Xd])
        mp = None if minv is None else (C.c_void_p * 2)(*[t.data_ptr() for t in minv])
        return L.hpccg_hip_group_poly32_solve_device(hs, nranks, nrhs, bp, (C.c_longlong * 2)(*ldb), xp,
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
        assert b"gather" in err() and b"group poly32:" in err()
        with pytest.raises(hp.HPCCGError):
            hp.group_poly32_info(gather)
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
        bound = hp.group_poly32_bound(cs.Ms)
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
            assert b"group poly32: member 1's minv[300]" in err(), err()
            with pytest.raises(hp.HPCCGError, match=r"member 1's minv\[300\]"):
                hp.group_HPCCG_poly32(cs.Ms, Bd, Xd, max_iter=10, minvs=mv)
            with pytest.raises(hp.HPCCGError, match=r"member 1's minv\[300\]"):
                hp.group_poly32_bound(cs.Ms, mv)
            assert untouched()
        with pytest.raises(hp.HPCCGError):
            hp.group_HPCCG_poly32(gather, Bd, Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError):
            hp.group_poly32_bound(cs.Ms[::-1])
        with pytest.raises(hp.HPCCGError):
            hp.group_last_trace_poly32(cs.Ms, 2)  # (the last solve had two columns)
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            hp.group_last_spectrum_poly32(other)
        assert untouched()
        assert torch.cuda.current_device() == dev0
        # the one-rank fp32-image library keeps refusing a member
        for m in cs.Ms:
            assert hp.poly32_lib().hpccg_hip_poly32_solve_device(m.h, 2, Bd[0].data_ptr(), n, Xd[0].data_ptr(), n,
                                                                 None, 2, 0.0, 0.0, 10, 0.0, it, nr, None) == EINVAL
            assert b"group" in err()
        assert untouched()
    finally:
        for M in other + gather + [plain]:
            M.close()
    # ... and a good solve afterwards
    assert_same(poly32_solve(hp, gpu, cs, B, X0, 10), ref)


@pytest.mark.parametrize("kind", list(tpg.BAD))
def test_a_bad_diagonal_on_one_member_is_refused(hp, gpu, kind):
    import torch
    A0, counts = tpg.global_matrix("csr3")
    start1 = counts[0]
    rp, cols, vals = tpg._edited(A0, tpg.BAD[kind])
    A = finish(rp, cols, vals)
    Ms = tpg.members_from_csr(hp, A, counts)
    # (a NaN has no fp32 image either, and the member's image comes before its preconditioner)
    what = "member 1: the matrix is outside fp32 range" if kind == "nan" else rf".*member 1 row {517 - start1} "
    try:
        Bd = [torch.ones((2, n), dtype=torch.float64, device=gpu) for n in counts]
        Xd = [torch.full((2, n), 0.5, dtype=torch.float64, device=gpu) for n in counts]
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match=rf"\(-1\).*group poly32: {what}"):
                hp.group_HPCCG_poly32(Ms, Bd, Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError, match=what):
            hp.group_poly32_bound(Ms)
        assert all(torch.all(x == 0.5) for x in Xd)
    finally:
        for M in Ms:
            M.close()


# ---------------------------------------------------------------------------
# 13. isolation and the workspace's life
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
        group = tpg.pcg_solve(hp, gpu, cs, B, X0, 40) + tpolyg.poly_solve(hp, gpu, cs, B, X0, 40)
        one = []
        for f in (hp.HPCCG_pcg, hp.HPCCG_poly, hp.HPCCG_poly32, hp.HPCCG_batch, hp.HPCCG_mixed):
            b1, x1 = dev(gpu, B1), dev(gpu, X1)
            _, it1, nr1, _ = f(M1, b1, x1, max_iter=40, device=True)
            one += [x1.cpu().numpy().tobytes(), it1.tobytes(), nr1.tobytes()]
        return single + group, ([x.cpu().numpy().tobytes() for x in Xd], its.tobytes(), nrs.tobytes(), one)

    try:
        before = others()
        counts = live(hp)
        first = poly32_solve(hp, gpu, cs, B, X0, 40)
        assert live(hp) == counts
        after = others()
        assert_same(after[0], before[0])
        assert after[1] == before[1]
        for _ in range(3):
            assert_same(poly32_solve(hp, gpu, cs, B, X0, 40), first)
        assert all(hp.group_poly32_workspace_bytes(M) > 0 for M in cs.Ms)
        assert M1.poly32_workspace_bytes() > 0 and hp.group_poly32_workspace_bytes(M1) == 0
    finally:
        M1.close()
        for M in cs.Ms:
            M.batch_release()
            hp.group_pcg_release(M)
            hp.group_poly_release(M)


def test_workspace_goes_with_the_members(hp, gpu):
    base = hp.group_poly32_live_workspaces()
    others = live(hp)
    cs = tpg.Case(hp, "2x8c")
    try:
        B, X0 = columns(cs, 2)
        first = poly32_solve(hp, gpu, cs, B, X0, 10)
        assert hp.group_poly32_live_workspaces() == base + 2
        image = hp.group_poly32_info(cs.Ms)[1]["image_bytes"]
        assert image == 4 * 27 * 512  # one slice of 27 slots
        assert all(hp.group_poly32_workspace_bytes(M) > image + 2 * 8 * 512 for M in cs.Ms)
        hp.group_poly32_release(cs.Ms[1])
        assert hp.group_poly32_live_workspaces() == base + 1 and hp.group_poly32_workspace_bytes(cs.Ms[1]) == 0
        assert_same(poly32_solve(hp, gpu, cs, B, X0, 10), first)  # rebuilt on demand, the image and the caches too
        small = hp.group_poly32_workspace_bytes(cs.Ms[1])
        assert small > image
        poly32_solve(hp, gpu, cs, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the image and the caches stay
        assert hp.group_poly32_workspace_bytes(cs.Ms[1]) > small
        assert_same(poly32_solve(hp, gpu, cs, B, X0, 10), first)
        for M in cs.Ms:
            hp.group_poly32_release(M)
            hp.group_poly32_release(M)  # (idempotent)
            assert hp.group_poly32_workspace_bytes(M) == 0
        assert hp.group_poly32_live_workspaces() == base
        with pytest.raises(hp.HPCCGError, match="no spectrum"):
            hp.group_last_spectrum_poly32(cs.Ms)
        # the image alone is a workspace too
        assert hp.group_poly32_info(cs.Ms)[0]["image_bytes"] == image
        assert [hp.group_poly32_workspace_bytes(M) for M in cs.Ms] == [image, image]
        assert_same(poly32_solve(hp, gpu, cs, B, X0, 10), first)
        assert hp.group_poly32_live_workspaces() == base + 2  # ... and closing the members without a release frees them
        assert first[0][1] == 9
        assert live(hp) == others
    finally:
        cs.close()
    assert hp.group_poly32_live_workspaces() == base
    assert live(hp) == others
