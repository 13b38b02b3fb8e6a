"""Diagonally preconditioned CG over an in-process rank group
(include/hpccg_hip_pcg_group.h, lib/libhpccg_hip_pcg_group.so): per column the
recurrence of hpccg_hip_pcg.h, every member on its own rows, the ghost planes of
p moved by one kernel per member, the three dots summed over the members in
rank order. All members share one device.

  1. m = 1 (and one power of two) everywhere: column c is bitwise group_HPCCG of
     that column on the same members (every member's x, niters, normr, trace);
  2. Jacobi on S A S with S b, S powers of two: s_i x'_i is bitwise the x of
     Jacobi on A with b, on every member (the per-row m from each member's own
     image, both image forms);
  3. the halo kernel against the halo by copies: the same bits; with m = 1 the
     group batch on the same members (the other user of the group engine,
     csrc/hpccg_group.h): the same bits;
  4. on matrices scaled by s_i = 10^u_i: the group's trace against the one-rank
     preconditioned solve of the global matrix and against the NumPy
     restatement below (they differ in the dots' summation order only);
  5. it pays: on a scaled 2 x 16x16x8 Jacobi converges where group_HPCCG does not;
  6. the diagonal read from each member's image is the CSR's;
  7. refusals; 8. the other solvers are undisturbed; 9. the workspace's life.

Shapes (members x local grid; those of test_gpu_batch_group.py, the smallest
that reach every path): 2 x 8^3 (one slice per member), 8 x 16^3 (interior
members with both ghost planes), 3 x 33x17x9 (561-row odd planes, unaligned,
the upper ghost plane starting inside the last slice's padding rows: the halo
kernel's one-double arm), 4 x 7x5x1 (ghost planes as large as the member),
2 x 12x10x8 7-pt, and a banded random SPD CSR in slabs of 500 / 513 / 487 rows
(the int32-column image) -- and the same global matrices with every entry
a_ij s_i s_j, s_i = 2^e_i, e_i random in [-6, 6] ("p2_"), or s_i = 10^u_i, u_i
uniform in [-1.5, 1.5] ("p10_"), split into the same slabs by group_from_csr.
Column counts 1, 2, 3, 4, 5, 7: every chunking of the launches.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import RTRANS_RTOL_MULTI, check_trace

pytestmark = pytest.mark.gpu

EINVAL, EPLAN = -1, -5
MAX_ITER = 60
NCOL = 7


# ---------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------
def random_spd(rng, n, per_row, band):
    """Symmetric, strictly diagonally dominant (so SPD), banded, entries of each
    row in random order; b = A 1 (the generator of test_gpu_batch_group.py)."""
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for _ in range(int(rng.integers(0, per_row + 1))):
            j = int(i + rng.integers(-band, band + 1))
            if 0 <= j < n and j != i:
                v = -float(rng.uniform(0.05, 1.0))
                rows[i][j] = v
                rows[j][i] = v
    row_ptr = np.zeros(n + 1, np.int64)
    cols, vals = [], []
    for i in range(n):
        d = rows[i]
        ent = list(d.items()) + [(i, sum(-v for v in d.values()) + float(rng.uniform(0.5, 2.0)))]
        for k in rng.permutation(len(ent)):
            cols.append(ent[k][0])
            vals.append(ent[k][1])
        row_ptr[i + 1] = len(cols)
    return finish(row_ptr, np.asarray(cols, np.int32), np.asarray(vals, np.float64))


def finish(row_ptr, cols, vals):
    """The oracle's CSR of the entries, b = A 1."""
    n = len(row_ptr) - 1
    A = oracle.CSR(row_ptr, cols, vals, np.zeros(n), np.zeros(n), np.ones(n))
    A.b = oracle.sparsemv(A, np.ones(n))
    return A


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


def scale_of(kind, n):
    rng = np.random.default_rng(77)
    return 2.0 ** rng.integers(-6, 7, n) if kind == "p2" else 10.0 ** rng.uniform(-1.5, 1.5, n)


STENCILS = {
    "2x8c": (8, 8, 8, 2, False),
    "8x16c": (16, 16, 16, 8, False),
    "3x33x17x9": (33, 17, 9, 3, False),
    "4x7x5x1": (7, 5, 1, 4, False),
    "2x12x10x8_7pt": (12, 10, 8, 2, True),
    "2x16x16x8": (16, 16, 8, 2, False),  # (5. only)
}
CSR_SLABS = (500, 513, 487)
SHAPES = ["2x8c", "8x16c", "3x33x17x9", "4x7x5x1", "2x12x10x8_7pt", "csr3"]
HAS_A = {name: int(name != "csr3") for name in SHAPES + ["2x16x16x8"]}


def global_matrix(name):
    """(the global matrix, the members' row counts) of an unscaled shape."""
    if name in STENCILS:
        nx, ny, nz, P, s7 = STENCILS[name]
        return oracle.generate(nx, ny, nz * P, use_7pt=s7), [nx * ny * nz] * P
    return random_spd(np.random.default_rng(31), sum(CSR_SLABS), 6, 40), list(CSR_SLABS)


def csr_parts(A, counts):
    parts, s = [], 0
    for n in counts:
        lo, hi = int(A.row_ptr[s]), int(A.row_ptr[s + n])
        parts.append((A.row_ptr[s:s + n + 1] - lo, A.cols[lo:hi], A.vals[lo:hi], s))
        s += n
    return parts


def members_from_csr(hp, A, counts):
    """The global matrix in slabs of counts rows: members of the z-slab plan."""
    Ms = hp.group_from_csr(csr_parts(A, counts), A.nrow)
    assert all(M.get_option("halo_mode") == 1 for M in Ms), [M.get_option("halo_mode") for M in Ms]
    return Ms


class Case:
    """A group, the global matrix on the host, the members' row ranges and the
    scaling s of a "p2_" / "p10_" shape (else None)."""

    def __init__(self, hp, name):
        kind, _, rest = name.partition("_")
        if kind in ("p2", "p10"):
            A0, counts = global_matrix(rest)
            self.s = scale_of(kind, A0.nrow)
            self.A = scaled(A0, self.s)
            self.Ms = members_from_csr(hp, self.A, counts)
            self.has_a = HAS_A[rest]
        else:
            self.A, counts = global_matrix(name)
            self.s = None
            if name in STENCILS:
                nx, ny, nz, P, s7 = STENCILS[name]
                self.Ms = hp.group_generate(nx, ny, nz, P, use_7pt=s7)
            else:
                self.Ms = members_from_csr(hp, self.A, counts)
            self.has_a = HAS_A[name]
        # both image forms are known to run: SELL-512-A on the stencils, plain and scaled, SELL-512 on the CSR
        assert [M.get_option("has_a") for M in self.Ms] == [self.has_a] * len(counts), name
        self.P = len(counts)
        self.rows = []
        s = 0
        for n, M in zip(counts, self.Ms):
            assert M.info()["nrow"] == n
            self.rows.append(slice(s, s + n))
            s += n
        self.N = s

    def split(self, a):
        """(ncol, N) global columns -> per member (ncol, n_r)."""
        return [np.ascontiguousarray(a[:, rw]) for rw in self.rows]

    def close(self):
        for M in self.Ms:
            M.close()


_cases = {}


def case(hp, name):
    if name not in _cases:
        _cases[name] = Case(hp, name)
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cases(hp):
    base = hp.group_pcg_live_workspaces()
    others = (hp.pcg_live_workspaces(), hp.batch_live_workspaces())
    yield
    for c in _cases.values():
        c.close()
    _cases.clear()
    assert hp.group_pcg_live_workspaces() == base
    assert (hp.pcg_live_workspaces(), hp.batch_live_workspaces()) == others


def columns(cs, ncol=NCOL, seed=5):
    """The test's global right-hand sides and initial guesses, (ncol, N) each."""
    b, N = cs.A.b, cs.N
    g = np.arange(N)
    rng = np.random.default_rng(seed)
    B = np.zeros((ncol, N))
    X0 = np.zeros((ncol, N))
    for c in range(ncol):
        if c == 0:
            B[c] = b
        elif c == 1:
            B[c] = b * 2.0 ** -3
            X0[c] = 0.25 * ((g % 7) - 3)
        elif c == 3:
            B[c] = rng.uniform(-1.0, 1.0, N)
            X0[c] = rng.uniform(-1.0, 1.0, N)
        else:
            B[c] = rng.uniform(-1.0, 1.0, N) * 2.0 ** (c - 4)
    return B, X0


def dev(gpu, a, pad=0, fill=7.5):
    """(ncol, n) host columns on the device with leading dimension n + pad."""
    import torch
    ncol, n = a.shape
    t = torch.full((ncol, n + pad), fill, dtype=torch.float64, device=gpu)
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t


def single_solves(hp, gpu, cs, B, X0, max_iter, tol=0.0):
    """Every column through group_HPCCG alone: [(xs per member, niters, normr, trace)]."""
    import torch
    out = []
    for c in range(B.shape[0]):
        bs = [torch.from_numpy(B[c, rw].copy()).to(gpu) for rw in cs.rows]
        xs = [torch.from_numpy(X0[c, rw].copy()).to(gpu) for rw in cs.rows]
        ierr, it, nr, _ = hp.group_HPCCG(cs.Ms, bs, xs, max_iter=max_iter, tolerance=tol)
        assert ierr == 0
        tr = cs.Ms[0].last_trace().copy()
        for M in cs.Ms[1:]:
            assert M.last_trace().tobytes() == tr.tobytes()
        out.append(([x.cpu().numpy() for x in xs], it, nr, tr))
    return out


def pcg_solve(hp, gpu, cs, B, X0, max_iter, tol=0.0, minv=None, pad=0, halo_copies=False):
    """[(xs per member, niters, normr, trace)] per column of a group
    preconditioned solve; minv: None (Jacobi), a number (that value everywhere)
    or a global array."""
    import torch
    Bd = [dev(gpu, a, pad) for a in cs.split(B)]
    Xd = [dev(gpu, a, pad) for a in cs.split(X0)]
    minvs = None
    if minv is not None:
        m = np.full(cs.N, 1.0) * np.float64(minv)
        minvs = [torch.from_numpy(m[rw].copy()).to(gpu) for rw in cs.rows]
    its, nrs, times = hp.group_HPCCG_pcg(cs.Ms, Bd, Xd, max_iter=max_iter, tolerance=tol, minvs=minvs,
                                         halo_copies=halo_copies)
    assert times[0] > 0.0 and not times[1:].any()
    X = [x.cpu().numpy() for x in Xd]
    if pad:
        for x, rw in zip(X, cs.rows):
            assert np.all(x[:, rw.stop - rw.start:] == 7.5)  # nothing stored between the columns
    return [([x[c, :rw.stop - rw.start].copy() for x, rw in zip(X, cs.rows)], int(its[c]), float(nrs[c]),
             hp.group_last_trace_pcg(cs.Ms, c).copy()) for c in range(B.shape[0])]


def assert_same(got, ref):
    assert len(got) == len(ref)
    for c, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == r[1], (c, g[1], r[1])
        assert np.float64(g[2]).tobytes() == np.float64(r[2]).tobytes(), (c, g[2], r[2])
        assert g[3].tobytes() == r[3].tobytes(), (c, "trace")
        for m, (gx, rx) in enumerate(zip(g[0], r[0])):
            assert gx.tobytes() == rx.tobytes(), (c, "x of member", m, float(np.max(np.abs(gx - rx))))


# ---------------------------------------------------------------------------
# The recurrence of include/hpccg_hip_pcg.h restated: oracle.sparsemv and a
# fixed-order float64 dot (dot: oracle.ddot, a sequential sum). trace[k] is the
# normr iteration k reports, sqrt(rr_{k-1}) (HPCCG.cpp:358), as in every solver
# here.
# ---------------------------------------------------------------------------
def restated(A, b, minv, max_iter, tol=0.0, dot=None):
    dot = dot or oracle.ddot
    with np.errstate(all="ignore"):
        x = np.zeros(A.nrow)
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


# ---------------------------------------------------------------------------
# 1. a uniform m: the group solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_uniform_m_is_the_group_solve(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs)
    assert X0[1].any() and X0[3].any()  # nonzero x0 among them
    ref = single_solves(hp, gpu, cs, B, X0, MAX_ITER)
    assert ref[0][1] > 0
    for nrhs, pad in ((1, 0), (2, 3), (3, 0), (4, 0), (5, 3), (7, 0)):
        assert_same(pcg_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, minv=1.0, pad=pad), ref[:nrhs])
    for q in (-3, 5):
        for nrhs in (5, 1):
            assert_same(pcg_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, minv=2.0 ** q), ref[:nrhs])
    # a tolerance that column 0 meets part-way, and no iteration at all
    tr0 = ref[0][3]
    tol = float(np.min(tr0[:len(tr0) // 2 + 1])) * (1.0 + 2.0 ** -10)
    for max_iter, t in ((MAX_ITER, tol), (1, 0.0), (0, 0.0)):
        part = single_solves(hp, gpu, cs, B[:4], X0[:4], max_iter, t)
        if t:
            assert part[0][1] < ref[0][1], (part[0][1], ref[0][1])
        assert_same(pcg_solve(hp, gpu, cs, B[:4], X0[:4], max_iter, t, minv=1.0), part)


def test_group_of_one_is_the_one_rank_solve(hp, gpu):
    """nranks == 1 runs the same code on a halo-free matrix: 0.0 + a total is
    the total, so every column is bitwise HPCCG_pcg's."""
    M = hp.Matrix.generate(12, 11, 10)
    try:
        A = oracle.generate(12, 11, 10)
        rng = np.random.default_rng(3)
        B = np.stack([A.b, rng.uniform(-1.0, 1.0, A.nrow), 0.5 * A.b])
        for nrhs in (3, 1):
            Bd, Xd = dev(gpu, B[:nrhs]), dev(gpu, np.zeros_like(B[:nrhs]))
            its, nrs, _ = hp.group_HPCCG_pcg([M], [Bd], [Xd], max_iter=40)
            Xs = dev(gpu, np.zeros_like(B[:nrhs]))
            _, its1, nrs1, _ = hp.HPCCG_pcg(M, Bd, Xs, max_iter=40, device=True)
            assert list(its) == list(its1) and nrs.tobytes() == nrs1.tobytes()
            assert Xd.cpu().numpy().tobytes() == Xs.cpu().numpy().tobytes()
            for c in range(nrhs):
                assert hp.group_last_trace_pcg([M], c).tobytes() == M.last_trace_pcg(c).tobytes()
    finally:
        M.close()


# ---------------------------------------------------------------------------
# 2. exact scaling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "csr3"])
def test_jacobi_commutes_with_a_power_of_two_scaling(hp, gpu, shape):
    cs, css = case(hp, shape), case(hp, "p2_" + shape)
    assert cs.has_a == css.has_a == HAS_A[shape]
    s, N = css.s, cs.N
    rng = np.random.default_rng(3)
    B = np.stack([cs.A.b, rng.uniform(-1.0, 1.0, N), cs.A.b * 2.0 ** -7, rng.uniform(-1.0, 1.0, N)])
    X0 = np.zeros((4, N))
    for nrhs in (4, 1, 2):
        got = pcg_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], 20)
        gots = pcg_solve(hp, gpu, css, B[:nrhs] * s, X0[:nrhs], 20)
        for c in range(nrhs):
            assert got[c][1] == gots[c][1] == 19
            for m, rw in enumerate(cs.rows):
                x, xs = got[c][0][m], gots[c][0][m] * s[rw]
                assert xs.tobytes() == x.tobytes(), (nrhs, c, m, float(np.max(np.abs(xs - x))))
                assert np.all(np.isfinite(x)) and x.any()


# ---------------------------------------------------------------------------
# 3. the halo kernel and the halo by copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x33x17x9", "4x7x5x1", "p10_csr3"])
def test_the_halo_kernel_equals_the_copies(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs, 5)
    kernel = pcg_solve(hp, gpu, cs, B, X0, MAX_ITER)
    copies = pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, halo_copies=True)
    assert kernel[0][1] > 0 and all(np.all(np.isfinite(x)) for x in kernel[0][0])
    assert_same(kernel, copies)
    assert_same(pcg_solve(hp, gpu, cs, B, X0, MAX_ITER), kernel)  # (the switch is the call's own)


def batch_solve(hp, gpu, cs, B, X0, max_iter):
    """pcg_solve's result of the group batch on the same members."""
    Bd = [dev(gpu, a) for a in cs.split(B)]
    Xd = [dev(gpu, a) for a in cs.split(X0)]
    its, nrs, _ = hp.group_HPCCG_batch(cs.Ms, Bd, Xd, max_iter=max_iter)
    X = [x.cpu().numpy() for x in Xd]
    return [([x[c].copy() for x in X], int(its[c]), float(nrs[c]), hp.group_last_trace_batch(cs.Ms, c).copy())
            for c in range(B.shape[0])]


@pytest.mark.parametrize("shape", ["3x33x17x9", "csr3"])
def test_both_users_of_the_group_engine_agree(hp, gpu, shape):
    """The group batch and the group pcg run one group engine (halo, sum, launch
    loop, read-back) with their own kernels; with m = 1 those compute the same
    numbers, so every member's x, niters, normr and every column's trace are
    the same bits. 7 columns: launches of 4 + 3 in both; 5: 4 + 1 here, 4 + 2
    in the batch. The batch runs before and after the pcg on the same members."""
    cs = case(hp, shape)
    try:
        for ncol in (7, 5):
            B, X0 = columns(cs, ncol)
            batch = batch_solve(hp, gpu, cs, B, X0, MAX_ITER)
            assert batch[0][1] > 0 and all(np.all(np.isfinite(x)) and x.any() for x in batch[0][0])
            assert_same(pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, minv=1.0), batch)
            assert_same(batch_solve(hp, gpu, cs, B, X0, MAX_ITER), batch)
    finally:
        for M in cs.Ms:
            M.batch_release()


# ---------------------------------------------------------------------------
# 4. the group against one rank and against the restatement
# ---------------------------------------------------------------------------
# The restatement run on the CPU with three dot orders -- oracle.ddot's
# sequential sum, numpy's blocked one, and the sequential sums of the members'
# slabs added in rank order -- agrees with itself on the checked part of the
# rtrans trace (60 iterations; 11 to 49 points) to 2.3e-12 (p10_2x8c), 1.6e-14
# (p10_csr3), 1.6e-13 (8x16c), 3.6e-13 (3x33x17x9), 7.3e-11 (4x7x5x1) and
# 3.5e-14 (7-pt): a thousandth of RTRANS_RTOL_MULTI at most, so the bound has
# room for what the members' summation order costs and for nothing else.
@pytest.mark.parametrize("shape", SHAPES)
def test_group_jacobi_follows_the_one_rank_solve(hp, gpu, shape):
    cs = case(hp, "p10_" + shape)
    A, N = cs.A, cs.N
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    M1 = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    try:
        def one_rank(tol):
            Bd, Xd = dev(gpu, B), dev(gpu, X0)
            _, its, nrs, _ = hp.HPCCG_pcg(M1, Bd, Xd, max_iter=MAX_ITER, tolerance=tol, device=True)
            return Xd.cpu().numpy()[0], int(its[0]), float(nrs[0]), M1.last_trace_pcg(0).copy()

        x1, it1, nr1, tr1 = one_rank(0.0)
        xs, it, nr, tr = pcg_solve(hp, gpu, cs, B, X0, MAX_ITER)[0]
        checked = check_trace(tr, tr1, RTRANS_RTOL_MULTI)
        print(f"{shape}: {checked} trace points checked against one rank, niters {it} / {it1}")
        assert checked >= 10, checked
        if shape in ("2x8c", "csr3"):
            _, _, _, tr_ref = restated(A, A.b, 1.0 / csr_diagonal(A), MAX_ITER)
            checked_ref = check_trace(tr, tr_ref, RTRANS_RTOL_MULTI)
            print(f"{shape}: {checked_ref} trace points checked against the restatement")
            assert checked_ref >= 10, checked_ref
        # a tolerance between two residuals of the one-rank solve (the widest
        # gap in the middle third of the checked part): the same stop
        lo, hi = checked // 3, 2 * checked // 3
        k = lo + int(np.argmax(tr1[lo:hi] / tr1[lo + 1:hi + 1]))
        assert tr1[k] > 1.01 * tr1[k + 1], (k, tr1[k], tr1[k + 1])
        tol = float(np.sqrt(tr1[k] * tr1[k + 1]))
        _, it1t, nr1t, _ = one_rank(tol)
        _, itt, nrt, _ = pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, tol)[0]
        assert itt == it1t and 0 < itt < it, (itt, it1t, it)
        assert abs(nrt - nr1t) <= RTRANS_RTOL_MULTI * nr1t, (nrt, nr1t)
    finally:
        M1.close()


# ---------------------------------------------------------------------------
# 5. it pays
# ---------------------------------------------------------------------------
def test_jacobi_converges_where_the_group_solve_does_not(hp, gpu):
    cs = case(hp, "p2_2x16x16x8")
    A, N = cs.A, cs.N
    B, X0 = A.b.reshape(1, N).copy(), np.zeros((1, N))
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    tol = 1e-10 * r0
    M1 = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    try:
        Bd, Xd = dev(gpu, B), dev(gpu, X0)
        _, its1, _, _ = hp.HPCCG_pcg(M1, Bd, Xd, max_iter=200, tolerance=tol, device=True)
    finally:
        M1.close()
    xs, it, nr, tr = pcg_solve(hp, gpu, cs, B, X0, 200, tol)[0]
    plain = single_solves(hp, gpu, cs, B, X0, 200, tol)[0]
    print(f"p2_2x16x16x8: Jacobi {it} iterations (one rank {int(its1[0])}), normr/r0 {nr / r0:.3e}; plain {plain[1]} "
          f"iterations, normr/r0 {plain[2] / r0:.3e}")
    assert abs(it - int(its1[0])) <= 1 and it < 100, (it, its1)
    assert nr <= tol
    assert plain[1] == 199 and plain[2] > tol, plain[1:3]


# ---------------------------------------------------------------------------
# 6. the diagonal
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + ["p10_" + s for s in SHAPES] + ["p2_3x33x17x9", "p2_csr3"])
def test_the_diagonal_is_the_csr_diagonal_of_each_members_rows(hp, gpu, shape):
    cs = case(hp, shape)
    d = csr_diagonal(cs.A)
    got = hp.group_pcg_diagonal(cs.Ms)
    for m, rw in enumerate(cs.rows):
        assert got[m].tobytes() == d[rw].tobytes(), (shape, m)


def _edited(A, edit):
    rp, cols, vals = A.row_ptr.copy(), A.cols.copy(), A.vals.copy()
    return edit(rp, cols, vals, rows_of(A))


def _diag_times(f):
    def edit(rp, cols, vals, rows):
        vals[(rows == 517) & (cols == 517)] *= f  # member 1's local row 17 (slabs from row 500 and from row 512)
        return rp, cols, vals
    return edit


def _missing_diag(rp, cols, vals, rows):
    keep = ~((rows == cols) & ((rows == 517) | (rows == 900)))
    lens = np.bincount(rows[keep], minlength=len(rp) - 1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), cols[keep], vals[keep]


BAD = {"zero": _diag_times(0.0), "negative": _diag_times(-1.0), "nan": _diag_times(float("nan")),
       "missing": _missing_diag}


@pytest.mark.parametrize("shape", ["csr3", "2x8c"])
@pytest.mark.parametrize("kind", list(BAD))
def test_a_bad_diagonal_on_one_member_is_refused(hp, gpu, shape, kind):
    import torch
    A0, counts = global_matrix(shape)
    start1 = counts[0]
    rp, cols, vals = _edited(A0, BAD[kind])
    A = finish(rp, cols, vals)
    Ms = members_from_csr(hp, A, counts)
    try:
        assert [M.get_option("has_a") for M in Ms] == [HAS_A[shape]] * len(counts)
        d = hp.group_pcg_diagonal(Ms)
        full = np.concatenate(d)
        if kind == "missing":
            assert full[517] == 0.0 and full[900] == 0.0 and np.all(np.delete(full, [517, 900]) > 0.0)
        else:
            assert full.tobytes() == csr_diagonal(A).tobytes()
        Bd = [torch.ones((2, n), dtype=torch.float64, device=gpu) for n in counts]
        Xd = [torch.full((2, n), 0.5, dtype=torch.float64, device=gpu) for n in counts]
        for _ in range(2):  # (the verdict is kept)
            with pytest.raises(hp.HPCCGError, match=rf"\(-1\).*member 1 row {517 - start1} "):
                hp.group_HPCCG_pcg(Ms, Bd, Xd, max_iter=10)
        assert all(torch.all(x == 0.5) for x in Xd)
        # a caller's m is taken on the same members (NaN entries aside: they reach every product)
        if kind != "nan":
            ones = [torch.ones(n, dtype=torch.float64, device=gpu) for n in counts]
            its, _, _ = hp.group_HPCCG_pcg(Ms, Bd, [x.clone() for x in Xd], max_iter=3, minvs=ones)
            assert list(its) == [2, 2]
    finally:
        for M in Ms:
            M.close()


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.pcg_group_lib()
    err = hp.lib().hpccg_hip_last_error
    cs = case(hp, "2x8c")
    three = case(hp, "3x33x17x9")
    n = 512
    B, X0 = columns(cs, 2)
    Bd = [dev(gpu, a) for a in cs.split(B)]
    Xd = [dev(gpu, a) for a in cs.split(X0)]
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()
    ref = pcg_solve(hp, gpu, cs, B, X0, 10)

    def call(Ms, ldb=(n, n), ldx=(n, n), nrhs=2, max_iter=10, nranks=2, minv=None):
        hs = (C.c_void_p * len(Ms))(*[M.h for M in Ms])
        bp = (C.c_void_p * 2)(*[t.data_ptr() for t in Bd])
        xp = (C.c_void_p * 2)(*[t.data_ptr() for t in Xd])
        mp = None if minv is None else (C.c_void_p * 2)(*[t.data_ptr() for t in minv])
        return L.hpccg_hip_group_pcg_solve_device(hs, nranks, nrhs, bp, (C.c_longlong * 2)(*ldb), xp,
                                                  (C.c_longlong * 2)(*ldx), mp, max_iter, 0.0, it, nr, None)

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
        assert call(cs.Ms[::-1]) == EINVAL  # the wrong order
        assert b"rank" in err()
        assert untouched()
        assert call(three.Ms[:2]) == EINVAL  # a wrong nranks: a subset of a group
        assert b"rank" in err()
        assert call(cs.Ms, nranks=1) == EINVAL
        assert call([plain, plain]) == EINVAL  # a single-rank matrix in a 2-slot call
        assert untouched()
        assert call([cs.Ms[0], other[1]]) == EINVAL  # members of two groups
        assert b"another group" in err()
        assert untouched()
        assert call(gather) == EPLAN
        assert b"gather" in err()
        assert untouched()
        assert call(cs.Ms, ldb=(n, n - 1)) == EINVAL
        assert b"leading dimension" in err()
        assert call(cs.Ms, ldx=(n - 1, n)) == EINVAL
        assert call(cs.Ms, nrhs=0) == EINVAL
        assert call(cs.Ms, max_iter=-1) == EINVAL
        assert untouched()
        # a caller's m with a bad entry on the last member
        for bad in (0.0, float("nan"), -1.0, float("inf")):
            mv = [torch.ones(n, dtype=torch.float64, device=gpu) for _ in range(2)]
            mv[1][300] = bad
            mv[1][411] = bad
            assert call(cs.Ms, minv=mv) == EINVAL
            assert b"member 1's minv[300]" in err(), err()
            with pytest.raises(hp.HPCCGError, match=r"member 1's minv\[300\]"):
                hp.group_HPCCG_pcg(cs.Ms, Bd, Xd, max_iter=10, minvs=mv)
            assert untouched()
        with pytest.raises(hp.HPCCGError):
            hp.group_HPCCG_pcg(gather, Bd, Xd, max_iter=10)
        with pytest.raises(hp.HPCCGError):
            hp.group_pcg_diagonal(cs.Ms[::-1])
        with pytest.raises(hp.HPCCGError):
            hp.group_last_trace_pcg(cs.Ms, 2)  # (the last solve had two columns)
        assert untouched()
        assert torch.cuda.current_device() == dev0
        # the one-rank library keeps refusing a member
        for m in cs.Ms:
            assert hp.pcg_lib().hpccg_hip_pcg_solve_device(m.h, 2, Bd[0].data_ptr(), n, Xd[0].data_ptr(), n, None, 10,
                                                           0.0, it, nr, None) == EINVAL
            assert b"group" in err()
        assert untouched()
    finally:
        for M in other + gather + [plain]:
            M.close()
    # ... and a good solve afterwards
    assert_same(pcg_solve(hp, gpu, cs, B, X0, 10), ref)


# ---------------------------------------------------------------------------
# 8. isolation
# ---------------------------------------------------------------------------
def test_other_solves_and_repeats_are_undisturbed(hp, gpu):
    cs = case(hp, "3x33x17x9")
    B, X0 = columns(cs, 4)
    prob = hp.generate_matrix(16, 16, 16)
    M1 = hp.Matrix.from_hpc(prob)
    B1, X1 = np.stack([prob.b, 0.5 * prob.b]), np.zeros((2, len(prob.b)))
    prob.close()

    def others():
        single = single_solves(hp, gpu, cs, B[:2], X0[:2], 40)
        Bd = [dev(gpu, a) for a in cs.split(B)]
        Xd = [dev(gpu, a) for a in cs.split(X0)]
        its, nrs, _ = hp.group_HPCCG_batch(cs.Ms, Bd, Xd, max_iter=40)
        b1, x1 = dev(gpu, B1), dev(gpu, X1)
        _, it1, nr1, _ = hp.HPCCG_pcg(M1, b1, x1, max_iter=40, device=True)
        return single, ([x.cpu().numpy().tobytes() for x in Xd], its.tobytes(), nrs.tobytes(),
                        x1.cpu().numpy().tobytes(), it1.tobytes(), nr1.tobytes())

    try:
        before = others()
        counts = (hp.pcg_live_workspaces(), hp.batch_live_workspaces())
        first = pcg_solve(hp, gpu, cs, B, X0, 40)
        assert (hp.pcg_live_workspaces(), hp.batch_live_workspaces()) == counts
        after = others()
        assert_same(after[0], before[0])
        assert after[1] == before[1]
        for _ in range(3):
            assert_same(pcg_solve(hp, gpu, cs, B, X0, 40), first)
        assert all(hp.group_pcg_workspace_bytes(M) > 0 for M in cs.Ms)
        assert M1.pcg_workspace_bytes() > 0 and hp.group_pcg_workspace_bytes(M1) == 0
    finally:
        M1.close()
        for M in cs.Ms:
            M.batch_release()


# ---------------------------------------------------------------------------
# 9. the workspace's life
# ---------------------------------------------------------------------------
def test_workspace_goes_with_the_members(hp, gpu):
    base = hp.group_pcg_live_workspaces()
    others = (hp.pcg_live_workspaces(), hp.batch_live_workspaces())
    cs = Case(hp, "2x8c")
    try:
        B, X0 = columns(cs, 2)
        first = pcg_solve(hp, gpu, cs, B, X0, 10)
        assert hp.group_pcg_live_workspaces() == base + 2
        assert all(hp.group_pcg_workspace_bytes(M) > 2 * 8 * 512 for M in cs.Ms)
        hp.group_pcg_release(cs.Ms[1])
        assert hp.group_pcg_live_workspaces() == base + 1 and hp.group_pcg_workspace_bytes(cs.Ms[1]) == 0
        assert_same(pcg_solve(hp, gpu, cs, B, X0, 10), first)  # rebuilt on demand, the Jacobi cache too
        small = hp.group_pcg_workspace_bytes(cs.Ms[1])
        pcg_solve(hp, gpu, cs, np.tile(B, (3, 1)), np.tile(X0, (3, 1)), 30)  # grows; the cache stays
        assert hp.group_pcg_workspace_bytes(cs.Ms[1]) > small
        assert_same(pcg_solve(hp, gpu, cs, B, X0, 10), first)
        for M in cs.Ms:
            hp.group_pcg_release(M)
            hp.group_pcg_release(M)  # (idempotent)
            assert hp.group_pcg_workspace_bytes(M) == 0
        assert hp.group_pcg_live_workspaces() == base
        assert_same(pcg_solve(hp, gpu, cs, B, X0, 10), first)
        assert hp.group_pcg_live_workspaces() == base + 2
        assert first[0][1] == 9
        assert (hp.pcg_live_workspaces(), hp.batch_live_workspaces()) == others
    finally:
        cs.close()
    assert hp.group_pcg_live_workspaces() == base
    assert (hp.pcg_live_workspaces(), hp.batch_live_workspaces()) == others
