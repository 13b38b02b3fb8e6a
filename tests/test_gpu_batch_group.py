"""Batched multi-right-hand-side CG over an in-process rank group
(include/hpccg_hip_batch_group.h, lib/libhpccg_hip_batch.so): column c of a
group batch is bitwise group_HPCCG of that column alone on the same members --
every member's x, niters, normr and the residual trace -- and every column of
the group SpMM is bitwise the CPU oracle's sparsemv of the z-stacked global
matrix (row sums in entry order, no contraction). All members share one device.

Shapes (members x local grid): 2 x 8^3 (one slice per member, 64-row planes),
8 x 16^3 (interior members with both ghost planes, one dot group each),
3 x 33x17x9 (561-row odd planes, longer than a slice and unaligned; a 441-row
tail slice, so the upper ghost plane starts inside the last slice's padding
rows), 4 x 7x5x1 (ghost planes as large as the member), 2 x 12x10x8 and
2 x 1x9x6 7-pt, and a banded random SPD CSR in three slabs (entries in random
order: no SELL-512-A image, the int32-column SpMM; band 40 against slabs of
487 rows and more, so a member couples to its neighbours only).
Column counts 2, 3, 4, 5, 7: every chunking of the launches.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import RTRANS_RTOL_MULTI, check_final, check_trace, solve_case, unhex

pytestmark = pytest.mark.gpu

EINVAL, EPLAN = -1, -5
MAX_ITER = 60
NCOL = 7


# ---------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------
def random_spd(rng, n, per_row, band):
    """Symmetric, strictly diagonally dominant (so SPD), banded, entries of each
    row in random order; b = A 1 (the generator of test_gpu_batch.py)."""
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
    A = oracle.CSR(row_ptr, np.asarray(cols, np.int32), np.asarray(vals, np.float64), np.zeros(n), np.zeros(n),
                   np.ones(n))
    A.b = oracle.sparsemv(A, np.ones(n))
    return A


STENCILS = {
    "2x8c": (8, 8, 8, 2, False),
    "8x16c": (16, 16, 16, 8, False),
    "3x33x17x9": (33, 17, 9, 3, False),
    "4x7x5x1": (7, 5, 1, 4, False),
    "2x12x10x8_7pt": (12, 10, 8, 2, True),
    "2x1x9x6_7pt": (1, 9, 6, 2, True),
}
CSR_SLABS = (500, 513, 487)
SHAPES = list(STENCILS) + ["csr3"]


class Case:
    """A group, the global matrix on the host, and the members' row ranges."""

    def __init__(self, hp, name):
        if name in STENCILS:
            nx, ny, nz, P, s7 = STENCILS[name]
            self.A = oracle.generate(nx, ny, nz * P, use_7pt=s7)
            self.Ms = hp.group_generate(nx, ny, nz, P, use_7pt=s7)
            counts = [nx * ny * nz] * P
        else:
            counts = list(CSR_SLABS)
            self.A = A = random_spd(np.random.default_rng(31), sum(counts), 6, 40)
            parts, s = [], 0
            for n in counts:
                lo, hi = int(A.row_ptr[s]), int(A.row_ptr[s + n])
                parts.append((A.row_ptr[s:s + n + 1] - lo, A.cols[lo:hi], A.vals[lo:hi], s))
                s += n
            self.Ms = hp.group_from_csr(parts, sum(counts))
            assert all(M.get_option("has_a") == 0 for M in self.Ms)  # the int32-column SpMM
        self.P = len(counts)
        self.rows = []
        s = 0
        for n, M in zip(counts, self.Ms):
            assert M.info()["nrow"] == n
            self.rows.append(slice(s, s + n))
            s += n
        self.N = s
        self.ref = None

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
    base = hp.batch_live_workspaces()
    yield
    for c in _cases.values():
        c.close()
    _cases.clear()
    assert hp.batch_live_workspaces() == base


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
    """The reference: every column through group_HPCCG alone."""
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


def batch_solve(hp, gpu, cs, B, X0, max_iter, tol=0.0, pad=0):
    Bd = [dev(gpu, a, pad) for a in cs.split(B)]
    Xd = [dev(gpu, a, pad) for a in cs.split(X0)]
    its, nrs, times = hp.group_HPCCG_batch(cs.Ms, Bd, Xd, max_iter=max_iter, tolerance=tol)
    assert times[0] > 0.0
    X = [x.cpu().numpy() for x in Xd]
    if pad:
        for x, rw in zip(X, cs.rows):
            assert np.all(x[:, rw.stop - rw.start:] == 7.5)  # nothing stored between the columns
    return [([x[c, :rw.stop - rw.start].copy() for x, rw in zip(X, cs.rows)], int(its[c]), float(nrs[c]),
             hp.group_last_trace_batch(cs.Ms, c).copy()) for c in range(B.shape[0])]


def assert_same(got, ref):
    assert len(got) == len(ref)
    for c, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == r[1], (c, g[1], r[1])
        assert np.float64(g[2]).tobytes() == np.float64(r[2]).tobytes(), (c, g[2], r[2])
        assert g[3].tobytes() == r[3].tobytes(), (c, "trace")
        for m, (gx, rx) in enumerate(zip(g[0], r[0])):
            assert gx.tobytes() == rx.tobytes(), (c, "x of member", m, float(np.max(np.abs(gx - rx))))


# ---------------------------------------------------------------------------
# 1. SpMM against the CPU oracle of the global matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_spmm_columns_are_the_oracles_sparsemv(hp, gpu, shape):
    import torch
    cs = case(hp, shape)
    V = np.random.default_rng(21).uniform(-1.0, 1.0, (NCOL, cs.N))
    ref = np.stack([oracle.sparsemv(cs.A, V[c]) for c in range(NCOL)])
    for nrhs, pad in ((1, 0), (2, 3), (3, 0), (4, 3), (5, 0), (7, 3)):
        Xd = [dev(gpu, a, pad) for a in cs.split(V[:nrhs])]
        Yd = [torch.full_like(x, -3.0) for x in Xd]
        hp.group_sparsemv_batch(cs.Ms, Xd, Yd)
        for r, rw in enumerate(cs.rows):
            Y = Yd[r].cpu().numpy()
            n = rw.stop - rw.start
            for c in range(nrhs):
                assert Y[c, :n].tobytes() == ref[c, rw].tobytes(), (nrhs, r, c)
            assert np.all(Y[:, n:] == -3.0)


# ---------------------------------------------------------------------------
# 2. solve parity with the group solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_solve_columns_are_group_solves(hp, gpu, shape):
    cs = case(hp, shape)
    B, X0 = columns(cs)
    ref = single_solves(hp, gpu, cs, B, X0, MAX_ITER)
    assert ref[0][1] > 0
    for nrhs, pad in ((2, 0), (3, 3), (4, 0), (5, 3), (7, 0), (1, 3)):
        got = batch_solve(hp, gpu, cs, B[:nrhs], X0[:nrhs], MAX_ITER, pad=pad)
        assert_same(got, ref[:nrhs])


# ---------------------------------------------------------------------------
# 3. the serial reference's run of the z-stacked global problem
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["27pt_16x16x16_x8ranks", "27pt_8x8x8_x2ranks", "7pt_12x10x8_x2ranks"])
def test_batch_column_matches_global_reference(hp, gpu, golden, name):
    c = solve_case(golden, name)
    P = c["ranks"]
    cs = case(hp, {"27pt_16x16x16_x8ranks": "8x16c", "27pt_8x8x8_x2ranks": "2x8c",
                   "7pt_12x10x8_x2ranks": "2x12x10x8_7pt"}[name])
    assert cs.P == P and cs.N == c["nx"] * c["ny"] * c["nz"] * P
    rng = np.random.default_rng(77)
    B = np.stack([rng.uniform(-1.0, 1.0, cs.N), cs.A.b, 0.5 * cs.A.b])  # the generated b in column 1
    X0 = np.zeros((3, cs.N))
    got = batch_solve(hp, gpu, cs, B, X0, 500)
    xs, niters, normr, tr = got[1]
    ref_tr = [unhex(t) for t in c["trace_normr"]]
    rr = c["runs"]["500"]
    assert tr[0] == ref_tr[0]
    assert check_trace(tr, ref_tr, RTRANS_RTOL_MULTI) >= 5
    check_final(niters, normr, tr, rr["niters"], unhex(rr["normr"]), ref_tr, 500)
    assert max(np.max(np.abs(x - 1.0)) for x in xs) <= 1e-12


# ---------------------------------------------------------------------------
# 4. every column stops on its own
# ---------------------------------------------------------------------------
def test_columns_stop_at_their_own_iteration(hp, gpu):
    import torch
    cs = case(hp, "3x33x17x9")
    b = cs.A.b
    rng = np.random.default_rng(9)
    x0 = rng.uniform(-1.0, 1.0, cs.N)
    # b = A x0 by the group SpMM itself: the column's first residual is exactly zero
    Xd = [dev(gpu, a) for a in cs.split(np.stack([x0, x0]))]
    Yd = [torch.zeros_like(x) for x in Xd]
    hp.group_sparsemv_batch(cs.Ms, Xd, Yd)
    ax0 = np.concatenate([y[0].cpu().numpy() for y in Yd])
    B = np.stack([b, b * 1e-6, b * 1e6, ax0])
    X0 = np.zeros((4, cs.N))
    X0[3] = x0
    tol = 1e-3
    ref = single_solves(hp, gpu, cs, B, X0, 150, tol)
    stops = [r[1] for r in ref]
    assert stops[3] == 0 and ref[3][2] == 0.0  # its loop never runs
    assert len(set(stops)) >= 3 and max(stops) < 149, stops  # the reference itself staggers
    got = batch_solve(hp, gpu, cs, B, X0, 150, tol)
    assert [g[1] for g in got] == stops
    assert_same(got, ref)  # every member's x: a finished column stayed frozen while the others ran
    assert np.concatenate(got[3][0]).tobytes() == x0.tobytes()


# ---------------------------------------------------------------------------
# 5. isolation and lifetime
# ---------------------------------------------------------------------------
def test_group_solves_and_batches_do_not_disturb_each_other(hp, gpu):
    base = hp.batch_live_workspaces()
    cs = Case(hp, "3x33x17x9")
    try:
        B, X0 = columns(cs, 4)
        before = single_solves(hp, gpu, cs, B[:2], X0[:2], 40)
        first = batch_solve(hp, gpu, cs, B, X0, 40)
        after = single_solves(hp, gpu, cs, B[:2], X0[:2], 40)
        assert_same(after, before)
        for _ in range(3):
            assert_same(batch_solve(hp, gpu, cs, B, X0, 40), first)
        assert_same(first[:2], before)
        assert all(M.batch_workspace_bytes() > 0 for M in cs.Ms)
        assert hp.batch_live_workspaces() == base + cs.P
    finally:
        cs.close()
    assert hp.batch_live_workspaces() == base


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_the_process_working(hp, gpu):
    import torch
    L = hp.batch_lib()
    cs = case(hp, "2x8c")
    three = case(hp, "3x33x17x9")
    n = 512
    B, X0 = columns(cs, 2)
    Bd = [dev(gpu, a) for a in cs.split(B)]
    Xd = [dev(gpu, a) for a in cs.split(X0)]
    it = (C.c_int * 2)()
    nr = (C.c_double * 2)()

    def call(Ms, ldb=(n, n), ldx=(n, n), nrhs=2, max_iter=10, nranks=2):
        hs = (C.c_void_p * len(Ms))(*[M.h for M in Ms])
        bp = (C.c_void_p * 2)(*[t.data_ptr() for t in Bd])
        xp = (C.c_void_p * 2)(*[t.data_ptr() for t in Xd])
        return L.hpccg_hip_group_batch_solve_device(hs, nranks, nrhs, bp, (C.c_longlong * 2)(*ldb), xp,
                                                    (C.c_longlong * 2)(*ldx), max_iter, 0.0, it, nr, None)

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
        assert b"rank" in hp.lib().hpccg_hip_last_error()
        assert untouched()
        assert call(three.Ms[:2]) == EINVAL  # a subset of a group
        assert untouched()
        assert call([plain, plain]) == EINVAL  # a single-rank matrix in a 2-slot call
        assert untouched()
        assert call([cs.Ms[0], other[1]]) == EINVAL  # members of two groups
        assert b"another group" in hp.lib().hpccg_hip_last_error()
        assert untouched()
        assert call([cs.Ms[0], gather[1]]) == EINVAL  # ... one made from CSR parts, one generated
        assert b"another group" in hp.lib().hpccg_hip_last_error()
        assert call(gather) == EPLAN
        assert b"gather" in hp.lib().hpccg_hip_last_error()
        assert untouched()
        assert call(cs.Ms, ldb=(n, n - 1)) == EINVAL
        assert call(cs.Ms, ldx=(n - 1, n)) == EINVAL
        assert call(cs.Ms, nrhs=0) == EINVAL
        assert call(cs.Ms, max_iter=-1) == EINVAL
        assert untouched()
        with pytest.raises(hp.HPCCGError):
            hp.group_sparsemv_batch(cs.Ms[::-1], Xd, Bd)
        with pytest.raises(hp.HPCCGError):
            hp.group_HPCCG_batch(gather, Bd, Xd, max_iter=10)
        assert untouched()
        assert torch.cuda.current_device() == dev0
        # the single-rank batch keeps refusing a member
        for m in cs.Ms:
            assert L.hpccg_hip_batch_solve_device(m.h, 2, Bd[0].data_ptr(), n, Xd[0].data_ptr(), n, 10, 0.0, it, nr,
                                                  None) == EINVAL
            assert b"batch" in hp.lib().hpccg_hip_last_error()
        assert untouched()
    finally:
        for M in other + gather + [plain]:
            M.close()
    # ... and a good batch afterwards
    assert_same(batch_solve(hp, gpu, cs, B, X0, 10), single_solves(hp, gpu, cs, B, X0, 10))


def test_group_of_one_is_the_single_rank_batch(hp, gpu):
    (Mg,) = hp.group_generate(12, 11, 10, 1)
    M = hp.Matrix.generate(12, 11, 10)
    try:
        A = oracle.generate(12, 11, 10)
        rng = np.random.default_rng(3)
        B = np.stack([A.b, rng.uniform(-1.0, 1.0, A.nrow), 0.5 * A.b])
        Bd, Xd = dev(gpu, B), dev(gpu, np.zeros_like(B))
        its, nrs, _ = hp.group_HPCCG_batch([Mg], [Bd], [Xd], max_iter=40)
        Xs = dev(gpu, np.zeros_like(B))
        _, its1, nrs1, _ = hp.HPCCG_batch(M, Bd, Xs, max_iter=40, device=True)
        assert list(its) == list(its1) and nrs.tobytes() == nrs1.tobytes()
        assert Xd.cpu().numpy().tobytes() == Xs.cpu().numpy().tobytes()
        for c in range(3):
            assert hp.group_last_trace_batch([Mg], c).tobytes() == M.last_trace_batch(c).tobytes()
    finally:
        Mg.close()
        M.close()
