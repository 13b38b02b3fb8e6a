"""Degenerate and non-finite columns through the multi-column solvers (the
column engine of csrc/hpccg_columns.h: batch, mixed, pcg and the two group
forms). tests/test_gpu_edge.py has these starts for the single solve; here they
are columns of a call:

  a. a bad column is, as a column, what the single solve makes of it (niters 0
     or 2, normr 0 or NaN, x untouched or all NaN) -- and with it the oracle;
  b. Jacobi and a caller's m: the outcome of the NumPy restatement;
  c. isolation: a finite column beside bad ones is bitwise the single-column
     call on it, wherever the bad ones stand, across the host's read of the
     "ended" word, through the host entry point too;
  d. nothing carried: after bad calls the same finite calls give the same bits
     from the same workspace, the SpMM is the oracle's, the other solvers on
     the matrix are unchanged;
  e. the refinement on a residual that is not finite or exactly zero ends at
     that residual step with x0 bit for bit (include/hpccg_hip_mixed.h, step 2).

The columns, the arrangements and the expected outcomes are those of
tests/columns_cases.py, which tests/test_columns_edge_cpu.py pins: every
expected value is exact, so nothing here has a tolerance. NaN and inf are data
to kernels that index by the matrix alone.

Shapes (the smallest that reach each image form and row kind): 16^3 (width 27,
8 full slices, the x-triple plan with four columns), 12x10x16 7-pt (width 7, a
tail slice), band600 (per-slice widths), dyadic_csr513 (SELL-512, one row in
the last slice), their "p2_" forms for Jacobi, plain_csr513 and pert_16c (the
refinement); groups of 2 x 12x10x8 27-pt (the bad entry on member 0's last
plane, on member 1's first, well inside member 1) and csr3.
"""
import math

import numpy as np
import pytest

import columns_cases as cc
import oracle
import test_gpu_batch as tb
import test_gpu_batch_group as tbg
import test_gpu_mixed as tm
import test_gpu_pcg as tp
import test_gpu_pcg_group as tpg
from test_gpu_edge import same as same_as_oracle

pytestmark = pytest.mark.gpu

MAX_ITER = cc.MAX_ITER
P2 = ["p2_" + s for s in cc.EXACT]


# ---------------------------------------------------------------------------
# problems and libraries
# ---------------------------------------------------------------------------
def prob(hp, shape):
    """(Matrix, oracle.CSR with b = A 1) from the column suites' own caches."""
    M, A, _ = (tm if shape in cc.REFINED else tp).problem(hp, shape)
    return M, A


_groups = {}


def group(hp, name):
    """A group case with the interface of test_gpu_pcg_group.Case."""
    if name not in _groups:
        if name == "csr3":
            cs = tpg.Case(hp, "csr3")
            cs.inf_rows = cc.group_rows(tpg.CSR_SLABS)
        else:  # 2 x 12x10x8 27-pt (that of test_gpu_edge.test_degenerate_starts_group)
            nx, ny, nz, P = 12, 10, 8, 2
            n = nx * ny * nz
            cs = object.__new__(tpg.Case)
            cs.A, cs.s, cs.has_a, cs.P, cs.N = oracle.generate(nx, ny, nz * P), None, 1, P, n * P
            cs.Ms = hp.group_generate(nx, ny, nz, P)
            cs.rows = [slice(r * n, (r + 1) * n) for r in range(P)]
            cs.inf_rows = cc.group_rows([n] * P, nx, ny)
        _groups[name] = cs
    return _groups[name]


@pytest.fixture(scope="module", autouse=True)
def _close_everything(hp):
    yield
    for mod in (tm, tp):
        for M, _, _ in mod._problems.values():
            M.close()
        mod._problems.clear()
    for cs in _groups.values():
        cs.close()
    _groups.clear()


def _flat(res):
    """A group suite's per-member x as one global vector."""
    return [(np.concatenate(r[0]),) + tuple(r[1:]) for r in res]


class Lib:
    """One multi-column library on one matrix (or group): run() the call,
    one() the single-column call a column must equal, workspace_bytes() per matrix."""

    def __init__(self, hp, gpu, name, shape):
        self.hp, self.gpu, self.name, self.shape = hp, gpu, name, shape
        self.group = name.startswith("g_")
        self.sweeps = name == "refine"
        self.kw = {}  # (refine: max_sweeps, inner_rtol)
        if self.group:
            self.cs = group(hp, shape)
            self.A = self.cs.A
        else:
            self.M, self.A = prob(hp, shape)
        self._refs = {}

    def run(self, B, X0, mi, tol=0.0):
        hp, gpu, n = self.hp, self.gpu, self.name
        if n == "batch":
            return tb.batch_solve(hp, gpu, self.M, B, X0, mi, tol)
        if n in ("mixed", "refine"):
            return tm.mixed_solve(hp, gpu, self.M, B, X0, mi, tol, **self.kw)
        if n in ("pcg1", "jacobi"):
            return tp.pcg_solve(hp, gpu, self.M, B, X0, mi, tol, minv=1.0 if n == "pcg1" else None)
        if n == "g_batch":
            return _flat(tbg.batch_solve(hp, gpu, self.cs, B, X0, mi, tol))
        return _flat(tpg.pcg_solve(hp, gpu, self.cs, B, X0, mi, tol, minv=1.0 if n == "g_pcg1" else None,
                                   halo_copies=n == "g_jacobi_copies"))

    def one(self, b, x0, mi, tol=0.0):
        """The single-column call: the single (or group) solve where the
        library is bitwise that, else the library's own one-column call."""
        key = (b.tobytes(), x0.tobytes(), mi, tol)
        if key not in self._refs:
            B, X0 = b.reshape(1, -1).copy(), x0.reshape(1, -1).copy()
            n = self.name
            if n in ("batch", "mixed", "pcg1"):
                r = tm.single_solves(self.hp, self.gpu, self.M, B, X0, mi, tol)[0]
            elif n in ("g_batch", "g_pcg1"):
                r = _flat(tbg.single_solves(self.hp, self.gpu, self.cs, B, X0, mi, tol))[0]
            else:
                r = self.run(B, X0, mi, tol)[0]
            self._refs[key] = r
        return self._refs[key]

    def host_run(self, B, X0, mi, tol=0.0):
        """The same call through the host entry point (one-rank libraries)."""
        hp, M, n = self.hp, self.M, self.name
        X = X0.copy()
        if n == "batch":
            _, its, nrs, _ = hp.HPCCG_batch(M, B.copy(), X, max_iter=mi, tolerance=tol)
            return [(X[c], int(its[c]), float(nrs[c]), M.last_trace_batch(c).copy()) for c in range(len(B))]
        if n in ("mixed", "refine"):
            _, its, nrs, _ = hp.HPCCG_mixed(M, B.copy(), X, max_iter=mi, tolerance=tol)
            return [(X[c], int(its[c]), float(nrs[c]), M.last_trace_mixed(c).copy(), M.last_sweeps_mixed(c))
                    for c in range(len(B))]
        minv = np.ones(B.shape[1]) if n == "pcg1" else None
        _, its, nrs, _ = hp.HPCCG_pcg(M, B.copy(), X, max_iter=mi, tolerance=tol, minv=minv)
        return [(X[c], int(its[c]), float(nrs[c]), M.last_trace_pcg(c).copy()) for c in range(len(B))]

    def workspace_bytes(self):
        if self.name in ("g_batch",):
            return [M.batch_workspace_bytes() for M in self.cs.Ms]
        if self.group:
            return [self.hp.group_pcg_workspace_bytes(M) for M in self.cs.Ms]
        return [{"batch": self.M.batch_workspace_bytes, "mixed": self.M.mixed_workspace_bytes,
                 "refine": self.M.mixed_workspace_bytes, "pcg1": self.M.pcg_workspace_bytes,
                 "jacobi": self.M.pcg_workspace_bytes}[self.name]()]

    def cases(self):
        if self.group:
            return cc.cases(self.A, self.cs.inf_rows)
        return cc.shape_cases(self.shape, self.A)


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def same_outcome(got, ref, sweeps=False):
    """A bad column against its reference: niters equal, normr equal or both
    NaN, x and trace equal with NaN where the reference's is NaN."""
    assert got[1] == ref[1], ("niters", got[1], ref[1])
    assert got[2] == ref[2] or (math.isnan(got[2]) and math.isnan(ref[2])), ("normr", got[2], ref[2])
    assert np.array_equal(got[0], ref[0], equal_nan=True), "x"
    assert np.array_equal(got[3], ref[3], equal_nan=True), ("trace", got[3], ref[3])
    if sweeps:
        assert np.array_equal(got[4][0], ref[4][0]) and np.array_equal(got[4][1], ref[4][1], equal_nan=True), \
            ("sweeps", got[4], ref[4])


def check_call(lib, label, cols, got, FB, FX, by_name, mi, tol):
    """Every finite column bitwise the single-column call on it, every bad
    column the outcome it has alone."""
    assert len(got) == len(cols)
    for c, col in enumerate(cols):
        try:
            if isinstance(col, int):
                tm.assert_same([got[c]], [lib.one(FB[col], FX[col], mi, tol)], sweeps=lib.sweeps)
                assert np.all(np.isfinite(got[c][0]))
            else:
                b, x0 = by_name[col]
                same_outcome(got[c], lib.one(b, x0, mi, tol), lib.sweeps)
        except AssertionError as e:
            raise AssertionError(f"{lib.name}/{lib.shape} {label} column {c} ({col}): {e}") from None


def bad_calls(lib):
    """(FB, FX, by_name, [(label, cols, B, X0, max_iter, tol)]) of a library's matrix."""
    FB, FX = cc.finite_columns(lib.A.b, lib.A.xexact)
    todo = lib.cases()
    by_name = {name: (b, x0) for name, b, x0, _, _ in todo}
    calls = []
    for label, cols, tol in cc.arrangements([t[0] for t in todo]):
        B, X0 = cc.assemble(cols, FB, FX, by_name)
        calls.append((label, cols, B, X0, MAX_ITER, tol))
    return FB, FX, by_name, calls


# ---------------------------------------------------------------------------
# a. the bad column alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cc.EXACT)
def test_a_bad_column_is_the_single_solve_of_it(hp, gpu, shape):
    M, A = prob(hp, shape)
    n = A.nrow
    fb, fx = A.b.reshape(1, n), np.zeros((1, n))
    for name, b, x0, mi, tol in cc.shape_cases(shape, A):
        B, X0 = b.reshape(1, n).copy(), x0.reshape(1, n).copy()
        try:
            ref = tm.single_solves(hp, gpu, M, B, X0, mi, tol)[0]
            orc = oracle.hpccg(A, b=b, x=x0, max_iter=mi, tolerance=tol)
            same_as_oracle((ref[1], ref[2], ref[0]), orc)
            cc.degenerate(*ref, x0)
            fin = tm.single_solves(hp, gpu, M, fb, fx, mi, tol)[0]
            assert fin[1] == mi - 1
            # batch: nrhs = 2 (one column is handed to the single solve), the second finite
            got = tb.batch_solve(hp, gpu, M, np.concatenate([B, fb]), np.concatenate([X0, fx]), mi, tol)
            same_outcome(got[0], ref)
            tm.assert_same(got[1:], [fin])
            # mixed, exact: the kR = 1 launch; pcg with m = 1
            same_outcome(tm.mixed_solve(hp, gpu, M, B, X0, mi, tol)[0], ref)
            same_outcome(tp.pcg_solve(hp, gpu, M, B, X0, mi, tol, minv=1.0)[0], ref)
        except AssertionError as e:
            raise AssertionError(f"{shape}/{name}: {e}") from None


# ---------------------------------------------------------------------------
# b. Jacobi and a caller's m
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P2)
def test_jacobi_and_a_callers_m_follow_the_restatement(hp, gpu, shape):
    M, A = prob(hp, shape)
    n = A.nrow
    jac = 1.0 / tp.csr_diagonal(A)
    m_any = np.random.default_rng(17).uniform(0.25, 4.0, n)
    fb, fx = A.b.reshape(1, n), np.zeros((1, n))
    for name, b, x0, mi, tol in cc.shape_cases(shape, A):
        B, X0 = b.reshape(1, n).copy(), x0.reshape(1, n).copy()
        for tag, minv, arg in (("default", jac, None), ("1/diag", jac, jac), ("any", m_any, m_any)):
            try:
                x, it, nr, tr = cc.expect_pcg(A, b, x0, mi, tol, minv)
                got = tp.pcg_solve(hp, gpu, M, B, X0, mi, tol, minv=arg)[0]
                assert got[1] == it, (got[1], it)
                assert math.isnan(got[2]) == math.isnan(nr) and (got[2] == 0.0) == (nr == 0.0), (got[2], nr)
                assert len(got[3]) == len(tr)
                if it == 0:
                    assert got[0].tobytes() == x0.tobytes()
                else:
                    assert np.isnan(x).all() and np.isnan(got[0]).all()
                # ... and beside a finite column, which is bitwise its own call
                two = tp.pcg_solve(hp, gpu, M, np.concatenate([fb, B]), np.concatenate([fx, X0]), mi, tol, minv=arg)
                same_outcome(two[1], got)
                tm.assert_same(two[:1], tp.pcg_solve(hp, gpu, M, fb, fx, mi, tol, minv=arg))
            except AssertionError as e:
                raise AssertionError(f"{shape}/{name}/{tag}: {e}") from None


# ---------------------------------------------------------------------------
# c. isolation
# ---------------------------------------------------------------------------
ONE_RANK = ([("batch", s) for s in cc.EXACT] + [("mixed", s) for s in cc.EXACT] +
            [("refine", s) for s in cc.REFINED] + [("pcg1", "16c"), ("pcg1", "dyadic_csr513")] +
            [("jacobi", s) for s in P2])
GROUPS = [(g, s) for s in ("2x12x10x8", "csr3") for g in ("g_batch", "g_pcg1", "g_jacobi", "g_jacobi_copies")]


def _id(p):
    return f"{p[0]}-{p[1]}"


@pytest.mark.parametrize("which", ONE_RANK + GROUPS, ids=_id)
def test_finite_columns_do_not_see_the_bad_ones(hp, gpu, which):
    lib = Lib(hp, gpu, *which)
    FB, FX, by_name, calls = bad_calls(lib)
    for label, cols, B, X0, mi, tol in calls:
        got = lib.run(B, X0, mi, tol)
        check_call(lib, label, cols, got, FB, FX, by_name, mi, tol)
        if label == "3/two_bad" and not lib.group:  # the host entry point: the device call
            host = lib.host_run(B, X0, mi, tol)
            for c, col in enumerate(cols):
                if isinstance(col, int):
                    tm.assert_same([host[c]], [got[c]], sweeps=lib.sweeps)
                else:
                    same_outcome(host[c], got[c], lib.sweeps)
    # the bad columns of a group are the oracle's serial outcome of the global problem
    # (under Jacobi: the restatement's)
    if lib.group:
        for name, b, x0, mi, tol in lib.cases():
            r = lib.one(b, x0, mi, tol)
            if lib.name in ("g_batch", "g_pcg1"):
                same_as_oracle((r[1], r[2], r[0]), oracle.hpccg(lib.A, b=b, x=x0, max_iter=mi, tolerance=tol))
            else:
                x, it, nr, tr = cc.expect_pcg(lib.A, b, x0, mi, tol)
                assert r[1] == it and math.isnan(r[2]) == math.isnan(nr) and len(r[3]) == len(tr), (name, r[1:3], it, nr)
                assert r[0].tobytes() == x0.tobytes() if it == 0 else np.isnan(r[0]).all(), name


@pytest.mark.parametrize("which", [("batch", "16c"), ("mixed", "16c"), ("pcg1", "16c"), ("jacobi", "p2_16c"),
                                   ("refine", "pert_16c")], ids=_id)
def test_a_column_that_ended_in_the_prologue_across_the_ended_reads(hp, gpu, which):
    """max_iter 150 and a tolerance every finite column meets only after more
    than kCheckEvery = 32 iterations: the host reads the "ended" word with the
    nan_b column counted in it since the prologue."""
    lib = Lib(hp, gpu, *which)
    FB, FX = cc.finite_columns(lib.A.b, lib.A.xexact)
    FB, FX = FB[:3], FX[:3]
    nan_b = {name: (b, x0) for name, b, x0, _, _ in lib.cases()}["nan_b"]
    mi = 150
    if lib.sweeps:
        # every sweep's inner recurrence runs to the tolerance itself: the first one past the read
        tol, mi, lib.kw = 1e-12 * float(np.linalg.norm(lib.A.b)), 4000, {"inner_rtol": 0.0}
    else:
        # below every residual of every column's first 34 iterations
        full = [lib.one(FB[c], FX[c], mi, 0.0) for c in range(3)]
        tol = min(float(np.min(r[3][:34])) for r in full) * (1.0 - 2.0 ** -10)
    refs = [lib.one(FB[c], FX[c], mi, tol) for c in range(3)]
    firsts = [int(r[4][0][0]) if lib.sweeps else r[1] for r in refs]
    print(f"{lib.name}: tolerance {tol:.3e}, stops {[r[1] for r in refs]}")
    assert all(32 < f for f in firsts) and all(r[1] < mi - 1 and r[2] <= tol for r in refs), firsts
    for pos in (0, 3):
        cols = [0, 1, 2]
        cols.insert(pos, "nan_b")
        B, X0 = cc.assemble(cols, FB, FX, {"nan_b": nan_b})
        got = lib.run(B, X0, mi, tol)
        check_call(lib, f"long@{pos}", cols, got, FB, FX, {"nan_b": nan_b}, mi, tol)
        assert got[pos][1] == 0 and math.isnan(got[pos][2])


# ---------------------------------------------------------------------------
# d. nothing carried
# ---------------------------------------------------------------------------
def _spmm_is_the_oracles(lib):
    """The library's SpMM entry point (where it has one) against the oracle."""
    import torch
    hp, gpu, A = lib.hp, lib.gpu, lib.A
    V = np.random.default_rng(21).uniform(-1.0, 1.0, (3, A.nrow))
    if lib.name == "g_batch":
        ref = np.stack([oracle.sparsemv(A, V[c]) for c in range(3)])
        Xd = [tbg.dev(gpu, a) for a in lib.cs.split(V)]
        Yd = [torch.full_like(x, -3.0) for x in Xd]
        hp.group_sparsemv_batch(lib.cs.Ms, Xd, Yd)
        Y = np.concatenate([y.cpu().numpy() for y in Yd], axis=1)
    elif lib.name in ("batch", "mixed", "refine"):
        Aref = A if lib.name == "batch" else cc.fp32_image(A)
        ref = np.stack([oracle.sparsemv(Aref, V[c]) for c in range(3)])
        Xd = tm.dev(gpu, V)
        Yd = torch.full_like(Xd, -3.0)
        (hp.HPC_sparsemv_batch if lib.name == "batch" else hp.HPC_sparsemv_mixed)(lib.M, Xd, Yd)
        Y = Yd.cpu().numpy()
    else:
        return
    assert Y.tobytes() == ref.tobytes(), (lib.name, lib.shape, float(np.max(np.abs(Y - ref))))


def _others(lib, B, X0):
    """The single (or group) solve and the other libraries on the same matrix."""
    hp, gpu = lib.hp, lib.gpu
    if lib.group:
        single = _flat(tbg.single_solves(hp, gpu, lib.cs, B[:2], X0[:2], MAX_ITER))
        rest = [_flat(tbg.batch_solve(hp, gpu, lib.cs, B[:3], X0[:3], MAX_ITER)),
                _flat(tpg.pcg_solve(hp, gpu, lib.cs, B[:3], X0[:3], MAX_ITER))]
    else:
        single = tm.single_solves(hp, gpu, lib.M, B[:2], X0[:2], MAX_ITER)
        rest = [tb.batch_solve(hp, gpu, lib.M, B[:3], X0[:3], MAX_ITER),
                tm.mixed_solve(hp, gpu, lib.M, B[:3], X0[:3], MAX_ITER),
                tp.pcg_solve(hp, gpu, lib.M, B[:3], X0[:3], MAX_ITER)]
    return [single] + rest


@pytest.mark.parametrize("which", ONE_RANK + GROUPS, ids=_id)
def test_nothing_of_a_bad_call_is_carried(hp, gpu, which):
    lib = Lib(hp, gpu, *which)
    A = lib.A
    WB, WX = tm.columns(A.b, A.xexact, 5)
    _, _, _, calls = bad_calls(lib)
    before = _others(lib, WB, WX)
    wide = lib.run(WB, WX, MAX_ITER)  # the widest call: the workspace at its final capacity
    narrow = lib.run(WB[:2], WX[:2], MAX_ITER)
    size = lib.workspace_bytes()
    assert all(s > 0 for s in size)
    assert all(np.all(np.isfinite(r[0])) for r in wide)
    for label, cols, B, X0, mi, tol in calls:
        got = lib.run(B, X0, mi, tol)
        assert any(np.isnan(r[0]).any() or math.isnan(r[2]) or not np.isfinite(r[2]) or r[1] == 0 for r in got), label
        if label in ("4/nan_b@1", "5/bad@4", "3/two_bad"):
            _spmm_is_the_oracles(lib)
    tm.assert_same(lib.run(WB, WX, MAX_ITER), wide, sweeps=lib.sweeps)
    tm.assert_same(lib.run(WB[:2], WX[:2], MAX_ITER), narrow, sweeps=lib.sweeps)
    assert lib.workspace_bytes() == size  # the same vectors, not new ones
    after = _others(lib, WB, WX)
    for a, b in zip(after, before):
        tm.assert_same(a, b)


# ---------------------------------------------------------------------------
# e. the refinement on a residual that is not finite or exactly zero
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cc.REFINED)
def test_the_refinement_ends_at_a_degenerate_residual(hp, gpu, shape):
    M, A = prob(hp, shape)
    assert M.mixed_info()["exact"] == 0
    n = A.nrow
    FB, FX = cc.finite_columns(A.b, A.xexact)
    for name, b, x0, mi, tol in cc.shape_cases(shape, A):
        x0 = x0.copy()
        if x0[5] == 0.0:
            x0[5] = -0.0  # an empty sweep's x += 0 would turn it into +0.0
        x, it, nr, tr, (its, res) = cc.expect_refined(A, b, x0, mi, tol)
        assert it == 0 and len(its) == 0  # (test_columns_edge_cpu.py)
        B = np.stack([FB[0], b, FB[1]])
        X0 = np.stack([FX[0], x0, FX[1]])
        try:
            for got in (tm.mixed_solve(hp, gpu, M, B[1:2], X0[1:2], mi, tol)[0],
                        tm.mixed_solve(hp, gpu, M, B, X0, mi, tol)[1]):
                assert got[1] == it == 0
                assert list(got[4][0]) == list(its) and len(got[4][1]) == len(res) == 1, got[4]
                assert (got[2] == 0.0) if nr == 0.0 else not math.isfinite(got[2]), (got[2], nr)
                assert np.float64(got[4][1][0]).tobytes() == np.float64(got[2]).tobytes()
                assert len(got[3]) == len(tr) == 0
                assert got[0].tobytes() == x0.tobytes()  # signs of zero included
            # the finite neighbours: their own single-column calls, sweeps included
            three = tm.mixed_solve(hp, gpu, M, B, X0, mi, tol)
            for c in (0, 2):
                alone = tm.mixed_solve(hp, gpu, M, B[c:c + 1], X0[c:c + 1], mi, tol)
                tm.assert_same(three[c:c + 1], alone, sweeps=True)
                assert three[c][1] > 0 and np.all(np.isfinite(three[c][0]))
        except AssertionError as e:
            raise AssertionError(f"{shape}/{name}: {e}") from None
