"""The non-temporal kernel forms of every library (option "nt",
include/hpccg_hip.h): each library picks its SpMV / SpMM form from one flag,
which the image's size sets (beyond 256e6 bytes: 27-pt 106^3, 7-pt about
4.6 M rows, SELL-512 beyond 21 M slots), so the other modules' shapes never
run those forms. Here the flag is forced at small shapes.

The reference throughout is the same call with the flag the other way: the
nt = 0 forms are held to the oracle, the single solve and the NumPy
restatements by the other modules. Comparisons are bitwise: x, niters, normr
and the whole trace per column; every byte of Y with the padding untouched.

  a. nt forced to 1 at small shapes, every image form (widths 27, 7,
     per-slice, SELL-512; exact and inexact fp32 images), 5 / 4 (ld = n + 3) /
     2 / 1 columns: batch, mixed, pcg (Jacobi and m = 1), poly and poly32
     (degrees 0, 2, 3), and the two SpMM entry points -- those against the
     oracle too, which catches what both forms could share;
  b. the in-process groups, every member forced and one member forced;
  c. the single solve under its kernel, fusion, resident and graph options;
  d. the automatic flag at its smallest natural shape, 27-pt 106^3, against
     nt forced to 0, the single solve and the oracle;
  e. refusals, and nothing left behind.

Two sets of right-hand sides everywhere: a chunk with an ended column runs
the SpMM's general slot loop (neither the nt arm nor the x-triple plan), so
beside the usual columns() -- whose column 2 starts at the solution -- there
is a set whose columns all run to max_iter (active_columns).

What the cases reach, from a build whose non-temporal loaders returned their
rows swapped: every test here failed but three kinds. The fp64 SpMM over
SELL-512 (spmm_sell_body) has one form, so pcg and poly on the three SELL-512
shapes have no nt arm to run and only hold that the flag disturbs nothing;
batch there runs it through its one-column call, which is the single solve
(k_spmv_sell); test_the_flag_turns_at_106 runs no kernel.
"""
import numpy as np
import pytest

import oracle
import test_gpu_batch as tb
import test_gpu_mixed as tm
import test_gpu_pcg as tp
import test_gpu_pcg_group as tpg
import test_gpu_poly as tpoly
import test_gpu_poly32 as tp32
import test_gpu_poly_group as tpolyg
from test_gpu_mixed import assert_same, columns, dev

pytestmark = pytest.mark.gpu

EINVAL = -1
MAX_ITER = 25
# 33c: 71 slices, interior ones on the triple plan, a 97-row tail slice, two dot groups
EXACT = ["33c", "16c", "12x10x16_7pt", "band600", "dyadic_csr513", "dyadic_csr3000"]
INEXACT = ["p10_33c", "p10_band600", "p10_dyadic_csr513", "pert_16c"]
SHAPES = EXACT + INEXACT
FORMS = ((5, 0), (4, 3), (2, 0), (1, 0))  # (columns, ld - n): a chunk of four and a remainder, ...
LIBS = ["batch", "mixed", "pcg", "poly", "poly32"]

_own = []  # matrices of this module alone


def problem(hp, name):
    """(Matrix, oracle.CSR with b = A 1) from the other modules' caches."""
    M, A, _ = tm.problem(hp, name) if name.startswith("pert_") else tp.problem(hp, name)
    return M, A


def live(hp):
    return (hp.batch_live_workspaces(), hp.mixed_live_workspaces(), hp.pcg_live_workspaces(),
            hp.poly_live_workspaces(), hp.poly32_live_workspaces(), hp.group_pcg_live_workspaces(),
            hp.group_poly_live_workspaces())


@pytest.fixture(scope="module", autouse=True)
def _close_everything(hp):
    yield
    for cache in (tm._problems, tp._problems):
        for M, _, _ in cache.values():
            M.close()
        cache.clear()
    for M in _own:
        M.close()
    _own.clear()
    assert live(hp) == (0,) * 7


def active_columns(b, nrhs, seed=6):
    """Right-hand sides and guesses whose columns all run to max_iter under a
    zero tolerance: b; b / 8 from a nonzero guess; uniform random vectors."""
    n = len(b)
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1.0, 1.0, (nrhs, n))
    X0 = np.zeros((nrhs, n))
    B[0] = b
    if nrhs > 1:
        B[1] = b * 2.0 ** -3
        X0[1] = 0.25 * ((np.arange(n) % 7) - 3)
    return B, X0


def both_ways(Ms, forced, run, same):
    """run() with the automatic flag (0 at these shapes), with the members
    `forced` at 1, and with the automatic flag again: the same bits all three
    times. Returns the first result."""
    assert [M.get_option("nt") for M in Ms] == [0] * len(Ms)
    ref = run()
    try:
        for M in forced:
            M.set_option("nt", 1)
            assert M.get_option("nt") == 1
        got = run()
    finally:
        for M in forced:
            M.set_option("nt", -1)
    assert [M.get_option("nt") for M in Ms] == [0] * len(Ms)
    again = run()
    same(got, ref)
    same(again, ref)  # nothing of the forced run stays
    return ref


# ---------------------------------------------------------------------------
# a. nt forced to 1 at small shapes: the one-rank libraries
# ---------------------------------------------------------------------------
def solves(hp, gpu, lib, M, B, X0, ld, active):
    """Every variant of a library's solve on one column set, in one list."""
    kw = dict(ld=ld)
    if lib == "batch":
        return tb.batch_solve(hp, gpu, M, B, X0, MAX_ITER, **kw)
    if lib == "mixed":
        # (an inexact image: one sweep that spends every iteration keeps all columns running)
        extra = dict(max_sweeps=1, inner_rtol=0.0) if active else {}
        return tm.mixed_solve(hp, gpu, M, B, X0, MAX_ITER, **kw, **extra)
    if lib == "pcg":
        return sum((tp.pcg_solve(hp, gpu, M, B, X0, MAX_ITER, minv=m, **kw) for m in (None, 1.0)), [])
    solve = tpoly.poly_solve if lib == "poly" else tp32.poly32_solve
    return sum((solve(hp, gpu, M, B, X0, MAX_ITER, degree=d, **kw) for d in (0, 2, 3)), [])


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forced_nt_solves(hp, gpu, shape, lib):
    M, A = problem(hp, shape)
    n = A.nrow
    same = (lambda g, r: assert_same(g, r, sweeps=True)) if lib == "mixed" else assert_same
    for active in (True, False):
        B, X0 = active_columns(A.b, 5) if active else columns(A.b, A.xexact, 5)
        for nrhs, pad in FORMS:
            ref = both_ways([M], [M], lambda: solves(hp, gpu, lib, M, B[:nrhs], X0[:nrhs], n + pad, active), same)
            if active:
                assert [r[1] for r in ref] == [MAX_ITER - 1] * len(ref), (nrhs, [r[1] for r in ref])
            elif nrhs > 2:
                assert ref[2][1] == 0 and ref[0][1] > 0  # the ended column beside running ones


@pytest.mark.parametrize("shape", SHAPES)
def test_forced_nt_spmm(hp, gpu, shape):
    import torch
    M, A = problem(hp, shape)
    n = A.nrow
    A32 = oracle.CSR(A.row_ptr, A.cols, A.vals.astype(np.float32).astype(np.float64), None, None, None)
    V = np.random.default_rng(21).uniform(-1.0, 1.0, (5, n))

    def same(got, ref):
        assert got.tobytes() == ref.tobytes()

    for spmm, Aref in ((hp.HPC_sparsemv_batch, A), (hp.HPC_sparsemv_mixed, A32)):
        want = oracle.sparsemv(Aref, V[0])

        def run(nrhs, pad):
            Xd = dev(gpu, V[:nrhs], n + pad)
            Yd = torch.full((nrhs, n + pad), -3.0, dtype=torch.float64, device=gpu)
            spmm(M, Xd, Yd)
            Y = Yd.cpu().numpy()
            assert np.all(Y[:, n:] == -3.0)
            if M.get_option("nt") == 1:  # the oracle: what the two forms could share
                assert Y[0, :n].tobytes() == want.tobytes(), (nrhs, float(np.max(np.abs(Y[0, :n] - want))))
            return Y

        for nrhs, pad in FORMS:
            both_ways([M], [M], lambda: run(nrhs, pad), same)

    def spmv():
        y = torch.zeros(n, dtype=torch.float64, device=gpu)
        hp.HPC_sparsemv(M, torch.from_numpy(V[0].copy()).to(gpu), y)
        return y.cpu().numpy()

    want = oracle.sparsemv(A, V[0])
    assert both_ways([M], [M], spmv, same).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------
# b. the in-process groups
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["single", "batch", "pcg", "poly"])
@pytest.mark.parametrize("shape", ["2x16x16x8", "2x12x10x8_7pt"])
def test_forced_nt_groups(hp, gpu, shape, lib):
    cs = tpg.Case(hp, shape)
    _own.extend(cs.Ms)
    assert cs.P == 2
    B, X0 = active_columns(cs.A.b, 4)

    def run():
        if lib == "single":
            return tpg.single_solves(hp, gpu, cs, B, X0, MAX_ITER)
        if lib == "batch":
            return tpg.batch_solve(hp, gpu, cs, B, X0, MAX_ITER)
        if lib == "pcg":
            return tpg.pcg_solve(hp, gpu, cs, B, X0, MAX_ITER, pad=3)
        return tpolyg.poly_solve(hp, gpu, cs, B, X0, MAX_ITER, degree=2, pad=3)

    try:
        # every member; then member 0 alone: members run their own kernels, so the bits do not move
        for forced in (cs.Ms, cs.Ms[:1]):
            ref = both_ways(cs.Ms, forced, run, tpg.assert_same)
            assert [r[1] for r in ref] == [MAX_ITER - 1] * 4
    finally:
        for M in cs.Ms:
            _own.remove(M)
            M.close()


# ---------------------------------------------------------------------------
# c. the single solve
# ---------------------------------------------------------------------------
def kept_sell(hp, name):
    """A matrix of this module with its SELL-512 image kept beside SELL-512-A."""
    hp.set_keep_sell(True)
    try:
        if name in tm.STENCILS:
            nx, ny, nz, s7 = tm.STENCILS[name]
            prob = hp.generate_matrix(nx, ny, nz, use_7pt=s7)
            M = hp.Matrix.from_hpc(prob)
            b = prob.b.copy()
            prob.close()
        else:
            A = tp.base_csr(name)
            M, b = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals), A.b.copy()
    finally:
        hp.set_keep_sell(False)
    _own.append(M)
    return M, b


def single(hp, M, b):
    x = np.zeros(len(b))
    ierr, it, nr, _ = hp.HPCCG(M, b, x, max_iter=MAX_ITER)
    assert ierr == 0
    return it, np.float64(nr).tobytes(), M.last_trace().tobytes(), x.tobytes()


@pytest.mark.parametrize("shape", ["33c", "12x10x16_7pt", "band600", "dyadic_csr3000"])
def test_forced_nt_single_solve_options(hp, gpu, shape):
    M, b = kept_sell(hp, shape)
    try:
        width = M.get_option("a_width") if M.get_option("has_a") else None
        assert width == {"33c": 27, "12x10x16_7pt": 7, "band600": 0, "dyadic_csr3000": None}[shape]
        assert M.get_option("has_sell") == 1 and M.get_option("nt") == 0
        if shape == "33c":
            assert M.get_option("resident_update") == 8  # the persistent launch is this shape's default
        base = single(hp, M, b)
        assert base[0] == MAX_ITER - 1
        M.set_option("graph_chunk", 8)  # (graphs replay from 8 iterations on)
        M.set_option("nt", 1)
        assert M.get_option("nt") == 1
        assert M.get_option("resident_update") in (0, 1)  # never the persistent launch while forced
        kernels = []
        for kernel in (0, 1, 2):
            try:
                M.set_option("spmv_kernel", kernel)
            except hp.HPCCGError:  # its image does not exist for this matrix
                continue
            kernels.append(kernel)
            for fuse_p in (0, -1):
                for fuse_update in (0, 1):
                    for resident in (0, 1):
                        for graph in (0, 1):
                            opts = dict(fuse_p=fuse_p, fuse_update=fuse_update, resident_update=resident,
                                        use_graph=graph)
                            for k, v in opts.items():
                                M.set_option(k, v)
                            assert M.get_option("nt") == 1 and M.get_option("resident_update") != 8
                            assert single(hp, M, b) == base, (kernel, opts)
        has = [M.get_option(k) for k in ("has_sell", "has_a", "has_pairs")]
        assert kernels == [k for k in (0, 1, 2) if has[k]] and has[:2] == [1, int(width is not None)], kernels
        if shape == "33c":
            assert kernels == [0, 1, 2]
        for k in ("spmv_kernel", "fuse_p", "fuse_update", "resident_update"):
            M.set_option(k, -1)
        M.set_option("nt", -1)
        assert M.get_option("nt") == 0
        assert single(hp, M, b) == base
    finally:
        _own.remove(M)
        M.close()


def test_a_changed_flag_recaptures_the_graph(hp, gpu):
    M, b = kept_sell(hp, "33c")
    try:
        base = single(hp, M, b)
        M.set_option("graph_chunk", 8)
        M.set_option("resident_update", 0)  # (the per-iteration launches: those are captured)
        for nt in (-1, 1, -1, 1, 0, 1):
            M.set_option("nt", nt)
            assert M.get_option("nt") == max(nt, 0)
            assert single(hp, M, b) == base, nt
            assert M.get_option("graph_used") == 1
        # the resident per-iteration launch stays selectable under the forced flag
        M.set_option("resident_update", 1)
        assert M.get_option("resident_update") == 1
        assert single(hp, M, b) == base
    finally:
        _own.remove(M)
        M.close()


# ---------------------------------------------------------------------------
# d. the automatic flag at the smallest natural shape
# ---------------------------------------------------------------------------
BIG = 106
BIG_ITER = 8


class Big:
    """27-pt 106^3 on the device: four columns that all run and a remainder
    column, and each column's single solve."""

    def __init__(self, hp, gpu):
        import torch
        self.M = hp.Matrix.generate(BIG, BIG, BIG)
        _own.append(self.M)
        n = self.n = int(self.M.info()["nrow"])
        b = torch.zeros(n, dtype=torch.float64, device=gpu)
        hp.HPC_sparsemv(self.M, torch.ones(n, dtype=torch.float64, device=gpu), b)  # b = A 1, exact
        g = torch.arange(n, dtype=torch.float64, device=gpu)
        gen = torch.Generator(device=gpu)
        gen.manual_seed(7)
        rnd = torch.rand((3, n), dtype=torch.float64, device=gpu, generator=gen) * 2.0 - 1.0
        self.B = torch.cat([torch.stack([b, b * 2.0 ** -3]), rnd])
        self.X0 = torch.zeros_like(self.B)
        self.X0[1] = 0.25 * (torch.remainder(g, 7) - 3)
        self.ref = []
        for c in range(5):
            x = self.X0[c].clone()
            ierr, it, nr, _ = hp.HPCCG(self.M, self.B[c], x, max_iter=BIG_ITER, device=True)
            assert ierr == 0 and it == BIG_ITER - 1
            self.ref.append((x, it, np.float64(nr).tobytes(), self.M.last_trace().tobytes()))


@pytest.fixture(scope="module")
def big(hp, gpu):
    return Big(hp, gpu)


def test_the_flag_turns_at_106(hp, gpu, big):
    info = big.M.info()
    assert info["nrow"] == BIG ** 3 and info["uniform_width"] == 27
    assert info["slots"] * 8 == 2327 * 27 * 512 * 8 == 257347584 > 256e6
    assert big.M.get_option("nt") == 1
    M = hp.Matrix.generate(BIG - 1, BIG - 1, BIG - 1)
    try:
        assert M.info()["slots"] * 8 == 2261 * 27 * 512 * 8 == 250048512 <= 256e6
        assert M.get_option("nt") == 0
    finally:
        M.close()


def big_solve(hp, gpu, big, lib, m1=False):
    """(X, [(niters, normr, trace)] per column) of one library's five-column solve, on the device."""
    import torch
    M, Xd = big.M, big.X0.clone()
    kw = dict(max_iter=BIG_ITER, device=True)
    if m1:
        kw["minv"] = torch.ones(big.n, dtype=torch.float64, device=gpu)
    call, trace = {"batch": (hp.HPCCG_batch, M.last_trace_batch), "mixed": (hp.HPCCG_mixed, M.last_trace_mixed),
                   "pcg": (hp.HPCCG_pcg, M.last_trace_pcg), "poly": (hp.HPCCG_poly, M.last_trace_poly),
                   "poly32": (hp.HPCCG_poly32, M.last_trace_poly32)}[lib]
    if lib in ("poly", "poly32"):
        kw["degree"] = 2
    ierr, its, nrs, _ = call(M, big.B, Xd, **kw)
    assert ierr == 0
    return Xd, [(int(its[c]), np.float64(nrs[c]).tobytes(), trace(c).tobytes()) for c in range(5)]


@pytest.mark.parametrize("lib", LIBS)
def test_automatic_nt_is_nt_forced_off(hp, gpu, big, lib):
    import torch
    M = big.M
    release = getattr(M, lib + "_release")
    try:
        assert M.get_option("nt") == 1
        runs = [False] + ([True] if lib == "pcg" else [])  # pcg: Jacobi, and m = 1
        auto = [big_solve(hp, gpu, big, lib, m1) for m1 in runs]
        M.set_option("nt", 0)
        try:
            assert M.get_option("nt") == 0
            off = [big_solve(hp, gpu, big, lib, m1) for m1 in runs]
        finally:
            M.set_option("nt", -1)
        assert M.get_option("nt") == 1
        for (Xa, ra), (Xo, ro) in zip(auto, off):
            assert [r[0] for r in ra] == [BIG_ITER - 1] * 5
            assert ra == ro
            assert torch.equal(Xa, Xo)
        if lib in ("batch", "mixed", "pcg"):  # ... and each column is the single solve
            X, res = auto[-1]
            for c in range(5):
                assert res[c] == big.ref[c][1:], c
                assert torch.equal(X[c], big.ref[c][0]), c
    finally:
        release()


def test_automatic_nt_spmm_is_the_oracle(hp, gpu, big):
    import torch
    M, n = big.M, big.n
    A = oracle.generate(BIG, BIG, BIG)
    try:
        assert M.get_option("nt") == 1
        Yd = torch.full((5, n + 3), -3.0, dtype=torch.float64, device=gpu)
        hp.HPC_sparsemv_batch(M, big.B, Yd)
        want = oracle.sparsemv(A, big.B[2].cpu().numpy())
        assert Yd[2, :n].cpu().numpy().tobytes() == want.tobytes()
        assert torch.all(Yd[:, n:] == -3.0)
        M.set_option("nt", 0)
        try:
            Y0 = torch.full((5, n + 3), -3.0, dtype=torch.float64, device=gpu)
            hp.HPC_sparsemv_batch(M, big.B, Y0)
        finally:
            M.set_option("nt", -1)
        assert torch.equal(Yd, Y0)
    finally:
        M.batch_release()


# ---------------------------------------------------------------------------
# e. refusals
# ---------------------------------------------------------------------------
def test_other_values_are_refused(hp, gpu):
    M, A = problem(hp, "16c")
    B, X0 = active_columns(A.b, 2)
    ref = tb.batch_solve(hp, gpu, M, B, X0, MAX_ITER)
    for start in (-1, 1):
        M.set_option("nt", start)
        for bad in (2, -2):
            assert hp.lib().hpccg_hip_set_option(M.h, b"nt", bad) == EINVAL
            assert b"nt must be" in hp.lib().hpccg_hip_last_error()
            with pytest.raises(hp.HPCCGError):
                M.set_option("nt", bad)
            assert M.get_option("nt") == max(start, 0)  # the flag is as it was
        assert_same(tb.batch_solve(hp, gpu, M, B, X0, MAX_ITER), ref)
    M.set_option("nt", -1)
    assert M.get_option("nt") == 0
