"""CPU-only checks of the BiCGStab library (lib/bicgstab/libhpccg_hip_bicgstab.so,
include/hpccg_hip_bicgstab.h): it is built one directory below the main library, exports
what its header declares, refuses bad arguments before touching HIP, and its
kernels keep their budget (read from its gfx950 code object): no spills,
scratch <= 32 B, the SpMM kernels <= 128 VGPRs, the others <= 64, one SpMM form
per form of the pcg library with as many non-temporal value loads. No other
library knows of it.

The NumPy restatement the GPU tests hold the solver to
(bicgstab_cases.restated_bicg) is pinned here: the window on which it agrees
with itself under two dot orders is long enough on every test matrix, the two
exact identities of the header hold bit for bit, and the degenerate columns end
as the header says.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bicgstab_cases as bc
import oracle
from bicgstab_cases import restated_bicg
from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes

EINVAL = -1
NAMES = ("abi_version", "solve_device", "solve", "last_trace", "last_status", "release", "workspace_bytes",
         "live_workspaces")


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.BICGSTAB_LIB_PATH), "run build(): libhpccg_hip_bicgstab.so is missing"
    declared = hp.bicgstab_exported_symbols()
    assert declared == sorted("hpccg_hip_bicgstab_" + s for s in NAMES), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.BICGSTAB_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the eight
    L = hp.bicgstab_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the fourteenth library only
    assert "hpccg_hip_bicgstab" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    # (it has lib/bicgstab/ to itself: lib/ holds the thirteen libraries of the CG family, and their tests count them)
    libdir = os.path.dirname(hp.BICGSTAB_LIB_PATH)
    assert libdir == os.path.join(hp.HERE, "lib", "bicgstab") and os.listdir(libdir) == ["libhpccg_hip_bicgstab.so"]
    others = sorted(os.path.join(hp.HERE, "lib", f) for f in os.listdir(os.path.join(hp.HERE, "lib")) if f.endswith(".so"))
    assert len(others) == 13 and hp.LIB_PATH in others and hp.PCG_LIB_PATH in others, others
    for other in others:
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "hpccg_hip_bicgstab" not in syms, other


def test_abi_version(hp):
    assert hp.bicgstab_lib().hpccg_hip_bicgstab_abi_version() == 1


def test_linked_against_the_main_library_one_directory_up(hp):
    out = subprocess.run(["readelf", "-d", hp.BICGSTAB_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\[\$ORIGIN/\.\.[:\]]", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.bicgstab_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    ll = (C.c_longlong * 1)()
    st = C.c_int(-7)
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first

    def solve(f, h=fake, nrhs=2, b=p, ldb=4, x=p, ldx=4, minv=None, max_iter=10, its=it, nrs=nr):
        return f(h, nrhs, b, ldb, x, ldx, minv, max_iter, 0.0, its, nrs, None)

    for f in (L.hpccg_hip_bicgstab_solve_device, L.hpccg_hip_bicgstab_solve):
        for kw in (dict(h=None), dict(b=None), dict(x=None), dict(its=None), dict(nrs=None)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"NULL" in err() and err().startswith(b"bicgstab:")
        for nrhs in (-1, -3, 0):
            assert solve(f, nrhs=nrhs) == EINVAL
            assert b"nrhs" in err() and err().startswith(b"bicgstab:")
        assert solve(f, max_iter=-1) == EINVAL
        assert b"max_iter" in err() and err().startswith(b"bicgstab:")
        # a leading dimension below every row count (one below this matrix's
        # rows needs the matrix: test_gpu_bicgstab.py)
        for kw in (dict(ldb=-1), dict(ldx=-1)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"leading dimension" in err() and err().startswith(b"bicgstab:")
    assert L.hpccg_hip_bicgstab_release(None) == EINVAL
    assert L.hpccg_hip_bicgstab_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_bicgstab_last_trace(fake, 0, None, 8) == EINVAL
    assert L.hpccg_hip_bicgstab_last_trace(fake, 0, buf, 8) == EINVAL  # (no solve ran on it: the records are searched only)
    assert b"no trace" in err() and err().startswith(b"bicgstab:")
    assert L.hpccg_hip_bicgstab_last_status(None, 0, C.byref(st)) == EINVAL
    assert L.hpccg_hip_bicgstab_last_status(fake, 0, None) == EINVAL
    assert L.hpccg_hip_bicgstab_last_status(fake, 0, C.byref(st)) == EINVAL and st.value == -7
    assert b"no status" in err() and err().startswith(b"bicgstab:")
    assert L.hpccg_hip_bicgstab_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_bicgstab_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_bicgstab_workspace_bytes(fake, ll) == 0 and ll[0] == 0
    assert L.hpccg_hip_bicgstab_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_bicgstab_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.bicgstab_live_workspaces() == 0


def test_a_strided_one_column_is_refused(hp):
    """A 1-D B or X is one column through a view; a strided one would be solved in a copy."""
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_bicgstab(None, np.zeros(8), np.zeros(16)[::2])
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_bicgstab(None, np.zeros(16)[::2], np.zeros(8))


def _twin(n):
    return n.replace("k_pcg_", "k_bicg_").replace("PcgArgs", "BicgArgs")


def test_kernel_budgets(hp):
    ks = _kernels(hp.BICGSTAB_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_bicg_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    spmm = {n: r for n, r in ks.items() if "k_bicg_spmm_" in n}
    # the pcg library's forms: widths 27, 7 and per-slice, one, two and four columns each; the int32-column
    # form likewise; the 27-wide four-column form also compiled for five waves per SIMD. One kernel per form
    # serves the three ends (Ap, v, t) by the launch's phase.
    frags = [f"k_bicg_spmm_a<{w}, {r}, 4>" for w in (27, 7, 0) for r in (1, 2, 4)]
    frags += ["k_bicg_spmm_a<27, 4, 5>"] + [f"k_bicg_spmm_sell<{r}>" for r in (1, 2, 4)]
    for frag in frags:
        assert any(frag in n for n in spmm), frag
    assert len(spmm) == len(frags), sorted(spmm)
    for n, r in spmm.items():
        assert r["vgpr_count"] <= 128, (n, r)
    rest = {n: r for n, r in ks.items() if n not in spmm}
    for frag in ["k_bicg_finalize", "k_bicg_init", "k_bicg_diag", "k_bicg_check"] + \
            [f"k_bicg_{k}<{r}>" for k in ("p", "s", "x") for r in (1, 2, 4)]:
        assert any(frag in n for n in rest), frag
    assert len(rest) == 13, sorted(rest)
    for n, r in rest.items():
        assert r["vgpr_count"] <= 64, (n, r)
    # every SpMM form of the pcg library has its twin here (one source, two wrappers)
    twins = [_twin(n) for n in _kernels(hp.PCG_LIB_PATH) if "k_pcg_spmm_" in n]
    assert len(twins) == len(spmm)
    for twin in twins:
        assert twin in ks, twin


def test_every_a_image_spmm_keeps_its_non_temporal_loads(hp):
    """The two arms of the SpMM bodies' branch on nt differ in the value loads'
    hint alone (csrc/hpccg_spmm.h: arm); every SELL-512-A form here keeps as
    many hinted loads as its twin of the pcg library.

    The counter (test_pcg_cpu's, as it is) wants white space after the hint and
    so misses a load whose operands reach the disassembly's comment column
    (`off offset:-4096 nt//`), which depends on the registers' names. It can
    only count too few, never too many; with that the comparison is "no fewer
    than the twin". Measured: eight forms equal; <0, 4, 4> 5 against 4 and
    <27, 2, 4> 20 against 19, where the pcg twin has one such missed load and
    the true numbers are equal."""
    from test_pcg_cpu import _nt_value_loads
    mine = {n: c for n, c in _nt_value_loads(hp.BICGSTAB_LIB_PATH).items() if "k_bicg_spmm_a<" in n}
    twins = {_twin(n): c for n, c in _nt_value_loads(hp.PCG_LIB_PATH).items() if "k_pcg_spmm_a<" in n}
    assert len(mine) == 10 and sorted(mine) == sorted(twins), (sorted(mine), sorted(twins))
    for n, c in twins.items():
        assert mine[n] >= c >= 1, (n, mine[n], c)


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def same(got, ref, x_scale=None):
    """niters, normr, trace, hist and status equal; x bitwise (got's times x_scale)."""
    assert got[1] == ref[1] and got[5] == ref[5], (got[1], ref[1], got[5], ref[5])
    assert np.float64(got[2]).tobytes() == np.float64(ref[2]).tobytes(), (got[2], ref[2])
    assert got[3].tobytes() == ref[3].tobytes(), "trace"
    assert got[4].tobytes() == ref[4].tobytes(), "hist"
    x = got[0] if x_scale is None else got[0] * x_scale
    assert x.tobytes() == ref[0].tobytes(), ("x", float(np.max(np.abs(x - ref[0]))))


@pytest.mark.parametrize("kind", bc.MKINDS)
@pytest.mark.parametrize("name", [n for n in bc.TABLE if n != "1x1x1"])
def test_the_window_is_not_empty(name, kind):
    """W >= 10, or the history falls under the cutoff inside the window: the
    GPU test cannot shrink its own window to nothing."""
    W, cut, seq, blk = bc.window(name, kind)
    A = bc.csr_of(name)
    m = bc.minv_of(A, kind)
    dx = float(np.max(np.abs(restated_bicg(A, A.b, m, W + 1)[0] - restated_bicg(A, A.b, m, W + 1, dot=bc.blocked_dot)[0])))
    print(f"{name}/{kind}: W {W} cut {cut} niters {seq[1]} status {seq[5]} "
          f"rr/rr0 at W-1 {seq[4][W - 1] / seq[4][0]:.3e} spread in x at W {dx:.3e}")
    assert W >= 10 or cut, (W, cut)
    assert W >= 4, W


@pytest.mark.parametrize("name", ["16c", "12x10x16_7pt", "band600s", "csr513s", "1x40x3"])
def test_a_uniform_power_of_two_m_is_m_one(name):
    A = bc.csr_of(name)
    x0 = 0.25 * ((np.arange(A.nrow) % 7) - 3)
    for b, x in ((A.b, None), (A.b * 2.0 ** -3, x0)):
        for max_iter, tol in ((25, 0.0), (2, 0.0), (60, 1e-6 * float(np.linalg.norm(b)))):
            ref = restated_bicg(A, b, np.ones(A.nrow), max_iter, tol, x0=x)
            assert ref[1] >= 1
            for m in (2.0 ** -3, 2.0 ** 5):
                same(restated_bicg(A, b, np.full(A.nrow, m), max_iter, tol, x0=x), ref)


@pytest.mark.parametrize("name", bc.SCALED)
def test_jacobi_commutes_with_a_power_of_two_column_scaling(name):
    """Jacobi on A S: s_j x'_j is bitwise the x of Jacobi on A, and the history is the same."""
    A0, As = bc.unscaled(name), bc.csr_of(name)
    s = bc.column_scale(A0.nrow)
    rng = np.random.default_rng(3)
    for b in (A0.b, rng.uniform(-1.0, 1.0, A0.nrow)):
        ref = restated_bicg(A0, b, bc.minv_of(A0, "jacobi"), 20)
        got = restated_bicg(As, b, bc.minv_of(As, "jacobi"), 20)
        assert ref[1] == 19 and np.all(np.isfinite(ref[0])) and ref[0].any()
        same(got, ref, x_scale=s)


def test_one_row_is_solved_exactly():
    A = bc.csr_of("1x1x1")
    for kind in bc.MKINDS:
        x, it, nr, tr, hist, status = restated_bicg(A, A.b, bc.minv_of(A, kind), 500)
        assert status == 2 and it >= 1 and hist[it] == 0.0, (status, it, hist)
        assert np.isfinite(x).all() and abs(x[0] - 1.0) <= 4 * np.finfo(float).eps, x


def test_the_two_by_two_breaks_down_at_k_1():
    rp, cols, vals = bc.two_by_two()
    A = oracle.CSR(rp, cols, vals, np.zeros(2), np.zeros(2), np.ones(2))
    x, it, nr, tr, hist, status = restated_bicg(A, np.array([1.0, -1.0]), np.ones(2), 50)
    assert status == 1 and it == 0 and not x.any() and len(tr) == 1 and nr == math.sqrt(2.0)
    # b = (1, 1): iteration 1 runs (alpha 0.5, t.s = 0.0 so omega = 0.0, x = (0.5, 0.5)) and leaves
    # rho_2 = rhat.r = 0.0 exactly: the other breakdown, after an iteration; no NaN anywhere
    x, it, nr, tr, hist, status = restated_bicg(A, np.array([1.0, 1.0]), np.ones(2), 50)
    assert status == 1 and it == 1 and x.tobytes() == np.array([0.5, 0.5]).tobytes() and hist[1] == 0.5
    # b = (3, 1), x = (1, 1): no denominator vanishes, and two iterations solve the two rows
    b = np.array([3.0, 1.0])
    x, it, nr, tr, hist, status = restated_bicg(A, b, np.ones(2), 50)
    assert status in (0, 2) and it >= 2 and np.isfinite(x).all(), (status, it)
    assert np.max(np.abs(oracle.sparsemv(A, x) - b)) <= 1e-14 and np.max(np.abs(x - 1.0)) <= 1e-14, x
    # ... and as a block beside 16c, the block's rows at rest
    B = bc.csr_of("breakdown")
    b = np.zeros(B.nrow)
    b[:2] = (1.0, -1.0)
    for kind in bc.MKINDS:
        x, it, nr, tr, hist, status = restated_bicg(B, b, bc.minv_of(B, kind), 50)
        assert status == 1 and it == 0 and not x.any(), (kind, status, it)


@pytest.mark.parametrize("name", ["16c", "csr513s"])
def test_non_finite_columns_end_by_the_lagged_test(name):
    """A NaN in b: r.r_0 is NaN, the loop test is false at once. An infinite b
    entry: r.r_0 is inf, which iterations 1 and 2 both test; r.r_1 is NaN."""
    A = bc.csr_of(name)
    row = A.nrow // 2
    for kind in bc.MKINDS:
        m = bc.minv_of(A, kind)
        b = A.b.copy()
        b[row] = np.nan
        x, it, nr, tr, hist, status = restated_bicg(A, b, m, 30)
        assert (it, status) == (0, 0) and math.isnan(nr) and not x.any()
        b[row] = np.inf
        x, it, nr, tr, hist, status = restated_bicg(A, b, m, 30)
        assert (it, status) == (2, 0) and math.isnan(nr) and np.isnan(x).all(), (it, status, nr)
        x, it, nr, tr, hist, status = restated_bicg(A, b, m, 2)
        assert (it, status) == (1, 0) and math.isinf(nr)
