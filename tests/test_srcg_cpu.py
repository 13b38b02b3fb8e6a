"""CPU-only checks of the single-reduction CG library
(lib/libhpccg_hip_srcg.so, include/hpccg_hip_srcg.h): it is built beside the
main library, exports what its header declares, refuses bad arguments before
touching HIP, and its kernels keep their budget (read from its gfx950 code
object): no spills, scratch <= 32 B, the SpMM kernels <= 128 VGPRs, the others
<= 64. No other library knows of it.

The NumPy restatement the GPU tests hold the solver to
(test_gpu_srcg.restated_sr) is pinned here against the classic one
(test_gpu_pcg.restated): the first iteration bitwise, the r.r history within a
tenth of the GPU tolerance, the degenerate columns' outcomes.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import columns_cases as cc
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes
from test_gpu_mixed import columns
from test_gpu_pcg import P10, csr_diagonal, restated
from test_gpu_srcg import restated_sr

EINVAL = -1


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.SRCG_LIB_PATH), "run build(): libhpccg_hip_srcg.so is missing"
    declared = hp.srcg_exported_symbols()
    assert declared == sorted("hpccg_hip_srcg_" + s for s in (
        "abi_version", "solve_device", "solve", "last_trace", "release", "workspace_bytes", "live_workspaces")), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.SRCG_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the seven
    L = hp.srcg_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the tenth library only
    assert "hpccg_hip_srcg" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    others = (hp.LIB_PATH, hp.BATCH_LIB_PATH, hp.MIXED_LIB_PATH, hp.PCG_LIB_PATH, hp.PCG_GROUP_LIB_PATH,
              hp.POLY_LIB_PATH, hp.POLY_GROUP_LIB_PATH, hp.POLY32_LIB_PATH, hp.POLY32_GROUP_LIB_PATH)
    assert len(set(others)) == 9
    for other in others:
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "hpccg_hip_srcg" not in syms, other


def test_abi_version(hp):
    assert hp.srcg_lib().hpccg_hip_srcg_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.SRCG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.srcg_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    ll = (C.c_longlong * 1)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first

    def solve(f, h=fake, nrhs=2, b=p, ldb=4, x=p, ldx=4, minv=None, max_iter=10, its=it, nrs=nr):
        return f(h, nrhs, b, ldb, x, ldx, minv, max_iter, 0.0, its, nrs, None)

    for f in (L.hpccg_hip_srcg_solve_device, L.hpccg_hip_srcg_solve):
        for kw in (dict(h=None), dict(b=None), dict(x=None), dict(its=None), dict(nrs=None)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"NULL" in err() and err().startswith(b"srcg:")
        for nrhs in (-1, -3, 0):
            assert solve(f, nrhs=nrhs) == EINVAL
            assert b"nrhs" in err() and err().startswith(b"srcg:")
        assert solve(f, max_iter=-1) == EINVAL
        assert b"max_iter" in err()
        # a leading dimension below every row count (one below this matrix's
        # rows needs the matrix: test_gpu_srcg.py)
        for kw in (dict(ldb=-1), dict(ldx=-1)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"leading dimension" in err()
    assert L.hpccg_hip_srcg_release(None) == EINVAL
    assert L.hpccg_hip_srcg_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_srcg_last_trace(fake, 0, None, 8) == EINVAL
    assert L.hpccg_hip_srcg_last_trace(fake, 0, buf, 8) == EINVAL  # (no solve ran on it: the records are searched only)
    assert b"no trace" in err()
    assert L.hpccg_hip_srcg_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_srcg_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_srcg_workspace_bytes(fake, ll) == 0 and ll[0] == 0
    assert L.hpccg_hip_srcg_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_srcg_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.srcg_live_workspaces() == 0


def test_a_strided_one_column_is_refused(hp):
    """A 1-D B or X is one column through a view; a strided one would be solved in a copy."""
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_srcg(None, np.zeros(8), np.zeros(16)[::2])
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_srcg(None, np.zeros(16)[::2], np.zeros(8))


def test_kernel_budgets(hp):
    ks = _kernels(hp.SRCG_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_srcg_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    spmm = {n: r for n, r in ks.items() if "k_srcg_spmm_" in n}
    # the pcg library's forms: widths 27, 7 and per-slice, one, two and four columns each; the int32-column
    # form likewise; the 27-wide four-column form also compiled for five waves per SIMD
    frags = [f"k_srcg_spmm_a<{w}, {r}, 4>" for w in (27, 7, 0) for r in (1, 2, 4)]
    frags += ["k_srcg_spmm_a<27, 4, 5>"] + [f"k_srcg_spmm_sell<{r}>" for r in (1, 2, 4)]
    for frag in frags:
        assert any(frag in n for n in spmm), frag
    assert len(spmm) == len(frags), sorted(spmm)
    for n, r in spmm.items():
        assert r["vgpr_count"] <= 128, (n, r)
    rest = {n: r for n, r in ks.items() if n not in spmm}
    for frag in ["k_srcg_finalize", "k_srcg_init", "k_srcg_diag", "k_srcg_check"] + \
            [f"k_srcg_{k}<{r}>" for k in ("step", "t") for r in (1, 2, 4)]:
        assert any(frag in n for n in rest), frag
    assert len(rest) == 10, sorted(rest)
    for n, r in rest.items():
        assert r["vgpr_count"] <= 64, (n, r)
    # every SpMM form of the pcg library has its twin here (one source, two wrappers)
    for n in _kernels(hp.PCG_LIB_PATH):
        if "k_pcg_spmm_" in n:
            twin = n.replace("k_pcg_", "k_srcg_").replace("PcgArgs", "SrcgArgs")
            assert twin in ks, twin


def test_every_a_image_spmm_keeps_its_non_temporal_loads(hp):
    """The two arms of the SpMM bodies' branch on nt differ in the value loads'
    hint alone (csrc/hpccg_spmm.h: arm); every SELL-512-A form here keeps as
    many hinted loads as its twin of the pcg library."""
    from test_pcg_cpu import _nt_value_loads
    mine = {n: c for n, c in _nt_value_loads(hp.SRCG_LIB_PATH).items() if "k_srcg_spmm_a<" in n}
    twins = {n.replace("k_pcg_", "k_srcg_").replace("PcgArgs", "SrcgArgs"): c
             for n, c in _nt_value_loads(hp.PCG_LIB_PATH).items() if "k_pcg_spmm_a<" in n}
    assert len(mine) == 10, sorted(mine)
    assert mine == twins, (mine, twins)
    assert min(mine.values()) >= 1, mine


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
FIRST =["16c", "12x10x16_7pt", "band600", "dyadic_csr513", "p10_33c", "p2_dyadic_csr3000"]

_csrs = {}


def csr(name):
    """cc.csr_of, with the p10 scaling of test_gpu_pcg beside its p2."""
    if name not in _csrs:
        if name.startswith("p10_"):
            from test_gpu_pcg import base_csr, scale_of, scaled
            A0 = base_csr(name[4:])
            _csrs[name] = scaled(A0, scale_of("p10", A0.nrow))
        else:
            _csrs[name] = cc.csr_of(name)
    return _csrs[name]


def same(got, ref):
    assert got[1] == ref[1], (got[1], ref[1])
    assert np.float64(got[2]).tobytes() == np.float64(ref[2]).tobytes(), (got[2], ref[2])
    assert got[3].tobytes() == ref[3].tobytes(), "trace"
    assert got[0].tobytes() == ref[0].tobytes(), ("x", float(np.max(np.abs(got[0] - ref[0]))))


@pytest.mark.parametrize("shape", FIRST)
def test_the_restatements_first_iteration_is_the_classic_one(shape):
    A = csr(shape)
    B, X0 = columns(A.b, A.xexact, 4)
    for minv in (1.0 / csr_diagonal(A), np.ones(A.nrow)):
        for c in (0, 1, 3):
            for max_iter in (1, 2):
                same(restated_sr(A, B[c], minv, max_iter, x0=X0[c]), restated(A, B[c], minv, max_iter, x0=X0[c]))
            got, ref = restated_sr(A, B[c], minv, 3, x0=X0[c]), restated(A, B[c], minv, 3, x0=X0[c])
            assert got[1] == ref[1] == 2 and got[3].tobytes() == ref[3].tobytes()


@pytest.mark.parametrize("shape", P10)
def test_the_restatement_follows_the_classic_one(shape):
    """The r.r history within RTRANS_RTOL_1GPU / 10 of the classic
    restatement's, and of its own under another dot order (numpy's blocked
    sum), over at least 10 points: the GPU tolerance has room for both."""
    A = csr(shape)
    minv = 1.0 / csr_diagonal(A)
    sr = restated_sr(A, A.b, minv, 200)
    classic = restated(A, A.b, minv, 200)
    blocked = restated_sr(A, A.b, minv, 200, dot=lambda x, y: np.float64(np.dot(x, y)))
    n1 = check_trace(sr[3], classic[3], RTRANS_RTOL_1GPU / 10)
    n2 = check_trace(blocked[3], sr[3], RTRANS_RTOL_1GPU / 10)
    print(f"{shape}: {n1} points against the classic restatement, {n2} against the other dot order")
    assert n1 >= 10 and n2 >= 10, (n1, n2)


@pytest.mark.parametrize("shape", cc.CPU_SHAPES)
def test_degenerate_columns_end_as_the_classic_ones(shape):
    A = cc.csr_of(shape)
    for name, b, x0, mi, tol in cc.shape_cases(shape, A):
        for tag, minv in (("jacobi", 1.0 / csr_diagonal(A)), ("half", np.full(A.nrow, 0.5))):
            try:
                got = restated_sr(A, b, minv, mi, tol, x0=x0)
                cc.degenerate(*got, x0)
                _, it, nr, _ = cc.expect_pcg(A, b, x0, mi, tol, minv)
                assert got[1] == it, (got[1], it)
                assert math.isnan(got[2]) == math.isnan(nr) and (got[2] == 0.0) == (nr == 0.0), (got[2], nr)
            except AssertionError as e:
                raise AssertionError(f"{shape}/{name}/{tag}: {e}") from None


def test_the_restatement_forms_p_and_s_at_k_1_as_the_kernel_does():
    """k == 1: p = u + 0.0*u and s = w + 0.0*w (the kernel's one expression
    with u read for p and beta 0.0), not copies: an infinite entry of u gives
    NaN there, and a finite one its own bits."""
    A = csr("12x10x16_7pt")
    minv = 1.0 / csr_diagonal(A)
    steps = []
    restated_sr(A, A.b, minv, 3, steps=steps)
    (k1, p1, s1), (k2, p2, s2) = steps
    assert (k1, k2) == (1, 2)
    u = minv * A.b
    assert p1.tobytes() == (u + 0.0 * u).tobytes() and not np.array_equal(p2, p1)
    row = A.nrow // 2
    b = A.b.copy()
    b[row] = np.inf
    steps = []
    restated_sr(A, b, minv, 2, steps=steps)
    _, p, s = steps[0]
    assert np.isnan(p[row]) and np.isfinite(np.delete(p, row)).all()  # u + 0.0*u, where u alone is inf
    assert np.isnan(s[row]) and np.isnan(s).sum() > 1  # w + 0.0*w: w is +-inf at the row and its neighbours
