"""CPU-only checks of the single-reduction polynomial CG library
(lib/libhpccg_hip_srpoly.so, include/hpccg_hip_srpoly.h): it is built beside
the main library, exports what its header declares, refuses bad arguments
before touching HIP, and its kernels keep their budget (read from its gfx950
code object): the kernel list is pinned, no spills, no scratch, every SpMM and
step form has the registers and the non-temporal loads of its twin in the poly
library, the light kernels <= 64 VGPRs. No other library and no other header
knows of it.

The NumPy restatement the GPU tests hold the solver to
(test_gpu_srpoly.restated_srpoly) is pinned here: its first iteration is
bitwise the classic polynomial restatement's (test_gpu_poly.restated), degree 0
is bitwise test_gpu_srcg.restated_sr, later iterations follow the classic
restatement within a tenth of the GPU tolerance, and degenerate columns end as
the classic ones.
"""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

import columns_cases as cc
import oracle
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes
from test_gpu_mixed import columns
from test_gpu_pcg import csr_diagonal
from test_gpu_poly import DEGREES, EIG_RATIO, P10, lap_csr, numpy_bound, restated
from test_gpu_srcg import restated_sr
from test_gpu_srpoly import restated_srpoly
from test_pcg_cpu import _nt_value_loads  # ... and of its disassembly
from test_poly_cpu import A_FORMS
from test_srcg_cpu import csr as srcg_csr, same

EINVAL = -1
MAX_DEGREE = 16
NAMES = ("abi_version", "solve_device", "solve", "bound", "last_spectrum", "last_trace", "release", "workspace_bytes",
         "live_workspaces")


def others(hp, mine):
    libs = sorted(glob.glob(os.path.join(hp.HERE, "lib", "libhpccg_hip*.so")))
    assert mine in libs and len(libs) == 13, libs
    return [p for p in libs if p != mine]


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.SRPOLY_LIB_PATH), "run build(): libhpccg_hip_srpoly.so is missing"
    declared = hp.srpoly_exported_symbols()
    assert declared == sorted("hpccg_hip_srpoly_" + s for s in NAMES), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.SRPOLY_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the nine
    L = hp.srpoly_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the twelfth library and its header only
    for other in others(hp, hp.SRPOLY_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "hpccg_hip_srpoly_" not in syms, other
    for header in glob.glob(os.path.join(hp.ROOT, "include", "*.h*")):
        if os.path.basename(header) not in ("hpccg_hip_srpoly.h", "hpccg_hip_srpoly_group.h"):
            assert "srpoly" not in open(header).read(), header
    # (the group header names this library's solve in its bitwise statements, and declares none of it)
    assert not re.findall(r"\bhpccg_hip_srpoly_\w+\s*\(",
                          open(os.path.join(hp.ROOT, "include", "hpccg_hip_srpoly_group.h")).read())


def test_abi_version(hp):
    assert hp.srpoly_lib().hpccg_hip_srpoly_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.SRPOLY_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.srpoly_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    ll = (C.c_longlong * 1)()
    dd = (C.c_double * 2)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first

    def solve(f, h=fake, nrhs=2, b=p, ldb=4, x=p, ldx=4, minv=None, degree=2, lmin=0.0, lmax=0.0, max_iter=10, its=it,
              nrs=nr):
        return f(h, nrhs, b, ldb, x, ldx, minv, degree, lmin, lmax, max_iter, 0.0, its, nrs, None)

    for f in (L.hpccg_hip_srpoly_solve_device, L.hpccg_hip_srpoly_solve):
        for kw in (dict(h=None), dict(b=None), dict(x=None), dict(its=None), dict(nrs=None)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"NULL" in err() and err().startswith(b"srpoly:")
        for nrhs in (-1, -3, 0):
            assert solve(f, nrhs=nrhs) == EINVAL
            assert b"nrhs" in err()
        assert solve(f, max_iter=-1) == EINVAL
        assert b"max_iter" in err()
        for kw in (dict(ldb=-1), dict(ldx=-1)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"leading dimension" in err()
        for degree in (-1, MAX_DEGREE + 1):
            assert solve(f, degree=degree) == EINVAL
            assert b"degree" in err() and err().startswith(b"srpoly:")
        nan, inf = float("nan"), float("inf")
        for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (-1.0, 2.0), (0.0, -2.0), (-1.0, 0.0), (nan, 2.0), (0.0, nan),
                           (0.1, inf), (inf, 0.0)):
            for degree in (0, 3):  # (checked whether or not the degree uses them)
                assert solve(f, lmin=lmin, lmax=lmax, degree=degree) == EINVAL, (lmin, lmax)
                assert b"bounds" in err()
    assert L.hpccg_hip_srpoly_bound(None, None, dd) == EINVAL
    assert L.hpccg_hip_srpoly_bound(fake, None, None) == EINVAL
    assert L.hpccg_hip_srpoly_last_spectrum(None, dd, dd) == EINVAL
    assert L.hpccg_hip_srpoly_last_spectrum(fake, None, dd) == EINVAL
    assert L.hpccg_hip_srpoly_last_spectrum(fake, dd, None) == EINVAL
    assert L.hpccg_hip_srpoly_last_spectrum(fake, dd, dd) == EINVAL  # (no solve ran on it: the records are searched only)
    assert b"no spectrum" in err()
    assert L.hpccg_hip_srpoly_release(None) == EINVAL
    assert L.hpccg_hip_srpoly_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_srpoly_last_trace(fake, 0, None, 8) == EINVAL
    assert L.hpccg_hip_srpoly_last_trace(fake, 0, buf, 8) == EINVAL
    assert b"no trace" in err()
    assert L.hpccg_hip_srpoly_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_srpoly_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_srpoly_workspace_bytes(fake, ll) == 0 and ll[0] == 0
    assert L.hpccg_hip_srpoly_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_srpoly_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.srpoly_live_workspaces() == 0


def test_a_strided_one_column_is_refused(hp):
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_srpoly(None, np.zeros(8), np.zeros(16)[::2])
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_srpoly(None, np.zeros(16)[::2], np.zeros(8))


def check_kernels(ks, prefix, twins, twin_prefix, light_names):
    """The pinned kernel list of a srpoly code object ks and its budget. twins:
    the poly (group) library's kernels; cheb is its step, spmm_* its spmm_*."""
    assert ks
    for n, r in ks.items():
        assert prefix in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] == 0, (n, r)
    heavy = {n: r for n, r in ks.items() if prefix + "spmm_" in n or prefix + "cheb" in n}
    frags = [f"{prefix}{k}<{w}, {r}, {wv}>(" for k in ("cheb", "spmm_a") for w, r, wv in A_FORMS]
    frags += [f"{prefix}{k}<{r}>(" for k in ("cheb_sell", "spmm_sell") for r in (1, 2, 4)]
    for frag in frags:
        assert sum(frag in n for n in heavy) == 1, frag
    assert len(heavy) == len(frags) == 26, sorted(heavy)
    light = {n: r for n, r in ks.items() if n not in heavy}
    want = [prefix + k + "(" for k in light_names]
    want += [f"{prefix}step<{r}, {f}>(" for r in (1, 2, 4) for f in ("true", "false")]
    want += [f"{prefix}t<{r}>(" for r in (1, 2, 4)]
    for frag in want:
        assert sum(frag in n for n in light) == 1, (frag, sorted(light))
    assert len(light) == len(want), sorted(light)
    for n, r in light.items():
        print(n.split("(")[0], r["vgpr_count"])
        assert r["vgpr_count"] <= 64, (n, r)
    # every SpMM and step form of the twin library is here with the same registers (one source, two wrappers)
    seen = 0
    for n, r in twins.items():
        if twin_prefix + "step" in n or twin_prefix + "spmm_" in n:
            mine = n.replace(twin_prefix + "step_sell<", prefix + "cheb_sell<").replace(
                twin_prefix + "step<", prefix + "cheb<").replace(twin_prefix + "spmm_", prefix + "spmm_").replace(
                "PolyArgs", "SrpolyArgs")
            assert mine in ks, mine
            print(mine.split("(")[0], ks[mine]["vgpr_count"])
            assert ks[mine]["vgpr_count"] == r["vgpr_count"] <= 128, (n, r, ks[mine])
            seen += 1
    assert seen == 26, seen


def check_nt_loads(path, prefix, twin_path, twin_prefix):
    """csrc/hpccg_spmm.h: arm. Every SELL-512-A form of the steps and of the
    SpMM keeps as many hinted value loads as its twin."""
    loads = _nt_value_loads(path)
    mine = {n.split("(")[0]: c for n, c in loads.items() if prefix + "cheb<" in n or prefix + "spmm_a<" in n}
    ref = {n.split("(")[0].replace(twin_prefix + "step<", prefix + "cheb<").replace(twin_prefix, prefix): c
           for n, c in _nt_value_loads(twin_path).items() if twin_prefix + "step<" in n or twin_prefix + "spmm_a<" in n}
    assert len(mine) == 2 * len(A_FORMS), sorted(mine)
    assert mine == ref, (mine, ref)
    assert min(mine.values()) >= 1, mine


def test_kernel_list_and_budgets(hp):
    check_kernels(_kernels(hp.SRPOLY_LIB_PATH), "k_srpoly_", _kernels(hp.POLY_LIB_PATH), "k_poly_",
                  ["finalize", "init", "diag", "check", "q", "bound", "bound_top"])


def test_every_a_image_form_keeps_its_non_temporal_loads(hp):
    check_nt_loads(hp.SRPOLY_LIB_PATH, "k_srpoly_", hp.POLY_LIB_PATH, "k_poly_")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
FIRST = ["16c", "12x10x16_7pt", "band600", "dyadic_csr513", "p10_33c", "p2_dyadic_csr3000", "p10_lap_16c"]

_csrs = {}


def csr(name):
    """test_srcg_cpu.csr, with test_gpu_poly's lap forms beside it."""
    if name not in _csrs:
        kind, _, rest = name.partition("_")
        if rest.startswith("lap_"):
            from test_gpu_pcg import scale_of, scaled
            A0 = lap_csr(rest)
            _csrs[name] = scaled(A0, scale_of(kind, A0.nrow))
        else:
            _csrs[name] = srcg_csr(name)
    return _csrs[name]


def interval(A, minv):
    lmax, _ = numpy_bound(A, minv)
    return lmax / EIG_RATIO, lmax


@pytest.mark.parametrize("shape", FIRST)
def test_the_restatements_first_iteration_is_the_classic_one(shape):
    A = csr(shape)
    B, X0 = columns(A.b, A.xexact, 4)
    for minv in (1.0 / csr_diagonal(A), np.ones(A.nrow)):
        lmin, lmax = interval(A, minv)
        for d in (0,) + tuple(DEGREES):
            for c in (0, 1, 3):
                for max_iter in (1, 2):
                    same(restated_srpoly(A, B[c], minv, d, lmin, lmax, max_iter, x0=X0[c]),
                         restated(A, B[c], minv, d, lmin, lmax, max_iter, x0=X0[c]))
                got = restated_srpoly(A, B[c], minv, d, lmin, lmax, 3, x0=X0[c])
                ref = restated(A, B[c], minv, d, lmin, lmax, 3, x0=X0[c])
                assert got[1] == ref[1] == 2 and got[3].tobytes() == ref[3].tobytes(), (d, c)


@pytest.mark.parametrize("shape", FIRST[:4])
def test_degree_0_of_the_restatement_is_the_srcg_one(shape):
    A = csr(shape)
    minv = 1.0 / csr_diagonal(A)
    same(restated_srpoly(A, A.b, minv, 0, 0.0, 0.0, 40), restated_sr(A, A.b, minv, 40))


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("shape", P10)
def test_the_restatement_follows_the_classic_one(shape, degree):
    """The r.r history within RTRANS_RTOL_1GPU / 10 of the classic
    restatement's, and of its own under another dot order (numpy's blocked
    sum), over at least 10 points; the iteration counts at 1e-10 r0 and at
    1e-14 r0 are the classic form's."""
    A = csr(shape)
    minv = 1.0 / csr_diagonal(A)
    lmin, lmax = interval(A, minv)
    sr = restated_srpoly(A, A.b, minv, degree, lmin, lmax, 200)
    classic = restated(A, A.b, minv, degree, lmin, lmax, 200)
    blocked = restated_srpoly(A, A.b, minv, degree, lmin, lmax, 200, dot=lambda x, y: np.float64(np.dot(x, y)))
    n1 = check_trace(sr[3], classic[3], RTRANS_RTOL_1GPU / 10)
    n2 = check_trace(blocked[3], sr[3], RTRANS_RTOL_1GPU / 10)
    print(f"{shape} degree {degree}: {n1} points against the classic restatement, {n2} against the other dot order")
    assert n1 >= 10 and n2 >= 10, (n1, n2)
    r0 = float(np.sqrt(oracle.ddot(A.b, A.b)))
    for rel in (1e-10, 1e-14):
        # (niters under a tolerance: the first k with trace[k] <= tol, as the loop test stops)
        its = [int(np.argmax(t[3] <= rel * r0)) for t in (sr, classic)]
        assert its[0] == its[1] > 0, (rel, its)
    x = restated_srpoly(A, A.b, minv, degree, lmin, lmax, 200, 1e-14 * r0)[0]
    assert float(np.max(np.abs(x - A.xexact))) <= 1e-10


@pytest.mark.parametrize("shape", cc.CPU_SHAPES)
def test_degenerate_columns_end_as_the_classic_ones(shape):
    A = cc.csr_of(shape)
    jac = 1.0 / csr_diagonal(A)
    lmin, lmax = interval(A, jac)
    for name, b, x0, mi, tol in cc.shape_cases(shape, A):
        for tag, minv in (("jacobi", jac), ("half", np.full(A.nrow, 0.5))):
            try:
                got = restated_srpoly(A, b, minv, 0, 0.0, 0.0, mi, tol, x0=x0)
                cc.degenerate(*got, x0)
                _, it, nr, _ = cc.expect_pcg(A, b, x0, mi, tol, minv)
                assert got[1] == it, (got[1], it)
                assert math.isnan(got[2]) == math.isnan(nr) and (got[2] == 0.0) == (nr == 0.0), (got[2], nr)
                got = restated_srpoly(A, b, minv, 2, lmin, lmax, mi, tol, x0=x0)
                _, it, nr, _ = restated(A, b, minv, 2, lmin, lmax, mi, tol, x0=x0)
                assert got[1] == it, (got[1], it)
                assert math.isnan(got[2]) == math.isnan(nr) and (got[2] == 0.0) == (nr == 0.0), (got[2], nr)
            except AssertionError as e:
                raise AssertionError(f"{shape}/{name}/{tag}: {e}") from None
