"""CPU-only checks of the polynomial-preconditioned CG library
(lib/libhpccg_hip_poly.so, include/hpccg_hip_poly.h): it is built beside the
main library, exports what its header declares, refuses bad arguments before
touching HIP, its kernels keep their budget (read from its gfx950 code
object): no spills, scratch <= 32 B, the SpMM-class kernels <= 128 VGPRs, the
light kernels <= 64; every SELL-512-A step form keeps its non-temporal value
loads; and the host routine of the Chebyshev scalars is the header's
expressions bit for bit.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes
from test_pcg_cpu import _nt_value_loads  # ... and of its disassembly

EINVAL = -1
MAX_DEGREE = 16


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.POLY_LIB_PATH), "run build(): libhpccg_hip_poly.so is missing"
    declared = hp.poly_exported_symbols()
    assert declared == sorted("hpccg_hip_poly_" + s for s in (
        "abi_version", "solve_device", "solve", "bound", "last_spectrum", "last_trace", "release", "workspace_bytes",
        "live_workspaces")), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.POLY_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the nine
    L = hp.poly_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the sixth library only
    assert "hpccg_hip_poly" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    for other in (hp.LIB_PATH, hp.BATCH_LIB_PATH, hp.MIXED_LIB_PATH, hp.PCG_LIB_PATH, hp.PCG_GROUP_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "hpccg_hip_poly" not in syms, other


def test_abi_version(hp):
    assert hp.poly_lib().hpccg_hip_poly_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.POLY_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.poly_lib()
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

    for f in (L.hpccg_hip_poly_solve_device, L.hpccg_hip_poly_solve):
        for kw in (dict(h=None), dict(b=None), dict(x=None), dict(its=None), dict(nrs=None)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"NULL" in err()
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
            assert b"degree" in err()
        nan, inf = float("nan"), float("inf")
        for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (-1.0, 2.0), (0.0, -2.0), (-1.0, 0.0), (nan, 2.0), (0.0, nan),
                           (0.1, inf), (inf, 0.0)):
            for degree in (0, 3):  # (checked whether or not the degree uses them)
                assert solve(f, lmin=lmin, lmax=lmax, degree=degree) == EINVAL, (lmin, lmax)
                assert b"bounds" in err()
    assert L.hpccg_hip_poly_bound(None, None, dd) == EINVAL
    assert L.hpccg_hip_poly_bound(fake, None, None) == EINVAL
    assert L.hpccg_hip_poly_last_spectrum(None, dd, dd) == EINVAL
    assert L.hpccg_hip_poly_last_spectrum(fake, None, dd) == EINVAL
    assert L.hpccg_hip_poly_last_spectrum(fake, dd, None) == EINVAL
    assert L.hpccg_hip_poly_last_spectrum(fake, dd, dd) == EINVAL  # (no solve ran on it: the records are searched only)
    assert b"no spectrum" in err()
    assert L.hpccg_hip_poly_release(None) == EINVAL
    assert L.hpccg_hip_poly_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_poly_last_trace(fake, 0, None, 8) == EINVAL
    assert L.hpccg_hip_poly_last_trace(fake, 0, buf, 8) == EINVAL
    assert b"no trace" in err()
    assert L.hpccg_hip_poly_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_poly_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_poly_workspace_bytes(fake, ll) == 0 and ll[0] == 0
    assert L.hpccg_hip_poly_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_poly_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.poly_live_workspaces() == 0


def test_a_strided_one_column_is_refused(hp):
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_poly(None, np.zeros(8), np.zeros(16)[::2])
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_poly(None, np.zeros(16)[::2], np.zeros(8))


# widths 27, 7 and per-slice; one, two and four columns each; the 27-wide four-column form also compiled
# for five waves per SIMD (the pcg library's plan choices); the int32-column twin likewise
A_FORMS = [(w, r, 4) for w in (27, 7, 0) for r in (1, 2, 4)] + [(27, 4, 5)]


def test_kernel_budgets(hp):
    ks = _kernels(hp.POLY_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_poly_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    heavy = {n: r for n, r in ks.items() if "k_poly_spmm_" in n or "k_poly_step" in n}
    frags = [f"k_poly_{k}<{w}, {r}, {wv}>" for k in ("step", "spmm_a") for w, r, wv in A_FORMS]
    frags += [f"k_poly_{k}<{r}>" for k in ("step_sell", "spmm_sell") for r in (1, 2, 4)]
    for frag in frags:
        assert any(frag in n for n in heavy), frag
    assert len(heavy) == len(frags), sorted(heavy)
    for n, r in heavy.items():
        print(n.split("(")[0], r["vgpr_count"])
        assert r["vgpr_count"] <= 128, (n, r)
    light = {n: r for n, r in ks.items() if n not in heavy}
    for frag in (["k_poly_finalize", "k_poly_init", "k_poly_diag", "k_poly_check", "k_poly_q", "k_poly_bound(",
                  "k_poly_bound_top"] +
                 [f"k_poly_{k}<{r}, {f}>" for k in ("p", "update") for r in (1, 2, 4) for f in ("true", "false")]):
        assert any(frag in n for n in light), frag
    assert len(light) == 7 + 12, sorted(light)
    for n, r in light.items():
        assert r["vgpr_count"] <= 64, (n, r)
    # every SpMM form of the pcg library has its twin and its step here (one source)
    for n in _kernels(hp.PCG_LIB_PATH):
        if "k_pcg_spmm_" in n:
            twin = n.replace("k_pcg_", "k_poly_").replace("PcgArgs", "PolyArgs")
            assert twin in ks, twin
            step = twin.replace("k_poly_spmm_a<", "k_poly_step<").replace("k_poly_spmm_sell<", "k_poly_step_sell<")
            assert step.replace(", bool)", ")") in ks, step


def test_every_a_image_form_keeps_its_non_temporal_loads(hp):
    """csrc/hpccg_spmm.h: arm. The steps run the shared bodies with other ends;
    each SELL-512-A form of the steps and of the SpMM keeps hinted value loads."""
    loads = _nt_value_loads(hp.POLY_LIB_PATH)
    for prefix in ("k_poly_step<", "k_poly_spmm_a<"):
        nt = {n: c for n, c in loads.items() if prefix in n}
        assert len(nt) == len(A_FORMS), sorted(nt)
        for n, c in nt.items():
            assert c >= 1, (n, c)


# ---------------------------------------------------------------------------
# the Chebyshev scalars
# ---------------------------------------------------------------------------
def coefficients(lmin, lmax, d):
    """include/hpccg_hip_poly.h's host expressions in NumPy doubles: c0, a[1..d], b[1..d]."""
    lmin, lmax = np.float64(lmin), np.float64(lmax)
    theta = np.float64(0.5) * (lmax + lmin)
    delta = np.float64(0.5) * (lmax - lmin)
    sigma = theta / delta
    rho = np.float64(1.0) / sigma
    c0 = np.float64(1.0) / theta
    a, b = [], []
    for _ in range(d):
        rho_new = np.float64(1.0) / (np.float64(2.0) * sigma - rho)
        a.append(rho_new * rho)
        b.append(np.float64(2.0) * rho_new / delta)
        rho = rho_new
    return c0, np.array(a, np.float64), np.array(b, np.float64)


def test_host_coefficients_are_the_headers_expressions(hp, tmp_path):
    """csrc/hpccg_poly_coeffs.h (plain C++, what hpccg_poly.hip's host code
    calls) compiled alone behind a C entry point."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "coeffs.cpp"
    src.write_text('#include "hpccg_poly_coeffs.h"\n'
                   'extern "C" int max_degree() { return hpccg::kPolyMaxDegree; }\n'
                   'extern "C" double eig_ratio() { return hpccg::kPolyEigRatio; }\n'
                   'extern "C" void coeffs(double lmin, double lmax, int d, double* c0, double* a, double* b)\n'
                   '{ hpccg::poly_coefficients(lmin, lmax, d, c0, a, b); }\n')
    so = tmp_path / "coeffs.so"
    subprocess.run([cxx, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                    "-I" + os.path.join(hp.HERE, "csrc"), str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.eig_ratio.restype = C.c_double
    L.coeffs.argtypes = [C.c_double, C.c_double, C.c_int] + [C.POINTER(C.c_double)] * 3
    assert L.max_degree() == MAX_DEGREE and L.eig_ratio() == 30.0
    for lmin, lmax in ((53.0 / 27.0 / 30.0, 53.0 / 27.0), (2.0 / 30.0, 2.0), (0.1, 1.0), (1e-3, 7.25), (0.37, 0.38),
                       (3e-7, 2.5e5)):
        for d in range(1, MAX_DEGREE + 1):
            c0 = C.c_double(0.0)
            a = (C.c_double * (MAX_DEGREE + 1))()
            b = (C.c_double * (MAX_DEGREE + 1))()
            L.coeffs(lmin, lmax, d, C.byref(c0), a, b)
            rc0, ra, rb = coefficients(lmin, lmax, d)
            assert np.float64(c0.value).tobytes() == rc0.tobytes(), (lmin, lmax, d)
            assert np.array(a[1:d + 1]).tobytes() == ra.tobytes(), (lmin, lmax, d)
            assert np.array(b[1:d + 1]).tobytes() == rb.tobytes(), (lmin, lmax, d)
            assert a[0] == 0.0 and b[0] == 0.0
            assert np.all(ra > 0.0) and np.all(rb > 0.0)
