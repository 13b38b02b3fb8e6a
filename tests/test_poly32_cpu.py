"""CPU-only checks of the polynomial-preconditioned CG library whose steps
stream an fp32 matrix image (lib/libhpccg_hip_poly32.so,
include/hpccg_hip_poly32.h): it is built beside the main library, exports what
its header declares and nothing else, refuses bad arguments before touching
HIP, its kernels keep their budget (read from its gfx950 code object): no
spills, no scratch, the SpMM-class kernels <= 128 VGPRs, the light
kernels <= 64; every step form stands beside its outer-SpMM twin; every
SELL-512-A step form keeps its non-temporal value loads; and the seven older
libraries export what they exported.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes
from test_pcg_cpu import _nt_value_loads  # ... and of its disassembly

EINVAL = -1
MAX_DEGREE = 16

NAMES = ("abi_version", "solve_device", "solve", "bound", "last_spectrum", "last_trace", "info", "release",
         "workspace_bytes", "live_workspaces")


def test_library_exports_every_declared_symbol_and_nothing_else(hp):
    assert os.path.exists(hp.POLY32_LIB_PATH), "run build(): libhpccg_hip_poly32.so is missing"
    declared = hp.poly32_exported_symbols()
    assert declared == sorted("hpccg_hip_poly32_" + s for s in NAMES), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.POLY32_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the ten
    L = hp.poly32_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the eighth library only
    assert "hpccg_hip_poly32" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    for other in (hp.LIB_PATH, hp.BATCH_LIB_PATH, hp.MIXED_LIB_PATH, hp.PCG_LIB_PATH, hp.PCG_GROUP_LIB_PATH,
                  hp.POLY_LIB_PATH, hp.POLY_GROUP_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "hpccg_hip_poly32" not in syms, other


def test_abi_version(hp):
    assert hp.poly32_lib().hpccg_hip_poly32_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.POLY32_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.poly32_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    ll = (C.c_longlong * 4)()
    dd = (C.c_double * 2)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first

    def solve(f, h=fake, nrhs=2, b=p, ldb=4, x=p, ldx=4, minv=None, degree=2, lmin=0.0, lmax=0.0, max_iter=10, its=it,
              nrs=nr):
        return f(h, nrhs, b, ldb, x, ldx, minv, degree, lmin, lmax, max_iter, 0.0, its, nrs, None)

    for f in (L.hpccg_hip_poly32_solve_device, L.hpccg_hip_poly32_solve):
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
        assert b"poly32:" in err()
    assert L.hpccg_hip_poly32_bound(None, None, dd) == EINVAL
    assert L.hpccg_hip_poly32_bound(fake, None, None) == EINVAL
    assert L.hpccg_hip_poly32_last_spectrum(None, dd, dd) == EINVAL
    assert L.hpccg_hip_poly32_last_spectrum(fake, None, dd) == EINVAL
    assert L.hpccg_hip_poly32_last_spectrum(fake, dd, None) == EINVAL
    assert L.hpccg_hip_poly32_last_spectrum(fake, dd, dd) == EINVAL  # (no solve ran on it: the records are searched only)
    assert b"no spectrum" in err()
    assert L.hpccg_hip_poly32_info(None, ll) == EINVAL
    assert L.hpccg_hip_poly32_info(fake, None) == EINVAL
    assert L.hpccg_hip_poly32_release(None) == EINVAL
    assert L.hpccg_hip_poly32_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_poly32_last_trace(fake, 0, None, 8) == EINVAL
    assert L.hpccg_hip_poly32_last_trace(fake, 0, buf, 8) == EINVAL
    assert b"no trace" in err()
    assert L.hpccg_hip_poly32_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_poly32_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_poly32_workspace_bytes(fake, ll) == 0 and ll[0] == 0
    assert L.hpccg_hip_poly32_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_poly32_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.poly32_live_workspaces() == 0


def test_a_strided_one_column_is_refused(hp):
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_poly32(None, np.zeros(8), np.zeros(16)[::2])
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_poly32(None, np.zeros(16)[::2], np.zeros(8))


# the fp32 forms: widths 27, 7 and per-slice; one, two and four columns each; each with plain and with
# non-temporal value loads (a template parameter: chosen on the host); the int32-column forms likewise
A32_FORMS = [(w, r, nt) for w in (27, 7, 0) for r in (1, 2, 4) for nt in ("false", "true")]
SELL32_FORMS = [(r, nt) for r in (1, 2, 4) for nt in ("false", "true")]
# the fp64 outer forms of an inexact image: the poly library's
A64_FORMS = [(w, r, 4) for w in (27, 7, 0) for r in (1, 2, 4)] + [(27, 4, 5)]


def test_kernel_list_and_budgets(hp):
    ks = _kernels(hp.POLY32_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_poly32_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] == 0, (n, r)  # no scratch
    heavy = {n: r for n, r in ks.items() if "k_poly32_spmm" in n or "k_poly32_step" in n}
    frags = [f"k_poly32_{k}<{w}, {r}, {nt}>" for k in ("step", "spmm_a") for w, r, nt in A32_FORMS]
    frags += [f"k_poly32_{k}<{r}, {nt}>" for k in ("step_sell", "spmm_sell") for r, nt in SELL32_FORMS]
    frags += [f"k_poly32_spmm64_a<{w}, {r}, {wv}>" for w, r, wv in A64_FORMS]
    frags += [f"k_poly32_spmm64_sell<{r}>" for r in (1, 2, 4)]
    for frag in frags:
        assert any(frag in n for n in heavy), frag
    assert len(heavy) == len(frags), sorted(heavy)
    for n, r in heavy.items():
        print(n.split("(")[0], r["vgpr_count"])
        assert r["vgpr_count"] <= 128, (n, r)
    light = {n: r for n, r in ks.items() if n not in heavy}
    for frag in (["k_poly32_convert", "k_poly32_finalize", "k_poly32_init", "k_poly32_diag", "k_poly32_check",
                  "k_poly32_q", "k_poly32_bound(", "k_poly32_bound_top"] +
                 [f"k_poly32_{k}<{r}, {f}>" for k in ("p", "update") for r in (1, 2, 4) for f in ("true", "false")]):
        assert any(frag in n for n in light), frag
    assert len(light) == 8 + 12, sorted(light)
    for n, r in light.items():
        assert r["vgpr_count"] <= 64, (n, r)
    # each step form beside its outer-SpMM twin (one source: csrc/hpccg_spmm32.h)
    for n in ks:
        if "k_poly32_step" in n:
            twin = n.replace("k_poly32_step_sell<", "k_poly32_spmm_sell<").replace("k_poly32_step<",
                                                                                  "k_poly32_spmm_a<")
            assert twin.replace("Poly32Args)", "Poly32Args, bool)") in ks, twin
    # the fp64 outer forms are the poly library's SpMM forms
    for n in _kernels(hp.POLY_LIB_PATH):
        if "k_poly_spmm_" in n:
            twin = n.replace("k_poly_spmm_", "k_poly32_spmm64_").replace("PolyArgs", "Poly32Args")
            assert twin in ks, twin


def test_every_a_image_step_form_keeps_its_non_temporal_loads(hp):
    """The hint is a template parameter of the kernel (csrc/hpccg_spmm32.h): the
    kNT forms of the steps and of the outer SpMM carry hinted 16-byte value
    loads, the plain forms none; the fp64 outer forms keep theirs
    (csrc/hpccg_spmm.h: arm)."""
    loads = _nt_value_loads(hp.POLY32_LIB_PATH)
    for prefix in ("k_poly32_step<", "k_poly32_spmm_a<"):
        nt = {n: c for n, c in loads.items() if prefix in n}
        assert len(nt) == len(A32_FORMS), sorted(nt)
        for n, c in nt.items():
            if "true>" in n:
                assert c >= 1, (n, c)
            else:
                assert c == 0, (n, c)
    for prefix in ("k_poly32_step_sell<", "k_poly32_spmm_sell<"):
        nt = {n: c for n, c in loads.items() if prefix in n}
        assert len(nt) == len(SELL32_FORMS), sorted(nt)
        for n, c in nt.items():
            assert (c >= 1) == ("true>" in n), (n, c)
    nt = {n: c for n, c in loads.items() if "k_poly32_spmm64_a<" in n}
    assert len(nt) == len(A64_FORMS), sorted(nt)
    for n, c in nt.items():
        assert c >= 1, (n, c)


def test_the_older_libraries_export_what_they_exported(hp):
    """The seven older libraries' symbol lists, through the package's helpers
    (each reads its header) and nm on the library."""
    libs = ((hp.BATCH_LIB_PATH, hp.batch_exported_symbols() + hp.group_batch_exported_symbols(), 8 + 4),
            (hp.MIXED_LIB_PATH, hp.mixed_exported_symbols(), 10),
            (hp.PCG_LIB_PATH, hp.pcg_exported_symbols(), 8),
            (hp.PCG_GROUP_LIB_PATH, hp.group_pcg_exported_symbols(), 7),
            (hp.POLY_LIB_PATH, hp.poly_exported_symbols(), 9),
            (hp.POLY_GROUP_LIB_PATH, hp.group_poly_exported_symbols(), 8))
    for path, declared, count in libs:
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
        assert exported == sorted(declared), path
        assert len(exported) == count, (path, exported)
    main = subprocess.run(["nm", "-D", "--defined-only", hp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    declared = hp.exported_symbols()
    assert len(declared) == 53, len(declared)
    for s in declared:
        assert f" T {s}" in main, s
    assert "poly32" not in main
