"""CPU-only checks of the group polynomial-preconditioned CG library whose
steps stream the members' fp32 images (lib/libhpccg_hip_poly32_group.so,
include/hpccg_hip_poly32_group.h): it is built beside the eight others, exports
exactly what its header declares, refuses bad arguments before touching HIP or
a matrix, and its kernels keep the poly32 library's budget (read from its gfx950
code object): no spills, scratch <= 32 B, the SpMM and step forms <= 128 VGPRs,
the light kernels <= 64; every step and SpMM form of the poly32 library has its
twin here with the same registers, there is no fp64 step kernel, and the kNT
forms keep their non-temporal value loads. The other eight libraries know
nothing of it and keep their kernel lists.
"""
import ctypes as C
import os
import re
import subprocess

from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes
from test_pcg_cpu import _nt_value_loads  # ... and of its disassembly
from test_poly32_cpu import A32_FORMS, A64_FORMS, SELL32_FORMS

EINVAL = -1
MAX_MEMBERS = 16
MAX_DEGREE = 16

NAMES = ("abi_version", "solve_device", "bound", "last_spectrum", "last_trace", "info", "release", "workspace_bytes",
         "live_workspaces")


def _others(hp):
    return (hp.LIB_PATH, hp.BATCH_LIB_PATH, hp.MIXED_LIB_PATH, hp.PCG_LIB_PATH, hp.PCG_GROUP_LIB_PATH,
            hp.POLY_LIB_PATH, hp.POLY_GROUP_LIB_PATH, hp.POLY32_LIB_PATH)


def test_library_exports_every_declared_symbol_and_nothing_else(hp):
    assert os.path.exists(hp.POLY32_GROUP_LIB_PATH), "run build(): libhpccg_hip_poly32_group.so is missing"
    declared = hp.group_poly32_exported_symbols()
    assert declared == sorted("hpccg_hip_group_poly32_" + s for s in NAMES), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.POLY32_GROUP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the nine
    # (the other libraries' prefixes stay their own)
    assert "hpccg_hip_poly32_" not in out and "hpccg_hip_group_poly_" not in out and "group_pcg" not in out
    L = hp.poly32_group_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the ninth library only
    assert "group_poly32" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    for other in _others(hp):
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "group_poly32" not in syms, other


def test_abi_version(hp):
    assert hp.poly32_group_lib().hpccg_hip_group_poly32_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.POLY32_GROUP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.poly32_group_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    dd = (C.c_double * 2)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first
    two = (C.c_void_p * 2)(p, p)  # (as matrices: two fake handles, refused before any is looked at)
    big = (C.c_void_p * (MAX_MEMBERS + 1))(*([p] * (MAX_MEMBERS + 1)))
    ld = (C.c_longlong * 2)(4, 4)

    def solve(Ms=two, nranks=2, nrhs=2, b=two, ldb=ld, x=two, ldx=ld, minv=None, degree=2, lmin=0.0, lmax=0.0,
              max_iter=10, its=it, nrs=nr):
        return L.hpccg_hip_group_poly32_solve_device(Ms, nranks, nrhs, b, ldb, x, ldx, minv, degree, lmin, lmax,
                                                     max_iter, 0.0, its, nrs, None)

    for kw in (dict(Ms=None), dict(b=None), dict(ldb=None), dict(x=None), dict(ldx=None), dict(its=None),
               dict(nrs=None)):
        assert solve(**kw) == EINVAL, kw
        assert b"NULL" in err(), kw
        assert b"group poly32:" in err(), err()
    for nranks in (0, -1, MAX_MEMBERS + 1):
        assert solve(Ms=big, nranks=nranks) == EINVAL, nranks
        assert b"nranks" in err()
    for nrhs in (0, -1, -3):
        assert solve(nrhs=nrhs) == EINVAL
        assert b"nrhs" in err()
    assert solve(max_iter=-1) == EINVAL
    assert b"max_iter" in err()
    # a caller's m for one member only
    for holes in ((None, p), (p, None)):
        assert solve(minv=(C.c_void_p * 2)(*holes)) == EINVAL, holes
        assert b"minv_dev" in err() and b"NULL" in err()
    for r, holes in enumerate(((None, p), (p, None))):
        assert solve(b=(C.c_void_p * 2)(*holes)) == EINVAL
        assert f"B_dev[{r}]".encode() in err()
        assert solve(x=(C.c_void_p * 2)(*holes)) == EINVAL
        assert f"X_dev[{r}]".encode() in err()
    # the degree and the interval: before any matrix is looked at (the handles are fakes)
    for degree in (-1, MAX_DEGREE + 1):
        assert solve(degree=degree) == EINVAL
        assert b"degree" in err()
    nan, inf = float("nan"), float("inf")
    for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (-1.0, 2.0), (0.0, -2.0), (-1.0, 0.0), (nan, 2.0), (0.0, nan),
                       (0.1, inf), (inf, 0.0)):
        for degree in (0, 3):  # (checked whether or not the degree uses them)
            assert solve(lmin=lmin, lmax=lmax, degree=degree) == EINVAL, (lmin, lmax)
            assert b"bounds" in err()
    for r, holes in enumerate(((None, p), (p, None))):
        assert solve(Ms=(C.c_void_p * 2)(*holes)) == EINVAL  # (a NULL handle: found before any is dereferenced)
        assert f"Ms[{r}]".encode() in err()

    assert L.hpccg_hip_group_poly32_bound(None, 2, None, dd) == EINVAL
    assert L.hpccg_hip_group_poly32_bound(two, 0, None, dd) == EINVAL
    assert L.hpccg_hip_group_poly32_bound(two, 2, None, None) == EINVAL
    assert L.hpccg_hip_group_poly32_bound(two, 2, (C.c_void_p * 2)(p, None), dd) == EINVAL
    assert b"minv_dev[1]" in err()
    assert L.hpccg_hip_group_poly32_last_spectrum(None, 2, dd, dd) == EINVAL
    assert L.hpccg_hip_group_poly32_last_spectrum(two, MAX_MEMBERS + 1, dd, dd) == EINVAL
    assert L.hpccg_hip_group_poly32_last_spectrum(two, 2, None, dd) == EINVAL
    assert L.hpccg_hip_group_poly32_last_spectrum(two, 2, dd, None) == EINVAL
    assert L.hpccg_hip_group_poly32_last_trace(None, 2, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_poly32_last_trace(two, MAX_MEMBERS + 1, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_poly32_last_trace(two, 2, 0, None, 8) == EINVAL
    ll = (C.c_longlong * 8)()
    assert L.hpccg_hip_group_poly32_info(None, 2, ll) == EINVAL
    assert b"NULL" in err()
    assert L.hpccg_hip_group_poly32_info(two, 2, None) == EINVAL
    assert b"NULL" in err()
    for nranks in (0, -1, MAX_MEMBERS + 1):
        assert L.hpccg_hip_group_poly32_info(big, nranks, ll) == EINVAL
        assert b"nranks" in err()
    assert L.hpccg_hip_group_poly32_info((C.c_void_p * 2)(p, None), 2, ll) == EINVAL
    assert b"Ms[1]" in err()
    assert L.hpccg_hip_group_poly32_release(None) == EINVAL
    assert L.hpccg_hip_group_poly32_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_group_poly32_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_group_poly32_workspace_bytes(fake, ll) == 0 and ll[0] == 0  # (the records are searched only)
    assert L.hpccg_hip_group_poly32_release(fake) == 0  # (no record: nothing to free)
    assert L.hpccg_hip_group_poly32_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_group_poly32_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.group_poly32_live_workspaces() == 0


def _heavy(n):
    return "k_poly32_group_spmm" in n or "k_poly32_group_step" in n


def test_kernel_list_and_budgets(hp):
    ks = _kernels(hp.POLY32_GROUP_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_poly32_group_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    heavy = {n: r for n, r in ks.items() if _heavy(n)}
    frags = [f"k_poly32_group_{k}<{w}, {r}, {nt}>" for k in ("step", "spmm_a") for w, r, nt in A32_FORMS]
    frags += [f"k_poly32_group_{k}<{r}, {nt}>" for k in ("step_sell", "spmm_sell") for r, nt in SELL32_FORMS]
    frags += [f"k_poly32_group_spmm64_a<{w}, {r}, {wv}>" for w, r, wv in A64_FORMS]
    frags += [f"k_poly32_group_spmm64_sell<{r}>" for r in (1, 2, 4)]
    for frag in frags:
        assert sum(frag in n for n in heavy) == 1, frag
    assert len(heavy) == len(frags), sorted(heavy)
    for n, r in heavy.items():
        print(n.split("(")[0], r["vgpr_count"])
        assert r["vgpr_count"] <= 128, (n, r)
    light = {n: r for n, r in ks.items() if n not in heavy}
    want = ["k_poly32_group_convert", "k_poly32_group_finalize", "k_poly32_group_init", "k_poly32_group_sum",
            "k_poly32_group_halo", "k_poly32_group_diag", "k_poly32_group_check", "k_poly32_group_q",
            "k_poly32_group_bound(", "k_poly32_group_bound_top"]
    want += [f"k_poly32_group_{k}<{r}, {f}>" for k in ("p", "update") for r in (1, 2, 4) for f in ("true", "false")]
    for frag in want:
        assert sum(frag in n for n in light) == 1, (frag, sorted(light))
    assert len(light) == len(want) == 10 + 12, sorted(light)
    for n, r in light.items():
        print(n.split("(")[0], r["vgpr_count"])
        assert r["vgpr_count"] <= 64, (n, r)


def test_every_poly32_form_has_its_twin_and_no_step_is_fp64(hp):
    """One source, two wrappers (csrc/hpccg_spmm32.h, csrc/hpccg_spmm.h): every
    step and SpMM form of the poly32 library stands here with the same
    registers, and so do its p, update and finalize kernels. No step kernel
    streams the fp64 image."""
    ks = _kernels(hp.POLY32_GROUP_LIB_PATH)
    kp = _kernels(hp.POLY32_LIB_PATH)
    twins = 0
    for n, r in kp.items():
        if any(f in n for f in ("k_poly32_step", "k_poly32_spmm", "k_poly32_p<", "k_poly32_update<",
                                "k_poly32_finalize")):
            twin = n.replace("k_poly32_", "k_poly32_group_").replace("Poly32Args", "Poly32GroupArgs")
            assert twin in ks, twin
            assert ks[twin]["vgpr_count"] == r["vgpr_count"], (n, r, ks[twin])
            twins += 1
    assert twins == 2 * (len(A32_FORMS) + len(SELL32_FORMS)) + len(A64_FORMS) + 3 + 12 + 1, twins
    steps = [n for n in ks if "step" in n]
    assert len(steps) == len(A32_FORMS) + len(SELL32_FORMS), steps
    for n in steps:
        assert "step64" not in n, n
        # (the fp32 forms end in kNT; an fp64 form would end in its kWaves)
        assert re.search(r"k_poly32_group_step(_sell)?<(\d+, )+(true|false)>", n), n
        assert not re.search(r"step<\d+, \d+, \d+>", n), n


def test_the_nt_forms_keep_their_non_temporal_loads(hp):
    """The hint is a template parameter of the kernel (csrc/hpccg_spmm32.h): the
    kNT forms of the steps and of the members' exact-image SpMM carry hinted
    16-byte value loads, as many as the poly32 library's twin; the plain forms
    none; the fp64 outer forms keep theirs (csrc/hpccg_spmm.h: arm)."""
    loads = _nt_value_loads(hp.POLY32_GROUP_LIB_PATH)
    ref = _nt_value_loads(hp.POLY32_LIB_PATH)
    for prefix in ("k_poly32_group_step<", "k_poly32_group_spmm_a<"):
        nt = {n: c for n, c in loads.items() if prefix in n}
        assert len(nt) == len(A32_FORMS), sorted(nt)
        for n, c in nt.items():
            if "true>" in n:
                assert c >= 1, (n, c)
            else:
                assert c == 0, (n, c)
    for prefix in ("k_poly32_group_step_sell<", "k_poly32_group_spmm_sell<"):
        nt = {n: c for n, c in loads.items() if prefix in n}
        assert len(nt) == len(SELL32_FORMS), sorted(nt)
        for n, c in nt.items():
            assert (c >= 1) == ("true>" in n), (n, c)
    nt = {n: c for n, c in loads.items() if "k_poly32_group_spmm64_a<" in n}
    assert len(nt) == len(A64_FORMS), sorted(nt)
    for n, c in nt.items():
        assert c >= 1, (n, c)
    compared = 0
    for n, c in ref.items():
        if "k_poly32_step" in n or "k_poly32_spmm" in n:
            twin = n.replace("k_poly32_", "k_poly32_group_").replace("Poly32Args", "Poly32GroupArgs")
            assert loads[twin] == c, (n, c, loads[twin])
            compared += 1
    assert compared == 2 * (len(A32_FORMS) + len(SELL32_FORMS)) + len(A64_FORMS) + 3, compared


def test_the_other_eight_libraries_keep_their_kernel_lists(hp):
    """The poly group unit's host code moved to csrc/hpccg_poly_group_host.h;
    no device code changed: the code objects hold the kernels they held."""
    assert len(_kernels(hp.LIB_PATH)) == 77
    kb = sorted(_kernels(hp.BATCH_LIB_PATH))
    assert len(kb) == 16 and all("k_batch_" in n for n in kb), kb
    km = sorted(_kernels(hp.MIXED_LIB_PATH))
    assert len(km) == 33 and all("k_mixed_" in n for n in km), km
    kp = sorted(_kernels(hp.PCG_LIB_PATH))
    assert len(kp) == 23 and all("k_pcg_" in n and "k_pcg_group_" not in n for n in kp), kp
    kg = sorted(_kernels(hp.PCG_GROUP_LIB_PATH))
    assert len(kg) == 25 and all("k_pcg_group_" in n for n in kg), kg
    ko = sorted(_kernels(hp.POLY_LIB_PATH))
    assert len(ko) == 45 and all("k_poly_" in n and "k_poly_group_" not in n for n in ko), ko
    kq = sorted(_kernels(hp.POLY_GROUP_LIB_PATH))
    assert len(kq) == 47 and all("k_poly_group_" in n for n in kq), kq
    k32 = sorted(_kernels(hp.POLY32_LIB_PATH))
    assert len(k32) == 81 and all("k_poly32_" in n and "k_poly32_group_" not in n for n in k32), k32
