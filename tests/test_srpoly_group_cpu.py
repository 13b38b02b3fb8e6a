"""CPU-only checks of the group single-reduction polynomial CG library
(lib/libhpccg_hip_srpoly_group.so, include/hpccg_hip_srpoly_group.h): it is
built beside the others, exports exactly what its header declares, refuses bad
arguments before touching HIP or a matrix, and its kernels keep their budget
(read from its gfx950 code object): the kernel list is pinned, no spills, no
scratch, every SpMM and step form has the registers and the non-temporal loads
of its twin in the group poly library, and the fused step those of the one-rank
library's. The other libraries know nothing of it.
"""
import ctypes as C
import os
import re
import subprocess

from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes
from test_srpoly_cpu import check_kernels, check_nt_loads, others

EINVAL = -1
MAX_MEMBERS = 16
MAX_DEGREE = 16

NAMES = ("abi_version", "solve_device", "bound", "last_spectrum", "last_trace", "release", "workspace_bytes",
         "live_workspaces")


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.SRPOLY_GROUP_LIB_PATH), "run build(): libhpccg_hip_srpoly_group.so is missing"
    declared = hp.group_srpoly_exported_symbols()
    assert declared == sorted("hpccg_hip_group_srpoly_" + s for s in NAMES), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.SRPOLY_GROUP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the eight
    # (the other libraries' prefixes stay their own)
    assert "hpccg_hip_srpoly_" not in out and "group_poly_" not in out and "group_srcg" not in out
    L = hp.srpoly_group_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the thirteenth library only
    for other in others(hp, hp.SRPOLY_GROUP_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "group_srpoly" not in syms, other
    for header in os.listdir(os.path.join(hp.ROOT, "include")):
        if header != "hpccg_hip_srpoly_group.h":
            assert "group_srpoly" not in open(os.path.join(hp.ROOT, "include", header)).read(), header


def test_abi_version(hp):
    assert hp.srpoly_group_lib().hpccg_hip_group_srpoly_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.SRPOLY_GROUP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.srpoly_group_lib()
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
        return L.hpccg_hip_group_srpoly_solve_device(Ms, nranks, nrhs, b, ldb, x, ldx, minv, degree, lmin, lmax,
                                                     max_iter, 0.0, its, nrs, None)

    for kw in (dict(Ms=None), dict(b=None), dict(ldb=None), dict(x=None), dict(ldx=None), dict(its=None),
               dict(nrs=None)):
        assert solve(**kw) == EINVAL, kw
        assert b"NULL" in err() and err().startswith(b"group srpoly:"), kw
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
        assert b"degree" in err() and err().startswith(b"group srpoly:")
    nan, inf = float("nan"), float("inf")
    for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (-1.0, 2.0), (0.0, -2.0), (-1.0, 0.0), (nan, 2.0), (0.0, nan),
                       (0.1, inf), (inf, 0.0)):
        for degree in (0, 3):  # (checked whether or not the degree uses them)
            assert solve(lmin=lmin, lmax=lmax, degree=degree) == EINVAL, (lmin, lmax)
            assert b"bounds" in err()
    for r, holes in enumerate(((None, p), (p, None))):
        assert solve(Ms=(C.c_void_p * 2)(*holes)) == EINVAL  # (a NULL handle: found before any is dereferenced)
        assert f"Ms[{r}]".encode() in err()

    assert L.hpccg_hip_group_srpoly_bound(None, 2, None, dd) == EINVAL
    assert L.hpccg_hip_group_srpoly_bound(two, 0, None, dd) == EINVAL
    assert L.hpccg_hip_group_srpoly_bound(two, 2, None, None) == EINVAL
    assert L.hpccg_hip_group_srpoly_bound(two, 2, (C.c_void_p * 2)(p, None), dd) == EINVAL
    assert b"minv_dev[1]" in err()
    assert L.hpccg_hip_group_srpoly_last_spectrum(None, 2, dd, dd) == EINVAL
    assert L.hpccg_hip_group_srpoly_last_spectrum(two, MAX_MEMBERS + 1, dd, dd) == EINVAL
    assert L.hpccg_hip_group_srpoly_last_spectrum(two, 2, None, dd) == EINVAL
    assert L.hpccg_hip_group_srpoly_last_spectrum(two, 2, dd, None) == EINVAL
    assert L.hpccg_hip_group_srpoly_last_trace(None, 2, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_srpoly_last_trace(two, MAX_MEMBERS + 1, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_srpoly_last_trace(two, 2, 0, None, 8) == EINVAL
    assert L.hpccg_hip_group_srpoly_release(None) == EINVAL
    ll = (C.c_longlong * 1)()
    assert L.hpccg_hip_group_srpoly_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_group_srpoly_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_group_srpoly_workspace_bytes(fake, ll) == 0 and ll[0] == 0  # (the records are searched only)
    assert L.hpccg_hip_group_srpoly_release(fake) == 0  # (no record: nothing to free)
    assert L.hpccg_hip_group_srpoly_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_group_srpoly_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.group_srpoly_live_workspaces() == 0


def test_kernel_list_and_budgets(hp):
    ks = _kernels(hp.SRPOLY_GROUP_LIB_PATH)
    check_kernels(ks, "k_srpoly_group_", _kernels(hp.POLY_GROUP_LIB_PATH), "k_poly_group_",
                  ["finalize", "init", "sum", "halo", "diag", "check", "q", "bound", "bound_top"])
    # the fused step, the t kernel and the finalize are the one-rank library's (one source, two wrappers)
    seen = 0
    for n, r in _kernels(hp.SRPOLY_LIB_PATH).items():
        if any(f in n for f in ("k_srpoly_step<", "k_srpoly_t<", "k_srpoly_finalize")):
            twin = n.replace("k_srpoly_", "k_srpoly_group_")
            assert ks[twin]["vgpr_count"] == r["vgpr_count"], (n, r, ks[twin])
            seen += 1
    assert seen == 10, seen


def test_every_a_image_form_keeps_its_non_temporal_loads(hp):
    check_nt_loads(hp.SRPOLY_GROUP_LIB_PATH, "k_srpoly_group_", hp.POLY_GROUP_LIB_PATH, "k_poly_group_")
