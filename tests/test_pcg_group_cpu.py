"""CPU-only checks of the group preconditioned-CG library
(lib/libhpccg_hip_pcg_group.so, include/hpccg_hip_pcg_group.h): it is built
beside the four others, exports exactly what its header declares, refuses bad
arguments before touching HIP, and its kernels keep the pcg library's budget
(read from its gfx950 code object): no spills, scratch <= 32 B, the SpMM
kernels <= 128 VGPRs, the light kernels <= 64. The other libraries know nothing
of it, and the batch and mixed libraries, which share hpccg_columns.h with it,
keep their kernel lists.
"""
import ctypes as C
import os
import re
import subprocess

from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes

EINVAL = -1
MAX_MEMBERS = 16

NAMES = ("abi_version", "solve_device", "diagonal", "last_trace", "release", "workspace_bytes", "live_workspaces")


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.PCG_GROUP_LIB_PATH), "run build(): libhpccg_hip_pcg_group.so is missing"
    declared = hp.group_pcg_exported_symbols()
    assert declared == sorted("hpccg_hip_group_pcg_" + s for s in NAMES), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.PCG_GROUP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the seven
    assert "hpccg_hip_pcg" not in out  # (the pcg library's prefix stays its own)
    L = hp.pcg_group_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the fifth library only
    header = open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    assert "group_pcg" not in header and "hpccg_hip_pcg" not in header
    for other in (hp.LIB_PATH, hp.BATCH_LIB_PATH, hp.MIXED_LIB_PATH, hp.PCG_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "group_pcg" not in syms, other


def test_abi_version(hp):
    assert hp.pcg_group_lib().hpccg_hip_group_pcg_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.PCG_GROUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.pcg_group_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first
    two = (C.c_void_p * 2)(p, p)
    big = (C.c_void_p * (MAX_MEMBERS + 1))(*([p] * (MAX_MEMBERS + 1)))
    ld = (C.c_longlong * 2)(4, 4)

    def solve(Ms=two, nranks=2, nrhs=2, b=two, ldb=ld, x=two, ldx=ld, minv=None, max_iter=10, its=it, nrs=nr):
        return L.hpccg_hip_group_pcg_solve_device(Ms, nranks, nrhs, b, ldb, x, ldx, minv, max_iter, 0.0, its, nrs,
                                                  None)

    for kw in (dict(Ms=None), dict(b=None), dict(ldb=None), dict(x=None), dict(ldx=None), dict(its=None),
               dict(nrs=None)):
        assert solve(**kw) == EINVAL, kw
        assert b"NULL" in err(), kw
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
    assert solve(Ms=(C.c_void_p * 2)(None, None)) == EINVAL  # (a NULL handle: nothing is dereferenced)
    assert b"Ms[0]" in err()

    assert L.hpccg_hip_group_pcg_diagonal(None, 2, two) == EINVAL
    assert L.hpccg_hip_group_pcg_diagonal(two, 0, two) == EINVAL
    assert L.hpccg_hip_group_pcg_diagonal(two, 2, None) == EINVAL
    assert L.hpccg_hip_group_pcg_diagonal(two, 2, (C.c_void_p * 2)(p, None)) == EINVAL
    assert L.hpccg_hip_group_pcg_last_trace(None, 2, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_pcg_last_trace(two, MAX_MEMBERS + 1, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_pcg_last_trace(two, 2, 0, None, 8) == EINVAL
    assert L.hpccg_hip_group_pcg_release(None) == EINVAL
    ll = (C.c_longlong * 1)()
    assert L.hpccg_hip_group_pcg_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_group_pcg_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_group_pcg_workspace_bytes(fake, ll) == 0 and ll[0] == 0  # (the records are searched only)
    assert L.hpccg_hip_group_pcg_release(fake) == 0  # (no record: nothing to free)
    assert L.hpccg_hip_group_pcg_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_group_pcg_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.group_pcg_live_workspaces() == 0


def test_kernel_budgets(hp):
    ks = _kernels(hp.PCG_GROUP_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_pcg_group_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    spmm = {n: r for n, r in ks.items() if "k_pcg_group_spmm_" in n}
    # the pcg library's forms: widths 27, 7 and per-slice; one, two and four columns each; the int32-column
    # form likewise; the 27-wide four-column form also compiled for five waves per SIMD
    frags = [f"k_pcg_group_spmm_a<{w}, {r}, 4>" for w in (27, 7, 0) for r in (1, 2, 4)]
    frags += ["k_pcg_group_spmm_a<27, 4, 5>"] + [f"k_pcg_group_spmm_sell<{r}>" for r in (1, 2, 4)]
    for frag in frags:
        assert any(frag in n for n in spmm), frag
    assert len(spmm) == len(frags), sorted(spmm)
    for n, r in spmm.items():
        assert r["vgpr_count"] <= 128, (n, r)
    light = {n: r for n, r in ks.items() if n not in spmm}
    want = ["k_pcg_group_init", "k_pcg_group_finalize", "k_pcg_group_sum", "k_pcg_group_halo", "k_pcg_group_diag",
            "k_pcg_group_check"] + [f"k_pcg_group_{k}<{r}>" for k in ("p", "update") for r in (1, 2, 4)]
    for frag in want:
        assert any(frag in n for n in light), frag
    assert len(light) == len(want), sorted(light)
    for n, r in light.items():
        assert r["vgpr_count"] <= 64, (n, r)
    # every kernel of the pcg library's recurrence has its twin here with the same registers (one source, two
    # wrappers); its finalize stays within the light budget with the r.z total's store
    kp = _kernels(hp.PCG_LIB_PATH)
    for n, r in kp.items():
        if any(f in n for f in ("k_pcg_spmm_", "k_pcg_p<", "k_pcg_update<", "k_pcg_finalize")):
            twin = n.replace("k_pcg_", "k_pcg_group_")
            assert twin in ks, twin
            assert ks[twin]["vgpr_count"] == r["vgpr_count"], (n, r, ks[twin])
    assert kp["k_pcg_finalize(PcgArgs, int, int)"]["vgpr_count"] <= 64


def test_the_shared_engine_left_the_batch_and_mixed_kernel_lists_alone(hp):
    """hpccg_columns.h changed inside col_finalize's preconditioned arm only, which neither library
    instantiates: their code objects hold the kernels they held."""
    kb = sorted(_kernels(hp.BATCH_LIB_PATH))
    want = ["k_batch_init(", "k_batch_finalize(", "k_batch_group_sum("]
    want += [f"k_batch_{k}<{r}>(" for k in ("p", "update", "spmm_sell") for r in (2, 4)]
    want += [f"k_batch_spmm_a<{w}, {r}, 4>(" for w in (27, 7, 0) for r in (2, 4)] + ["k_batch_spmm_a<27, 4, 5>("]
    for frag in want:
        assert sum(frag in n for n in kb) == 1, (frag, kb)
    assert len(kb) == len(want) == 16, kb
    km = sorted(_kernels(hp.MIXED_LIB_PATH))
    assert len(km) == 33 and all("k_mixed_" in n for n in km), km
    for frag in ("k_mixed_finalize", "k_mixed_p<", "k_mixed_update<", "k_mixed_spmm"):
        assert any(frag in n for n in km), (frag, km)
