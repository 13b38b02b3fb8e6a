"""hpccg_sycl_amd -- Python mirror of the reference HPCCG interface over the
MI355X C ABI (include/hpccg_hip.h, lib/libhpccg_hip.so).

Names and argument meaning follow the reference (Dart120/HPCCG-SYCL):

* ``generate_matrix(nx, ny, nz, rank=0, size=1, use_7pt=False)`` ->
  generate_matrix.cpp:196 (host HPC_Sparse_Matrix, global columns)
* ``Matrix.from_hpc(problem)`` / ``Matrix.from_csr(...)`` / ``Matrix.generate(...)``
  -> the device-resident matrix HPCCG() reads (HPC_Sparse_Matrix.hpp:54-85)
* ``HPCCG(M, b, x, max_iter, tolerance)`` -> HPCCG.cpp:312-402, returns
  ``(ierr, niters, normr, times)`` and updates ``x`` in place
* ``HPC_sparsemv(M, x, y)``, ``ddot(n, x, y)``, ``waxpby(n, alpha, x, beta, y, w)``
  -> HPC_sparsemv.cpp:68, ddot.cpp:60, waxpby.cpp:69 on device buffers

There is no CPU fallback: if the HIP library is missing or no GPU is present,
calls raise (``HPCCGError``). The package directory name contains a hyphen,
so import it by path (``load()`` below, or importlib).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip.so")
CLI_PATH = os.path.join(HERE, "bin", "test_HPCCG")
ROOT = os.path.dirname(HERE)

_lib = None


class HPCCGError(RuntimeError):
    pass


def build(jobs: int = 8) -> None:
    """Compile the gfx950 library and CLI in-tree (hipcc cross-compiles)."""
    subprocess.run(["make", "-s", "-C", HERE, f"-j{jobs}"], check=True)


# hpccg_hip_allgather_fn (include/hpccg_hip.h): send, recv, bytes per rank, ctx
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p)
_host_allgather = None  # the live callback of comm_init_host (ctypes must keep it)


class _HPCMatrix(C.Structure):
    """HPC_Sparse_Matrix (HPC_Sparse_Matrix.hpp:54-85, non-MPI layout)."""
    _fields_ = [
        ("title", C.c_char_p), ("start_row", C.c_int), ("stop_row", C.c_int),
        ("total_nrow", C.c_int), ("total_nnz", C.c_longlong), ("local_nrow", C.c_int),
        ("local_ncol", C.c_int), ("local_nnz", C.c_int), ("nnz_in_row", C.POINTER(C.c_int)),
        ("ptr_to_vals_in_row", C.POINTER(C.POINTER(C.c_double))),
        ("ptr_to_inds_in_row", C.POINTER(C.POINTER(C.c_int))),
        ("ptr_to_diags", C.POINTER(C.POINTER(C.c_double))),
        ("list_of_vals", C.POINTER(C.c_double)), ("list_of_inds", C.POINTER(C.c_int)),
    ]


def lib() -> C.CDLL:
    """Load libhpccg_hip.so (import torch first so one HIP runtime is shared)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("HPCCG_HIP_LIB", LIB_PATH)  # diagnostics: A/B against another build
    if not os.path.exists(path):
        raise HPCCGError(f"{path} missing: run build() (the HIP path has no CPU fallback)")
    try:  # share torch's HIP runtime when torch is around (same sonames)
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(path)  # RTLD_LOCAL: never interpose HPCCG() into other libraries
    vp, ip, dp, lp = C.c_void_p, C.c_int, C.c_double, C.c_longlong
    PI, PD = C.POINTER(C.c_int), C.POINTER(C.c_double)
    sig = {
        "hpccg_hip_abi_version": (ip, []),
        "hpccg_hip_last_error": (C.c_char_p, []),
        "hpccg_hip_device_count": (ip, [PI]),
        "hpccg_hip_set_device": (ip, [ip]),
        "hpccg_hip_comm_unique_id": (ip, [C.c_char_p]),
        "hpccg_hip_comm_init": (ip, [C.c_char_p, ip, ip]),
        "hpccg_hip_comm_init_host": (ip, [ip, ip, ALLGATHER_FN, vp]),
        "hpccg_hip_comm_mode": (ip, [PI]),
        "hpccg_hip_diag_canary_check": (ip, [PI, C.c_char_p, ip]),
        "hpccg_hip_comm_destroy": (ip, []),
        "hpccg_hip_comm_size": (ip, [PI, PI]),
        "hpccg_hip_comm_allreduce_host": (ip, [PD, ip, ip]),
        "hpccg_hip_transport_verdict": (ip, [PI, PI]),
        "hpccg_hip_device_name": (ip, [C.c_char_p, ip, PI]),
        "hpccg_hip_runtime_info": (ip, [PI, C.c_char_p, ip, C.c_char_p, C.c_char_p, ip]),
        "hpccg_generate_matrix": (ip, [ip, ip, ip, ip, ip, ip, C.POINTER(C.POINTER(_HPCMatrix)),
                                       C.POINTER(PD), C.POINTER(PD), C.POINTER(PD)]),
        "hpccg_free_problem": (None, [C.POINTER(_HPCMatrix), PD, PD, PD]),
        "hpccg_hip_matrix_create": (ip, [C.POINTER(_HPCMatrix), C.POINTER(vp)]),
        "hpccg_hip_matrix_create_csr": (ip, [ip, ip, ip, vp, vp, vp, C.POINTER(vp)]),
        "hpccg_hip_matrix_generate": (ip, [ip, ip, ip, ip, C.POINTER(vp)]),
        "hpccg_hip_matrix_destroy": (ip, [vp]),
        "hpccg_hip_matrix_info": (ip, [vp, C.POINTER(lp)]),
        "hpccg_hip_matrix_vectors": (ip, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "hpccg_hip_solve": (ip, [vp, vp, vp, ip, dp, PI, PD, PD, ip]),
        "hpccg_hip_solve_device": (ip, [vp, vp, vp, ip, dp, PI, PD, PD, ip]),
        "hpccg_hip_last_trace": (ip, [vp, PD, ip]),
        "hpccg_hip_set_option": (ip, [vp, C.c_char_p, lp]),
        "hpccg_hip_get_option": (ip, [vp, C.c_char_p, C.POINTER(lp)]),
        "hpccg_hip_kernel_times": (ip, [vp, PD]),
        "hpccg_hip_kernel_times_iter": (ip, [vp, PD, ip]),
        "hpccg_hip_diag_spmv": (ip, [vp, ip, ip, PD]),
        "hpccg_hip_diag_slot_plan": (ip, [ip, ip, ip, ip, PI, ip, PI]),
        "hpccg_hip_diag_timeline": (ip, [vp, C.POINTER(C.c_uint64), ip]),
        "hpccg_hip_diag_realloc": (ip, [vp, ip, C.POINTER(C.c_uint64)]),
        "hpccg_hip_probe_placement": (ip, [vp, ip]),
        "hpccg_hip_diag_placement": (ip, [vp, PD, ip]),
        "hpccg_hip_set_placement_probe": (ip, [ip]),
        "hpccg_hip_sparsemv": (ip, [vp, vp, vp]),
        "hpccg_hip_ddot": (ip, [ip, vp, vp, PD]),
        "hpccg_hip_waxpby": (ip, [ip, dp, vp, dp, vp, vp]),
        "hpccg_hip_HPCCG": (ip, [C.POINTER(_HPCMatrix), vp, vp, ip, dp, PI, PD, PD]),
        "hpccg_hip_dropin_release": (ip, [C.POINTER(_HPCMatrix)]),
        "hpccg_hip_dropin_cached": (ip, [C.POINTER(_HPCMatrix)]),
        "hpccg_hip_set_keep_sell": (ip, [ip]),
        "hpccg_sell_build": (lp, [ip, lp, lp, vp, vp, vp, vp, vp, vp]),
        "hpccg_halo_plan": (ip, [ip, ip, ip, vp, vp, PI]),
        "hpccg_slab_plan": (ip, [ip, ip, PI, PI]),
        "hpccg_hip_group_generate": (ip, [ip, ip, ip, ip, ip, PI, C.POINTER(vp)]),
        "hpccg_hip_set_halo_mode": (ip, [ip]),
        "hpccg_gather_plan": (ip, [ip, PI, ip, ip, vp, vp, ip, PI, PI, PI, PI, PI, PI]),
        "hpccg_read_HPC_row": (ip, [C.c_char_p, ip, ip, C.POINTER(C.POINTER(_HPCMatrix)),
                                    C.POINTER(PD), C.POINTER(PD), C.POINTER(PD)]),
        "hpccg_hip_group_create_csr": (ip, [ip, PI, PI, PI, ip, C.POINTER(vp), C.POINTER(vp),
                                            C.POINTER(vp), C.POINTER(vp)]),
        "hpccg_hip_group_solve": (ip, [C.POINTER(vp), ip, C.POINTER(vp), C.POINTER(vp), ip, dp, PI,
                                       PD, PD]),
    }
    for name, (res, args) in sig.items():
        if path != LIB_PATH and not hasattr(L, name):
            continue  # an older build under A/B (HPCCG_HIP_LIB): bind what it has
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


_vp, _ip, _dp, _lp = C.c_void_p, C.c_int, C.c_double, C.c_longlong
_PI, _PD, _PV, _PL = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)
_units = {}  # slot -> the library of that unit, once loaded


def _load_unit(slot: str, path: str, what: str, no_fallback: str, sig: dict) -> C.CDLL:
    """The library of one unit, loaded on first use with its signatures bound.
    It is linked against libhpccg_hip.so beside it, so lib() is loaded first
    and both share one copy of the main library. what, no_fallback: "the pcg
    library", "the preconditioned solve has no fallback" of its messages."""
    L = _units.get(slot)
    if L is not None:
        return L
    if os.environ.get("HPCCG_HIP_LIB", LIB_PATH) != LIB_PATH:
        raise HPCCGError(f"{what} runs on the in-tree libhpccg_hip.so only (HPCCG_HIP_LIB is set)")
    lib()
    if not os.path.exists(path):
        raise HPCCGError(f"{path} missing: run build() ({no_fallback})")
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise HPCCGError(f"{path} does not load: {e}") from e
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _units[slot] = L
    return L


BATCH_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_batch.so")


def batch_lib() -> C.CDLL:
    """Load libhpccg_hip_batch.so (include/hpccg_hip_batch.h) on first use. It
    is linked against libhpccg_hip.so beside it, so lib() is loaded first and
    both share one copy of the main library."""
    return _load_unit("batch", BATCH_LIB_PATH, "the batch library", "the batched solve has no fallback", {
        "hpccg_hip_batch_abi_version": (_ip, []),
        "hpccg_hip_batch_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_batch_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_batch_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_batch_sparsemv": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp]),
        "hpccg_hip_batch_release": (_ip, [_vp]),
        "hpccg_hip_batch_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_batch_live_workspaces": (_ip, [_PI]),
        # include/hpccg_hip_batch_group.h
        "hpccg_hip_group_batch_abi_version": (_ip, []),
        "hpccg_hip_group_batch_solve_device": (_ip, [_PV, _ip, _ip, _PV, _PL, _PV, _PL, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_group_batch_sparsemv": (_ip, [_PV, _ip, _ip, _PV, _PL, _PV, _PL]),
        "hpccg_hip_group_batch_last_trace": (_ip, [_PV, _ip, _ip, _PD, _ip]),
    })


MIXED_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_mixed.so")


def mixed_lib() -> C.CDLL:
    """Load libhpccg_hip_mixed.so (include/hpccg_hip_mixed.h) on first use. It
    is linked against libhpccg_hip.so beside it, so lib() is loaded first and
    both share one copy of the main library."""
    return _load_unit("mixed", MIXED_LIB_PATH, "the mixed library", "the mixed solve has no fallback", {
        "hpccg_hip_mixed_abi_version": (_ip, []),
        "hpccg_hip_mixed_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _ip, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_mixed_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _ip, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_mixed_sparsemv": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp]),
        "hpccg_hip_mixed_info": (_ip, [_vp, _PL]),
        "hpccg_hip_mixed_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_mixed_last_sweeps": (_ip, [_vp, _ip, _PI, _PD, _ip]),
        "hpccg_hip_mixed_release": (_ip, [_vp]),
        "hpccg_hip_mixed_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_mixed_live_workspaces": (_ip, [_PI]),
    })


PCG_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_pcg.so")


def pcg_lib() -> C.CDLL:
    """Load libhpccg_hip_pcg.so (include/hpccg_hip_pcg.h) on first use. It is
    linked against libhpccg_hip.so beside it, so lib() is loaded first and both
    share one copy of the main library."""
    return _load_unit("pcg", PCG_LIB_PATH, "the pcg library", "the preconditioned solve has no fallback", {
        "hpccg_hip_pcg_abi_version": (_ip, []),
        "hpccg_hip_pcg_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_pcg_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_pcg_diagonal": (_ip, [_vp, _vp]),
        "hpccg_hip_pcg_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_pcg_release": (_ip, [_vp]),
        "hpccg_hip_pcg_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_pcg_live_workspaces": (_ip, [_PI]),
    })


SRCG_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_srcg.so")


def srcg_lib() -> C.CDLL:
    """Load libhpccg_hip_srcg.so (include/hpccg_hip_srcg.h) on first use. It is
    linked against libhpccg_hip.so beside it, so lib() is loaded first and both
    share one copy of the main library."""
    return _load_unit("srcg", SRCG_LIB_PATH, "the srcg library", "the single-reduction solve has no fallback", {
        "hpccg_hip_srcg_abi_version": (_ip, []),
        "hpccg_hip_srcg_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_srcg_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_srcg_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_srcg_release": (_ip, [_vp]),
        "hpccg_hip_srcg_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_srcg_live_workspaces": (_ip, [_PI]),
    })


BICGSTAB_LIB_PATH = os.path.join(HERE, "lib", "bicgstab", "libhpccg_hip_bicgstab.so")


def bicgstab_lib() -> C.CDLL:
    """Load lib/bicgstab/libhpccg_hip_bicgstab.so (include/hpccg_hip_bicgstab.h)
    on first use. It is linked against libhpccg_hip.so one directory up, so
    lib() is loaded first and both share one copy of the main library."""
    return _load_unit("bicgstab", BICGSTAB_LIB_PATH, "the bicgstab library", "the BiCGStab solve has no fallback", {
        "hpccg_hip_bicgstab_abi_version": (_ip, []),
        "hpccg_hip_bicgstab_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_bicgstab_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_bicgstab_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_bicgstab_last_status": (_ip, [_vp, _ip, _PI]),
        "hpccg_hip_bicgstab_release": (_ip, [_vp]),
        "hpccg_hip_bicgstab_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_bicgstab_live_workspaces": (_ip, [_PI]),
    })


PCG_GROUP_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_pcg_group.so")


def pcg_group_lib() -> C.CDLL:
    """Load libhpccg_hip_pcg_group.so (include/hpccg_hip_pcg_group.h) on first
    use. It is linked against libhpccg_hip.so beside it, so lib() is loaded
    first and both share one copy of the main library."""
    return _load_unit("pcg_group", PCG_GROUP_LIB_PATH, "the group pcg library", "the group preconditioned solve has no fallback", {
        "hpccg_hip_group_pcg_abi_version": (_ip, []),
        "hpccg_hip_group_pcg_solve_device": (_ip, [_PV, _ip, _ip, _PV, _PL, _PV, _PL, _PV, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_group_pcg_diagonal": (_ip, [_PV, _ip, _PV]),
        "hpccg_hip_group_pcg_last_trace": (_ip, [_PV, _ip, _ip, _PD, _ip]),
        "hpccg_hip_group_pcg_release": (_ip, [_vp]),
        "hpccg_hip_group_pcg_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_group_pcg_live_workspaces": (_ip, [_PI]),
    })


SRCG_GROUP_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_srcg_group.so")


def srcg_group_lib() -> C.CDLL:
    """Load libhpccg_hip_srcg_group.so (include/hpccg_hip_srcg_group.h) on first
    use. It is linked against libhpccg_hip.so beside it, so lib() is loaded
    first and both share one copy of the main library."""
    return _load_unit("srcg_group", SRCG_GROUP_LIB_PATH, "the group srcg library", "the group single-reduction solve has no fallback", {
        "hpccg_hip_group_srcg_abi_version": (_ip, []),
        "hpccg_hip_group_srcg_solve_device": (_ip, [_PV, _ip, _ip, _PV, _PL, _PV, _PL, _PV, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_group_srcg_last_trace": (_ip, [_PV, _ip, _ip, _PD, _ip]),
        "hpccg_hip_group_srcg_release": (_ip, [_vp]),
        "hpccg_hip_group_srcg_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_group_srcg_live_workspaces": (_ip, [_PI]),
    })


SRPOLY_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_srpoly.so")


def srpoly_lib() -> C.CDLL:
    """Load libhpccg_hip_srpoly.so (include/hpccg_hip_srpoly.h) on first use. It
    is linked against libhpccg_hip.so beside it, so lib() is loaded first and
    both share one copy of the main library."""
    return _load_unit("srpoly", SRPOLY_LIB_PATH, "the srpoly library", "the single-reduction polynomial solve has no fallback", {
        "hpccg_hip_srpoly_abi_version": (_ip, []),
        "hpccg_hip_srpoly_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_srpoly_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_srpoly_bound": (_ip, [_vp, _vp, _PD]),
        "hpccg_hip_srpoly_last_spectrum": (_ip, [_vp, _PD, _PD]),
        "hpccg_hip_srpoly_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_srpoly_release": (_ip, [_vp]),
        "hpccg_hip_srpoly_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_srpoly_live_workspaces": (_ip, [_PI]),
    })


SRPOLY_GROUP_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_srpoly_group.so")


def srpoly_group_lib() -> C.CDLL:
    """Load libhpccg_hip_srpoly_group.so (include/hpccg_hip_srpoly_group.h) on
    first use. It is linked against libhpccg_hip.so beside it, so lib() is
    loaded first and both share one copy of the main library."""
    return _load_unit("srpoly_group", SRPOLY_GROUP_LIB_PATH, "the group srpoly library", "the group single-reduction polynomial solve has no fallback", {
        "hpccg_hip_group_srpoly_abi_version": (_ip, []),
        "hpccg_hip_group_srpoly_solve_device": (_ip, [_PV, _ip, _ip, _PV, _PL, _PV, _PL, _PV, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_group_srpoly_bound": (_ip, [_PV, _ip, _PV, _PD]),
        "hpccg_hip_group_srpoly_last_spectrum": (_ip, [_PV, _ip, _PD, _PD]),
        "hpccg_hip_group_srpoly_last_trace": (_ip, [_PV, _ip, _ip, _PD, _ip]),
        "hpccg_hip_group_srpoly_release": (_ip, [_vp]),
        "hpccg_hip_group_srpoly_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_group_srpoly_live_workspaces": (_ip, [_PI]),
    })


POLY_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_poly.so")


def poly_lib() -> C.CDLL:
    """Load libhpccg_hip_poly.so (include/hpccg_hip_poly.h) on first use. It is
    linked against libhpccg_hip.so beside it, so lib() is loaded first and both
    share one copy of the main library."""
    return _load_unit("poly", POLY_LIB_PATH, "the poly library", "the polynomial solve has no fallback", {
        "hpccg_hip_poly_abi_version": (_ip, []),
        "hpccg_hip_poly_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_poly_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_poly_bound": (_ip, [_vp, _vp, _PD]),
        "hpccg_hip_poly_last_spectrum": (_ip, [_vp, _PD, _PD]),
        "hpccg_hip_poly_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_poly_release": (_ip, [_vp]),
        "hpccg_hip_poly_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_poly_live_workspaces": (_ip, [_PI]),
    })


POLY_GROUP_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_poly_group.so")


def poly_group_lib() -> C.CDLL:
    """Load libhpccg_hip_poly_group.so (include/hpccg_hip_poly_group.h) on first
    use. It is linked against libhpccg_hip.so beside it, so lib() is loaded
    first and both share one copy of the main library."""
    return _load_unit("poly_group", POLY_GROUP_LIB_PATH, "the group poly library", "the group polynomial solve has no fallback", {
        "hpccg_hip_group_poly_abi_version": (_ip, []),
        "hpccg_hip_group_poly_solve_device": (_ip, [_PV, _ip, _ip, _PV, _PL, _PV, _PL, _PV, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_group_poly_bound": (_ip, [_PV, _ip, _PV, _PD]),
        "hpccg_hip_group_poly_last_spectrum": (_ip, [_PV, _ip, _PD, _PD]),
        "hpccg_hip_group_poly_last_trace": (_ip, [_PV, _ip, _ip, _PD, _ip]),
        "hpccg_hip_group_poly_release": (_ip, [_vp]),
        "hpccg_hip_group_poly_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_group_poly_live_workspaces": (_ip, [_PI]),
    })


POLY32_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_poly32.so")


def poly32_lib() -> C.CDLL:
    """Load libhpccg_hip_poly32.so (include/hpccg_hip_poly32.h) on first use. It
    is linked against libhpccg_hip.so beside it, so lib() is loaded first and
    both share one copy of the main library."""
    return _load_unit("poly32", POLY32_LIB_PATH, "the poly32 library", "the fp32-image polynomial solve has no fallback", {
        "hpccg_hip_poly32_abi_version": (_ip, []),
        "hpccg_hip_poly32_solve_device": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_poly32_solve": (_ip, [_vp, _ip, _vp, _lp, _vp, _lp, _vp, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_poly32_bound": (_ip, [_vp, _vp, _PD]),
        "hpccg_hip_poly32_last_spectrum": (_ip, [_vp, _PD, _PD]),
        "hpccg_hip_poly32_last_trace": (_ip, [_vp, _ip, _PD, _ip]),
        "hpccg_hip_poly32_info": (_ip, [_vp, _PL]),
        "hpccg_hip_poly32_release": (_ip, [_vp]),
        "hpccg_hip_poly32_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_poly32_live_workspaces": (_ip, [_PI]),
    })


POLY32_GROUP_LIB_PATH = os.path.join(HERE, "lib", "libhpccg_hip_poly32_group.so")


def poly32_group_lib() -> C.CDLL:
    """Load libhpccg_hip_poly32_group.so (include/hpccg_hip_poly32_group.h) on
    first use. It is linked against libhpccg_hip.so beside it, so lib() is
    loaded first and both share one copy of the main library."""
    return _load_unit("poly32_group", POLY32_GROUP_LIB_PATH, "the group poly32 library", "the group fp32-image polynomial solve has no fallback", {
        "hpccg_hip_group_poly32_abi_version": (_ip, []),
        "hpccg_hip_group_poly32_solve_device": (_ip, [_PV, _ip, _ip, _PV, _PL, _PV, _PL, _PV, _ip, _dp, _dp, _ip, _dp, _PI, _PD, _PD]),
        "hpccg_hip_group_poly32_bound": (_ip, [_PV, _ip, _PV, _PD]),
        "hpccg_hip_group_poly32_last_spectrum": (_ip, [_PV, _ip, _PD, _PD]),
        "hpccg_hip_group_poly32_last_trace": (_ip, [_PV, _ip, _ip, _PD, _ip]),
        "hpccg_hip_group_poly32_info": (_ip, [_PV, _ip, _PL]),
        "hpccg_hip_group_poly32_release": (_ip, [_vp]),
        "hpccg_hip_group_poly32_workspace_bytes": (_ip, [_vp, _PL]),
        "hpccg_hip_group_poly32_live_workspaces": (_ip, [_PI]),
    })


def _declared(header: str, pattern: str) -> list[str]:
    """The names pattern finds in include/<header>, sorted."""
    import re
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(pattern, f.read())))


def group_poly32_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_poly32_group.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_poly32_group.h", r"\b(hpccg_hip_group_poly32_\w+)\s*\(")


def poly32_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_poly32.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_poly32.h", r"\b(hpccg_hip_poly32_\w+)\s*\(")


def group_srpoly_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_srpoly_group.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_srpoly_group.h", r"\b(hpccg_hip_group_srpoly_\w+)\s*\(")


def srpoly_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_srpoly.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_srpoly.h", r"\b(hpccg_hip_srpoly_\w+)\s*\(")


def group_poly_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_poly_group.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_poly_group.h", r"\b(hpccg_hip_group_poly_\w+)\s*\(")


def poly_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_poly.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_poly.h", r"\b(hpccg_hip_poly_\w+)\s*\(")


def group_pcg_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_pcg_group.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_pcg_group.h", r"\b(hpccg_hip_group_pcg_\w+)\s*\(")


def pcg_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_pcg.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_pcg.h", r"\b(hpccg_hip_pcg_\w+)\s*\(")


def srcg_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_srcg.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_srcg.h", r"\b(hpccg_hip_srcg_\w+)\s*\(")


def bicgstab_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_bicgstab.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_bicgstab.h", r"\b(hpccg_hip_bicgstab_\w+)\s*\(")


def group_srcg_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_srcg_group.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_srcg_group.h", r"\b(hpccg_hip_group_srcg_\w+)\s*\(")


def mixed_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_mixed.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_mixed.h", r"\b(hpccg_hip_mixed_\w+)\s*\(")


def batch_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_batch.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_batch.h", r"\b(hpccg_hip_batch_\w+)\s*\(")


def group_batch_exported_symbols() -> list[str]:
    """Functions include/hpccg_hip_batch_group.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip_batch_group.h", r"\b(hpccg_hip_group_batch_\w+)\s*\(")


def exported_symbols() -> list[str]:
    """Functions include/hpccg_hip.h declares (checked by the CPU suite)."""
    return _declared("hpccg_hip.h", r"\b(hpccg_\w+)\s*\(")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().hpccg_hip_last_error().decode(errors="replace")
        raise HPCCGError(f"{what} failed ({rc}): {msg}")


def _live(slot: str, name: str) -> int:
    """hpccg_hip_<name>'s count; 0 when the unit's library was never loaded."""
    L = _units.get(slot)
    if L is None:
        return 0
    c = C.c_int(0)
    _check(getattr(L, "hpccg_hip_" + name)(C.byref(c)), name)
    return c.value


def _workspace_bytes(slot: str, name: str, h) -> int:
    """hpccg_hip_<name>'s bytes of matrix h; 0 when the unit's library was never loaded."""
    L = _units.get(slot)
    if L is None:
        return 0
    v = C.c_longlong(0)
    _check(getattr(L, "hpccg_hip_" + name)(h, C.byref(v)), name)
    return v.value


def _release(slot: str, name: str, h) -> None:
    """hpccg_hip_<name> on matrix h, where there is one and the unit's library was ever loaded."""
    L = _units.get(slot)
    if h and L is not None:
        _check(getattr(L, "hpccg_hip_" + name)(h), name)


def _ptr(a) -> int:
    """Device pointer of a torch tensor (or an int). Work torch queued on the
    tensor is completed first: the library runs on its own HIP stream."""
    if isinstance(a, int):
        return a
    if a.is_cuda:
        import time
        import torch
        s = torch.cuda.current_stream(a.device)
        while not s.query():  # polled (a blocking synchronize wakes ~0.1 ms late), the GIL released
            time.sleep(0)
    return a.data_ptr()


# ---------------------------------------------------------------------------
# host problem (reference generate_matrix)
# ---------------------------------------------------------------------------
class Problem:
    """A host HPC_Sparse_Matrix with x0, b, xexact (owned; freed on close)."""

    def __init__(self, A, x, b, xe, nrow):
        self.A, self._x, self._b, self._xe, self.nrow = A, x, b, xe, nrow

    @property
    def x(self) -> np.ndarray:
        return np.ctypeslib.as_array(self._x, (self.nrow,)).copy()

    @property
    def b(self) -> np.ndarray:
        return np.ctypeslib.as_array(self._b, (self.nrow,)).copy()

    @property
    def xexact(self) -> np.ndarray:
        return np.ctypeslib.as_array(self._xe, (self.nrow,)).copy()

    def to_csr(self):
        """(row_ptr int64, cols int32, vals float64) in stored entry order."""
        A = self.A.contents
        n = A.local_nrow
        lens = np.ctypeslib.as_array(A.nnz_in_row, (n,)).astype(np.int64)
        row_ptr = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=row_ptr[1:])
        nnz = int(row_ptr[-1])
        base_v = C.cast(A.list_of_vals, C.c_void_p).value
        base_i = C.cast(A.list_of_inds, C.c_void_p).value
        vals = np.ctypeslib.as_array(A.list_of_vals, (nnz,)).copy()
        cols = np.ctypeslib.as_array(A.list_of_inds, (nnz,)).copy()
        # rows are laid out back to back from list_of_* (generate_matrix.cpp:247-258)
        first_v = C.cast(A.ptr_to_vals_in_row[0], C.c_void_p).value if n else base_v
        first_i = C.cast(A.ptr_to_inds_in_row[0], C.c_void_p).value if n else base_i
        assert first_v == base_v and first_i == base_i
        return row_ptr, cols, vals

    def close(self):
        if self.A:
            lib().hpccg_free_problem(self.A, self._x, self._b, self._xe)
            self.A = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generate_matrix(nx, ny, nz, rank=0, size=1, use_7pt=False) -> Problem:
    L = lib()
    A = C.POINTER(_HPCMatrix)()
    x, b, xe = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
    _check(L.hpccg_generate_matrix(nx, ny, nz, rank, size, int(use_7pt), C.byref(A), C.byref(x),
                                   C.byref(b), C.byref(xe)), "generate_matrix")
    return Problem(A, x, b, xe, nx * ny * nz)


def read_HPC_row(data_file: str, rank=0, size=1) -> Problem:
    """read_HPC_row.cpp:217-373 (Mode 2): rank's block of rows of the system in
    data_file (global columns), with x0, b, xexact from the file."""
    L = lib()
    A = C.POINTER(_HPCMatrix)()
    x, b, xe = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
    _check(L.hpccg_read_HPC_row(os.fsencode(data_file), rank, size, C.byref(A), C.byref(x), C.byref(b),
                                C.byref(xe)), "read_HPC_row")
    p = Problem(A, x, b, xe, A.contents.local_nrow)
    p.start_row = A.contents.start_row
    p.total_nrow = A.contents.total_nrow
    p.total_nnz = A.contents.total_nnz
    return p


def set_halo_mode(mode: int) -> None:
    """0 auto, 1 z-slab only, 2 gather plan (matrices created afterwards)."""
    _check(lib().hpccg_hip_set_halo_mode(mode), "set_halo_mode")


def set_keep_sell(keep: bool) -> None:
    """Matrices created afterwards keep their SELL-512 image beside SELL-512-A
    (kernel A/B comparisons only; default off)."""
    _check(lib().hpccg_hip_set_keep_sell(int(keep)), "set_keep_sell")


def set_placement_probe(tries: int) -> None:
    """Placement probe of matrices created afterwards: -1 auto (6 candidates
    when the values exceed 512 MB), 0 off, 1..16 candidates."""
    _check(lib().hpccg_hip_set_placement_probe(int(tries)), "set_placement_probe")


SPMV_SELL, SPMV_DIRECT, SPMV_PAIRS = 0, 1, 2
SPMV_KERNEL_NAMES = {0: "SELL-512 (int32 columns, x gathered)",
                     1: "SELL-512-A (offset-aligned slots, x read at the slice's offsets)",
                     2: "SELL-512-A (offset-aligned slots, x from LDS windows shared by slice pairs)"}


# ---------------------------------------------------------------------------
# device matrix
# ---------------------------------------------------------------------------
class Matrix:
    def __init__(self, handle):
        self.h = handle

    @classmethod
    def from_hpc(cls, prob: Problem) -> "Matrix":
        h = C.c_void_p()
        _check(lib().hpccg_hip_matrix_create(prob.A, C.byref(h)), "matrix_create")
        return cls(h)

    @classmethod
    def from_csr(cls, row_ptr, cols, vals, start_row=0, total_nrow=None) -> "Matrix":
        row_ptr = np.ascontiguousarray(row_ptr, np.int64)
        cols = np.ascontiguousarray(cols, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        n = len(row_ptr) - 1
        total = n if total_nrow is None else total_nrow
        h = C.c_void_p()
        _check(lib().hpccg_hip_matrix_create_csr(n, start_row, total, row_ptr.ctypes.data,
                                                 cols.ctypes.data, vals.ctypes.data, C.byref(h)),
               "matrix_create_csr")
        return cls(h)

    @classmethod
    def generate(cls, nx, ny, nz, use_7pt=False) -> "Matrix":
        h = C.c_void_p()
        _check(lib().hpccg_hip_matrix_generate(nx, ny, nz, int(use_7pt), C.byref(h)),
               "matrix_generate")
        return cls(h)

    def info(self) -> dict:
        a = (C.c_longlong * 8)()
        _check(lib().hpccg_hip_matrix_info(self.h, a), "matrix_info")
        return {"nrow": a[0], "ncol": a[1], "nnz": a[2], "slots": a[3], "ghost_lo": a[4],
                "ghost_hi": a[5], "spmv_kernel": a[6], "uniform_width": a[7]}

    def vectors(self):
        """Device pointers (b, x0, xexact) of a device-generated matrix."""
        b, x0, xe = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().hpccg_hip_matrix_vectors(self.h, C.byref(b), C.byref(x0), C.byref(xe)),
               "matrix_vectors")
        return b.value, x0.value, xe.value

    def set_option(self, key: str, value: int) -> None:
        _check(lib().hpccg_hip_set_option(self.h, key.encode(), int(value)), "set_option")

    def get_option(self, key: str) -> int:
        v = C.c_longlong(0)
        _check(lib().hpccg_hip_get_option(self.h, key.encode(), C.byref(v)), "get_option")
        return v.value

    def kernel_times(self) -> dict:
        """hipEvent timings of the last solve (needs set_option('event_timing', 1))."""
        out = (C.c_double * 4)()
        _check(lib().hpccg_hip_kernel_times(self.h, out), "kernel_times")
        return {"spmv_ms": out[0], "spmv_launches": int(out[1]), "update_ms": out[2],
                "update_launches": int(out[3])}

    def kernel_times_iter(self, cap: int = 100000) -> np.ndarray:
        """Per-iteration (SpMV ms, update ms) of the last event-timed solve."""
        out = np.zeros(2 * cap, np.float64)
        n = lib().hpccg_hip_kernel_times_iter(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "kernel_times_iter")
        return out[:2 * n].reshape(n, 2)

    def diag_spmv(self, kernel: int, reps: int = 20) -> float:
        """Average us per launch of an SpMV kernel (0 SELL-512, 1 SELL-512-A
        direct, 2 SELL-512-A pair windows), prologue form (diagnostics)."""
        us = C.c_double(0.0)
        _check(lib().hpccg_hip_diag_spmv(self.h, kernel, reps, C.byref(us)), "diag_spmv")
        return us.value

    def diag_timeline(self) -> np.ndarray:
        """Block timeline (option dbg_timeline 1) of the last SpMV launch
        that ran an iteration, 8 words per row (include/hpccg_hip.h): the ring
        pair kernel one row per pair, the direct kernel's fused-update
        defaults one row per block of the launch."""
        cap = 3 * ((int(self.info()["nrow"]) + 511) // 512) + 1024  # the buffer: every block of any launch
        out = np.zeros(cap * 8, np.uint64)
        n = lib().hpccg_hip_diag_timeline(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), cap)
        _check(n if n < 0 else 0, "diag_timeline")
        return out[:8 * n].reshape(n, 8)

    def diag_realloc(self, which: int, mode: int = 0) -> int:
        """Move a device buffer to new memory (0 values, 1 p ring, 2 r, 3 Ap,
        4 x) allocated by mode (0 hipMalloc, 1 contiguous, 2/3/4 VMM at 2 MB /
        64 MB / 1 GB alignment); returns its virtual address (diagnostics:
        physical placement)."""
        va = C.c_uint64(0)
        _check(lib().hpccg_hip_diag_realloc(self.h, which | (mode << 8), C.byref(va)), "diag_realloc")
        return va.value

    def probe_placement(self, tries: int = 6) -> np.ndarray:
        """Time CG iterations on the current placement, then on up to `tries`
        contiguous placements of the values (keep the fastest), then of the p
        ring, r and Ap (likewise); results unchanged. Returns placement()."""
        _check(lib().hpccg_hip_probe_placement(self.h, int(tries)), "probe_placement")
        return self.placement()

    def placement(self) -> np.ndarray:
        """us per CG iteration of each candidate of the last placement probe
        ([0] the placement before it, then the values, ring, r and Ap
        candidates in turn; empty if none ran). Option placement_pick: one
        byte per buffer, values | ring << 8 | r << 16 | Ap << 24."""
        out = np.zeros(65, np.float64)
        n = lib().hpccg_hip_diag_placement(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), 65)
        _check(n if n < 0 else 0, "diag_placement")
        return out[:n]

    def last_trace(self, cap: int = 100000) -> np.ndarray:
        out = np.zeros(cap, np.float64)
        n = lib().hpccg_hip_last_trace(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        return out[:max(n, 0)]

    def last_trace_batch(self, col: int, cap: int = 100000) -> np.ndarray:
        """Residual trace of column col of the last HPCCG_batch on this matrix."""
        out = np.zeros(cap, np.float64)
        n = batch_lib().hpccg_hip_batch_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_trace_batch")
        return out[:n]

    def batch_release(self) -> None:
        """Free this matrix's batch workspace now (close() does it too)."""
        _release("batch", "batch_release", self.h)

    def batch_workspace_bytes(self) -> int:
        return _workspace_bytes("batch", "batch_workspace_bytes", self.h)

    def mixed_info(self) -> dict:
        """The fp32 image of this matrix (built on first use): exact (every
        value survives double -> float -> double: the mixed solve is then
        bitwise the fp64 solve), its device bytes, the device bytes of the rest
        of the mixed workspace, and the values that did not survive."""
        a = (C.c_longlong * 4)()
        _check(mixed_lib().hpccg_hip_mixed_info(self.h, a), "mixed_info")
        return {"exact": int(a[0]), "image_bytes": int(a[1]), "workspace_bytes": int(a[2]), "inexact_values": int(a[3])}

    def last_trace_mixed(self, col: int, cap: int = 100000) -> np.ndarray:
        """The inner recurrences' normr of column col of the last HPCCG_mixed on
        this matrix, sweep after sweep (it_s + 1 entries each)."""
        out = np.zeros(cap, np.float64)
        n = mixed_lib().hpccg_hip_mixed_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_trace_mixed")
        return out[:n]

    def last_sweeps_mixed(self, col: int, cap: int = 4096):
        """(iters, resid) of column col of the last HPCCG_mixed: the inner
        iterations of every sweep, and the fp64 residual norm before every
        sweep with the final one appended (len(resid) == len(iters) + 1)."""
        it = np.zeros(cap, np.int32)
        rs = np.zeros(cap, np.float64)
        n = mixed_lib().hpccg_hip_mixed_last_sweeps(self.h, int(col), it.ctypes.data_as(C.POINTER(C.c_int)),
                                                    rs.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_sweeps_mixed")
        return it[:n], rs[:n + 1]

    def mixed_release(self) -> None:
        """Free this matrix's mixed workspace and fp32 image now (close() does it too)."""
        _release("mixed", "mixed_release", self.h)

    def mixed_workspace_bytes(self) -> int:
        return _workspace_bytes("mixed", "mixed_workspace_bytes", self.h)

    def diagonal_pcg(self) -> np.ndarray:
        """The matrix's diagonal as the preconditioned solve reads it from the
        device image (0.0 where a row stores none)."""
        import torch
        n = int(self.info()["nrow"])
        d = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
        _check(pcg_lib().hpccg_hip_pcg_diagonal(self.h, _ptr(d)), "diagonal_pcg")
        return d.cpu().numpy()[:n].copy()

    def last_trace_pcg(self, col: int, cap: int = 100000) -> np.ndarray:
        """Residual trace (norm of r) of column col of the last HPCCG_pcg on this matrix."""
        out = np.zeros(cap, np.float64)
        n = pcg_lib().hpccg_hip_pcg_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_trace_pcg")
        return out[:n]

    def pcg_release(self) -> None:
        """Free this matrix's pcg workspace (with its cached 1 / a_ii) now (close() does it too)."""
        _release("pcg", "pcg_release", self.h)

    def pcg_workspace_bytes(self) -> int:
        return _workspace_bytes("pcg", "pcg_workspace_bytes", self.h)

    def last_trace_srcg(self, col: int, cap: int = 100000) -> np.ndarray:
        """Residual trace (norm of r) of column col of the last HPCCG_srcg on this matrix."""
        out = np.zeros(cap, np.float64)
        n = srcg_lib().hpccg_hip_srcg_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_trace_srcg")
        return out[:n]

    def srcg_release(self) -> None:
        """Free this matrix's srcg workspace (with its cached 1 / a_ii) now (close() does it too)."""
        _release("srcg", "srcg_release", self.h)

    def srcg_workspace_bytes(self) -> int:
        return _workspace_bytes("srcg", "srcg_workspace_bytes", self.h)

    def last_trace_bicgstab(self, col: int, cap: int = 100000) -> np.ndarray:
        """Residual trace (norm of r) of column col of the last HPCCG_bicgstab on this matrix."""
        out = np.zeros(cap, np.float64)
        n = bicgstab_lib().hpccg_hip_bicgstab_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)),
                                                         cap)
        if n < 0:
            _check(n, "last_trace_bicgstab")
        return out[:n]

    def last_status_bicgstab(self, col: int) -> int:
        """How column col of the last HPCCG_bicgstab on this matrix ended: 0 the
        loop test, 1 breakdown, 2 an exactly zero residual."""
        st = C.c_int(-1)
        _check(bicgstab_lib().hpccg_hip_bicgstab_last_status(self.h, int(col), C.byref(st)), "last_status_bicgstab")
        return st.value

    def bicgstab_release(self) -> None:
        """Free this matrix's bicgstab workspace (with its cached 1 / a_ii) now (close() does it too)."""
        _release("bicgstab", "bicgstab_release", self.h)

    def bicgstab_workspace_bytes(self) -> int:
        return _workspace_bytes("bicgstab", "bicgstab_workspace_bytes", self.h)

    def last_trace_poly(self, col: int, cap: int = 100000) -> np.ndarray:
        """Residual trace (norm of r) of column col of the last HPCCG_poly on this matrix."""
        out = np.zeros(cap, np.float64)
        n = poly_lib().hpccg_hip_poly_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_trace_poly")
        return out[:n]

    def last_spectrum_poly(self) -> tuple:
        """(lmin, lmax) the last HPCCG_poly on this matrix used."""
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _check(poly_lib().hpccg_hip_poly_last_spectrum(self.h, C.byref(lo), C.byref(hi)), "last_spectrum_poly")
        return lo.value, hi.value

    def poly_release(self) -> None:
        """Free this matrix's poly workspace (with its cached 1 / a_ii and bound) now (close() does it too)."""
        _release("poly", "poly_release", self.h)

    def poly_workspace_bytes(self) -> int:
        return _workspace_bytes("poly", "poly_workspace_bytes", self.h)

    def last_trace_srpoly(self, col: int, cap: int = 100000) -> np.ndarray:
        """Residual trace (norm of r) of column col of the last HPCCG_srpoly on this matrix."""
        out = np.zeros(cap, np.float64)
        n = srpoly_lib().hpccg_hip_srpoly_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_trace_srpoly")
        return out[:n]

    def last_spectrum_srpoly(self) -> tuple:
        """(lmin, lmax) the last HPCCG_srpoly on this matrix used."""
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _check(srpoly_lib().hpccg_hip_srpoly_last_spectrum(self.h, C.byref(lo), C.byref(hi)), "last_spectrum_srpoly")
        return lo.value, hi.value

    def srpoly_release(self) -> None:
        """Free this matrix's srpoly workspace (with its cached 1 / a_ii and bound) now (close() does it too)."""
        _release("srpoly", "srpoly_release", self.h)

    def srpoly_workspace_bytes(self) -> int:
        return _workspace_bytes("srpoly", "srpoly_workspace_bytes", self.h)

    def last_trace_poly32(self, col: int, cap: int = 100000) -> np.ndarray:
        """Residual trace (norm of r) of column col of the last HPCCG_poly32 on this matrix."""
        out = np.zeros(cap, np.float64)
        n = poly32_lib().hpccg_hip_poly32_last_trace(self.h, int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
        if n < 0:
            _check(n, "last_trace_poly32")
        return out[:n]

    def last_spectrum_poly32(self) -> tuple:
        """(lmin, lmax) the last HPCCG_poly32 on this matrix used."""
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _check(poly32_lib().hpccg_hip_poly32_last_spectrum(self.h, C.byref(lo), C.byref(hi)), "last_spectrum_poly32")
        return lo.value, hi.value

    def poly32_release(self) -> None:
        """Free this matrix's poly32 workspace and fp32 image now (close() does it too)."""
        _release("poly32", "poly32_release", self.h)

    def poly32_workspace_bytes(self) -> int:
        return _workspace_bytes("poly32", "poly32_workspace_bytes", self.h)

    def close(self):
        # (a batch workspace goes with the matrix: the library's destroy hook,
        # whether or not the batch library was ever loaded)
        if self.h:
            lib().hpccg_hip_matrix_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dropin_HPCCG(prob: Problem, x: np.ndarray, max_iter: int = 500, tolerance: float = 0.0):
    """The C drop-in hpccg_hip_HPCCG (HPCCG.hpp:61-63 signature) on a host
    problem: device matrix cached per HPC_Sparse_Matrix (address + content
    fingerprint). Returns (ierr, niters, normr, times)."""
    it = C.c_int(0)
    nr = C.c_double(0.0)
    times = np.zeros(7, np.float64)
    b = np.ascontiguousarray(prob.b, np.float64)
    assert x.dtype == np.float64 and x.flags.c_contiguous
    rc = lib().hpccg_hip_HPCCG(prob.A, b.ctypes.data, x.ctypes.data, max_iter, tolerance, C.byref(it),
                               C.byref(nr), times.ctypes.data_as(C.POINTER(C.c_double)))
    _check(rc, "hpccg_hip_HPCCG")
    return rc, it.value, nr.value, times


def HPCCG(M: Matrix, b, x, max_iter: int = 500, tolerance: float = 0.0, print_residuals=False,
          device=False):
    """HPCCG.cpp:312-402. b, x: numpy (host) or, with device=True, device
    pointers/tensors. x is updated in place. Returns (ierr, niters, normr, times)."""
    it = C.c_int(0)
    nr = C.c_double(0.0)
    times = np.zeros(7, np.float64)
    tp = times.ctypes.data_as(C.POINTER(C.c_double))
    L = lib()
    if device:
        rc = L.hpccg_hip_solve_device(M.h, _ptr(b), _ptr(x), max_iter, tolerance, C.byref(it),
                                      C.byref(nr), tp, int(print_residuals))
    else:
        assert x.dtype == np.float64 and x.flags.c_contiguous
        bb = np.ascontiguousarray(b, np.float64)
        rc = L.hpccg_hip_solve(M.h, bb.ctypes.data, x.ctypes.data, max_iter, tolerance,
                               C.byref(it), C.byref(nr), tp, int(print_residuals))
    _check(rc, "HPCCG")
    return rc, it.value, nr.value, times


# ---------------------------------------------------------------------------
# batched multi-right-hand-side solve (include/hpccg_hip_batch.h)
# ---------------------------------------------------------------------------
def _cols(a, nrhs, ld, what):
    """(pointer, nrhs, ld) of a column set: a 2-D array whose row c is column c
    (numpy C-contiguous float64, or a torch tensor with unit inner stride; the
    row stride is the leading dimension), or a raw pointer with nrhs and ld."""
    if isinstance(a, int):
        if nrhs is None or ld is None:
            raise HPCCGError(f"{what}: a raw pointer needs nrhs and its leading dimension")
        return a, int(nrhs), int(ld)
    if isinstance(a, np.ndarray):
        if a.dtype != np.float64 or a.ndim != 2 or not a.flags.c_contiguous:
            raise HPCCGError(f"{what}: a C-contiguous float64 array of shape (nrhs, ld)")
        return a.ctypes.data, a.shape[0], a.shape[1] if ld is None else int(ld)
    if a.dim() != 2 or (a.shape[1] > 1 and a.stride(1) != 1):
        raise HPCCGError(f"{what}: a 2-D tensor of shape (nrhs, ld) with unit inner stride")
    if ld is None:
        ld = a.stride(0) if a.shape[0] > 1 else a.shape[1]
    return _ptr(a), a.shape[0], int(ld)


def HPCCG_batch(M: Matrix, B, X, max_iter: int = 500, tolerance: float = 0.0, device=False, nrhs=None,
                ldb=None, ldx=None):
    """nrhs CG solves against M in one pass over the matrix per iteration
    (hpccg_hip_batch_solve[_device]); column c is bitwise HPCCG(M, B[c], X[c]).
    B, X: shape (nrhs, ld) with row c holding column c (ld >= nrow; the C
    ABI's column-major layout) -- numpy on the host or, with device=True,
    tensors / device pointers. X is updated in place. Returns
    (ierr, niters[nrhs], normr[nrhs], times)."""
    L = batch_lib()
    bp, nb, ldb_ = _cols(B, nrhs, ldb, "B")
    xp, nx_, ldx_ = _cols(X, nrhs, ldx, "X")
    if nb != nx_:
        raise HPCCGError(f"B holds {nb} columns, X {nx_}")
    if not device and not (isinstance(B, np.ndarray) and isinstance(X, np.ndarray)):
        raise HPCCGError("host solve: B and X are numpy arrays")
    it = np.zeros(max(nb, 1), np.int32)
    nr = np.zeros(max(nb, 1), np.float64)
    times = np.zeros(7, np.float64)
    f = L.hpccg_hip_batch_solve_device if device else L.hpccg_hip_batch_solve
    rc = f(M.h, nb, bp, ldb_, xp, ldx_, max_iter, tolerance, it.ctypes.data_as(C.POINTER(C.c_int)),
           nr.ctypes.data_as(C.POINTER(C.c_double)), times.ctypes.data_as(C.POINTER(C.c_double)))
    _check(rc, "HPCCG_batch")
    return rc, it[:nb], nr[:nb], times


def HPC_sparsemv_batch(M: Matrix, X, Y, nrhs=None, ldx=None, ldy=None) -> int:
    """Y[c] = A X[c] for every column (device tensors / pointers, shape
    (nrhs, ld)); each column is bitwise HPC_sparsemv of that column."""
    xp, nx_, ldx_ = _cols(X, nrhs, ldx, "X")
    yp, ny_, ldy_ = _cols(Y, nrhs, ldy, "Y")
    if nx_ != ny_:
        raise HPCCGError(f"X holds {nx_} columns, Y {ny_}")
    _check(batch_lib().hpccg_hip_batch_sparsemv(M.h, nx_, xp, ldx_, yp, ldy_), "HPC_sparsemv_batch")
    return 0


def batch_live_workspaces() -> int:
    """Matrices that hold a batch workspace (0 when the library was never loaded)."""
    return _live("batch", "batch_live_workspaces")



# ---------------------------------------------------------------------------
# mixed-precision solve (include/hpccg_hip_mixed.h)
# ---------------------------------------------------------------------------
def _one_column(a, what):
    """A 1-D array or tensor as one column, shape (1, n): a view of the same
    memory (X is updated in place), so it must have unit stride."""
    if isinstance(a, int) or a.ndim != 1:
        return a
    stride = a.strides[0] // a.itemsize if isinstance(a, np.ndarray) else a.stride(0)
    if a.shape[0] > 1 and stride != 1:
        raise HPCCGError(f"{what}: a 1-D column must be contiguous (stride {stride})")
    return a[None, :]


def HPCCG_mixed(M: Matrix, B, X, max_iter: int = 500, tolerance: float = 0.0, max_sweeps: int = 8,
                inner_rtol: float = -1.0, device=False, nrhs=None, ldb=None, ldx=None):
    """nrhs CG solves against M with the matrix values streamed from an fp32
    image, all arithmetic in fp64 (hpccg_hip_mixed_solve[_device]). Where the
    image is exact (Matrix.mixed_info) column c is bitwise HPCCG(M, B[c], X[c]);
    otherwise the solve is an iterative refinement against the fp64 matrix and
    normr is the fp64 residual norm of the returned x. B, X: as HPCCG_batch (a
    1-D array or tensor is one column). X is updated in place. Returns
    (ierr, niters[nrhs], normr[nrhs], times)."""
    L = mixed_lib()
    B, X = _one_column(B, "B"), _one_column(X, "X")
    bp, nb, ldb_ = _cols(B, nrhs, ldb, "B")
    xp, nx_, ldx_ = _cols(X, nrhs, ldx, "X")
    if nb != nx_:
        raise HPCCGError(f"B holds {nb} columns, X {nx_}")
    if not device and not (isinstance(B, np.ndarray) and isinstance(X, np.ndarray)):
        raise HPCCGError("host solve: B and X are numpy arrays")
    it = np.zeros(max(nb, 1), np.int32)
    nr = np.zeros(max(nb, 1), np.float64)
    times = np.zeros(7, np.float64)
    f = L.hpccg_hip_mixed_solve_device if device else L.hpccg_hip_mixed_solve
    rc = f(M.h, nb, bp, ldb_, xp, ldx_, max_iter, tolerance, int(max_sweeps), float(inner_rtol),
           it.ctypes.data_as(C.POINTER(C.c_int)), nr.ctypes.data_as(C.POINTER(C.c_double)),
           times.ctypes.data_as(C.POINTER(C.c_double)))
    _check(rc, "HPCCG_mixed")
    return rc, it[:nb], nr[:nb], times


def HPC_sparsemv_mixed(M: Matrix, X, Y, nrhs=None, ldx=None, ldy=None) -> int:
    """Y[c] = A~ X[c] for every column, A~ being the fp32 image of M (device
    tensors / pointers, shape (nrhs, ld))."""
    xp, nx_, ldx_ = _cols(X, nrhs, ldx, "X")
    yp, ny_, ldy_ = _cols(Y, nrhs, ldy, "Y")
    if nx_ != ny_:
        raise HPCCGError(f"X holds {nx_} columns, Y {ny_}")
    _check(mixed_lib().hpccg_hip_mixed_sparsemv(M.h, nx_, xp, ldx_, yp, ldy_), "HPC_sparsemv_mixed")
    return 0


def mixed_live_workspaces() -> int:
    """Matrices that hold a mixed workspace (0 when the library was never loaded)."""
    return _live("mixed", "mixed_live_workspaces")


# ---------------------------------------------------------------------------
# diagonally preconditioned solve (include/hpccg_hip_pcg.h)
# ---------------------------------------------------------------------------
def _minv_ptr(M: Matrix, minv, device):
    """(pointer, keep-alive) of a caller's m: nrow entries, host or device."""
    nrow = int(M.info()["nrow"])
    if device:
        if not isinstance(minv, int) and (minv.dim() != 1 or minv.shape[0] < nrow or
                                          (minv.shape[0] > 1 and minv.stride(0) != 1)):
            raise HPCCGError(f"minv: a contiguous 1-D tensor of {nrow} entries")
        return _ptr(minv), minv
    keep = np.ascontiguousarray(minv, np.float64)
    if keep.ndim != 1 or keep.shape[0] < nrow:
        raise HPCCGError(f"minv: a 1-D array of {nrow} entries")
    return keep.ctypes.data, keep


def _column_solve(what, solve, M, B, X, minv, device, nrhs, ldb, ldx, *rest):
    """What the one-rank preconditioned solves share: the columns of B and X (a
    1-D array or tensor is one column), a caller's minv, the call of solve
    (the library's host or device entry point; rest: its arguments between
    minv and niters) and the result (ierr, niters[nrhs], normr[nrhs], times)."""
    B, X = _one_column(B, "B"), _one_column(X, "X")
    bp, nb, ldb_ = _cols(B, nrhs, ldb, "B")
    xp, nx_, ldx_ = _cols(X, nrhs, ldx, "X")
    if nb != nx_:
        raise HPCCGError(f"B holds {nb} columns, X {nx_}")
    if not device and not (isinstance(B, np.ndarray) and isinstance(X, np.ndarray)):
        raise HPCCGError("host solve: B and X are numpy arrays")
    mp, keep = (None, None) if minv is None else _minv_ptr(M, minv, device)
    it = np.zeros(max(nb, 1), np.int32)
    nr = np.zeros(max(nb, 1), np.float64)
    times = np.zeros(7, np.float64)
    rc = solve(M.h, nb, bp, ldb_, xp, ldx_, mp, *rest, it.ctypes.data_as(C.POINTER(C.c_int)),
               nr.ctypes.data_as(C.POINTER(C.c_double)), times.ctypes.data_as(C.POINTER(C.c_double)))
    _check(rc, what)
    return rc, it[:nb], nr[:nb], times


def HPCCG_pcg(M: Matrix, B, X, max_iter: int = 500, tolerance: float = 0.0, minv=None, device=False, nrhs=None,
              ldb=None, ldx=None):
    """nrhs preconditioned CG solves against M with M^-1 = diag(minv)
    (hpccg_hip_pcg_solve[_device]); minv None is Jacobi, 1 / a_ii. The loop
    test, niters and normr are on the 2-norm of r, as in HPCCG. B, X: as
    HPCCG_batch (a 1-D array or tensor is one column); minv: nrow entries, all
    finite and > 0 -- numpy on the host or, with device=True, a tensor / device
    pointer. X is updated in place. Returns (ierr, niters[nrhs], normr[nrhs],
    times)."""
    L = pcg_lib()
    return _column_solve("HPCCG_pcg", L.hpccg_hip_pcg_solve_device if device else L.hpccg_hip_pcg_solve, M, B, X, minv,
                         device, nrhs, ldb, ldx, max_iter, tolerance)


def pcg_live_workspaces() -> int:
    """Matrices that hold a pcg workspace (0 when the library was never loaded)."""
    return _live("pcg", "pcg_live_workspaces")


# ---------------------------------------------------------------------------
# single-reduction preconditioned solve (include/hpccg_hip_srcg.h)
# ---------------------------------------------------------------------------
def HPCCG_srcg(M: Matrix, B, X, max_iter: int = 500, tolerance: float = 0.0, minv=None, device=False, nrhs=None,
               ldb=None, ldx=None):
    """HPCCG_pcg in the single-reduction (Chronopoulos-Gear) form
    (hpccg_hip_srcg_solve[_device]): one finalize and three launches per
    iteration for one more vector. Its first iteration is HPCCG_pcg's bit for
    bit; later ones agree to rounding. B, X, minv and the return value: as
    HPCCG_pcg. X is updated in place."""
    L = srcg_lib()
    return _column_solve("HPCCG_srcg", L.hpccg_hip_srcg_solve_device if device else L.hpccg_hip_srcg_solve, M, B, X, minv,
                         device, nrhs, ldb, ldx, max_iter, tolerance)


def srcg_live_workspaces() -> int:
    """Matrices that hold a srcg workspace (0 when the library was never loaded)."""
    return _live("srcg", "srcg_live_workspaces")


# ---------------------------------------------------------------------------
# BiCGStab for non-symmetric matrices (include/hpccg_hip_bicgstab.h)
# ---------------------------------------------------------------------------
def HPCCG_bicgstab(M: Matrix, B, X, max_iter: int = 500, tolerance: float = 0.0, minv=None, device=False, nrhs=None,
                   ldb=None, ldx=None):
    """nrhs right-preconditioned BiCGStab solves against M, symmetric or not,
    with M^-1 = diag(minv) (hpccg_hip_bicgstab_solve[_device]); minv None is
    Jacobi, 1 / a_ii. The loop test, niters and normr are on the 2-norm of r,
    as in HPCCG; how a column ended is M.last_status_bicgstab(c). B, X, minv
    and the return value: as HPCCG_pcg. X is updated in place."""
    L = bicgstab_lib()
    return _column_solve("HPCCG_bicgstab", L.hpccg_hip_bicgstab_solve_device if device else L.hpccg_hip_bicgstab_solve,
                         M, B, X, minv, device, nrhs, ldb, ldx, max_iter, tolerance)


def bicgstab_live_workspaces() -> int:
    """Matrices that hold a bicgstab workspace (0 when the library was never loaded)."""
    return _live("bicgstab", "bicgstab_live_workspaces")


# ---------------------------------------------------------------------------
# Chebyshev polynomial preconditioned solve (include/hpccg_hip_poly.h)
# ---------------------------------------------------------------------------
def _interval(degree, lmin, lmax):
    """degree, lmin, lmax as the polynomial libraries take them (0.0: the default)."""
    return int(degree), 0.0 if lmin is None else float(lmin), 0.0 if lmax is None else float(lmax)


def _poly_solve(what, L, unit, M, B, X, degree, lmin, lmax, minv, device, max_iter, tolerance, nrhs, ldb, ldx):
    """What the one-rank polynomial solves share: library L's
    hpccg_hip_<unit>_solve[_device] through _column_solve."""
    solve = getattr(L, f"hpccg_hip_{unit}_solve_device" if device else f"hpccg_hip_{unit}_solve")
    return _column_solve(what, solve, M, B, X, minv, device, nrhs, ldb, ldx, *_interval(degree, lmin, lmax), max_iter,
                         tolerance)


def _poly_bound(what, bound, M, minv):
    mp, keep = (None, None) if minv is None else _minv_ptr(M, minv, True)
    v = C.c_double(0.0)
    _check(bound(M.h, mp, C.byref(v)), what)
    return v.value


def HPCCG_poly(M: Matrix, B, X, degree: int = 2, lmin=None, lmax=None, minv=None, device=False, max_iter: int = 500,
               tolerance: float = 0.0, nrhs=None, ldb=None, ldx=None):
    """nrhs CG solves against M preconditioned by the Chebyshev polynomial of
    `degree` steps in diag(minv) A on [lmin, lmax] (hpccg_hip_poly_solve[_device]);
    minv None is Jacobi, lmax None the symmetric Gershgorin bound, lmin None
    lmax / 30. Degree 0 is HPCCG_pcg bit for bit. A caller's bounds are not
    verified. The loop test, niters and normr are on the 2-norm of r, as in
    HPCCG. B, X, minv: as HPCCG_pcg. X is updated in place. Returns
    (ierr, niters[nrhs], normr[nrhs], times)."""
    return _poly_solve("HPCCG_poly", poly_lib(), "poly", M, B, X, degree, lmin, lmax, minv, device, max_iter, tolerance,
                       nrhs, ldb, ldx)


def poly_bound(M: Matrix, minv=None) -> float:
    """The symmetric Gershgorin bound on the spectrum of diag(minv) A that
    HPCCG_poly takes for lmax; minv: a device tensor / pointer of nrow entries,
    or None for Jacobi."""
    return _poly_bound("poly_bound", poly_lib().hpccg_hip_poly_bound, M, minv)


def poly_live_workspaces() -> int:
    """Matrices that hold a poly workspace (0 when the library was never loaded)."""
    return _live("poly", "poly_live_workspaces")


# ---------------------------------------------------------------------------
# single-reduction solve with the polynomial preconditioner (include/hpccg_hip_srpoly.h)
# ---------------------------------------------------------------------------
def HPCCG_srpoly(M: Matrix, B, X, degree: int = 2, lmin=None, lmax=None, minv=None, device=False,
                 max_iter: int = 500, tolerance: float = 0.0, nrhs=None, ldb=None, ldx=None):
    """HPCCG_poly in the single-reduction (Chronopoulos-Gear) form
    (hpccg_hip_srpoly_solve[_device]): the three dots of an iteration are
    completed at one point, 3 + degree launches per iteration, for two more
    vectors. Degree 0 is HPCCG_srcg bit for bit; the first iteration
    (max_iter <= 2) is HPCCG_poly bit for bit with the same interval; later
    ones agree to rounding. Arguments and return: HPCCG_poly's. X is updated in
    place."""
    return _poly_solve("HPCCG_srpoly", srpoly_lib(), "srpoly", M, B, X, degree, lmin, lmax, minv, device, max_iter, tolerance,
                       nrhs, ldb, ldx)


def srpoly_bound(M: Matrix, minv=None) -> float:
    """The symmetric Gershgorin bound that HPCCG_srpoly takes for lmax
    (poly_bound's value); minv: a device tensor / pointer of nrow entries, or
    None for Jacobi."""
    return _poly_bound("srpoly_bound", srpoly_lib().hpccg_hip_srpoly_bound, M, minv)


def srpoly_live_workspaces() -> int:
    """Matrices that hold a srpoly workspace (0 when the library was never loaded)."""
    return _live("srpoly", "srpoly_live_workspaces")


# ---------------------------------------------------------------------------
# the polynomial solve with its steps streamed from an fp32 matrix image
# (include/hpccg_hip_poly32.h)
# ---------------------------------------------------------------------------
def HPCCG_poly32(M: Matrix, B, X, degree: int = 2, lmin=None, lmax=None, minv=None, device=False,
                 max_iter: int = 500, tolerance: float = 0.0, nrhs=None, ldb=None, ldx=None):
    """HPCCG_poly with the polynomial's steps reading an fp32 image of the
    matrix values (hpccg_hip_poly32_solve[_device]); the system solved is the
    fp64 one. Where the image is exact (poly32_info) every column is HPCCG_poly
    bit for bit; degree 0 is HPCCG_pcg bit for bit on any matrix. A matrix
    outside fp32 range is refused. Arguments and return: HPCCG_poly's."""
    return _poly_solve("HPCCG_poly32", poly32_lib(), "poly32", M, B, X, degree, lmin, lmax, minv, device, max_iter, tolerance,
                       nrhs, ldb, ldx)


def poly32_bound(M: Matrix, minv=None) -> float:
    """The symmetric Gershgorin bound of the fp64 image that HPCCG_poly32 takes
    for lmax (poly_bound's value); minv: a device tensor / pointer of nrow
    entries, or None for Jacobi."""
    return _poly_bound("poly32_bound", poly32_lib().hpccg_hip_poly32_bound, M, minv)


def poly32_info(M: Matrix) -> dict:
    """The poly32 library's fp32 image of M (built on first use): exact (every
    value survives double -> float -> double: HPCCG_poly32 is then HPCCG_poly
    bit for bit), its device bytes, and the values that did not survive."""
    a = (C.c_longlong * 4)()
    _check(poly32_lib().hpccg_hip_poly32_info(M.h, a), "poly32_info")
    return {"exact": int(a[0]), "image_bytes": int(a[1]), "inexact_values": int(a[2])}


def poly32_live_workspaces() -> int:
    """Matrices that hold a poly32 workspace (0 when the library was never loaded)."""
    return _live("poly32", "poly32_live_workspaces")


# ---------------------------------------------------------------------------
# in-process rank group: the z-slab ranks of one job driven by one thread
# ---------------------------------------------------------------------------
def _ints(v):
    return None if v is None else (C.c_int * len(v))(*[int(d) for d in v])


def group_generate(nx, ny, nz, nranks, use_7pt=False, devices=None) -> list:
    """Rank r of an nranks z-slab job (generate_matrix.cpp:225-229) for every r,
    generated on devices[r] (default: the current device for all)."""
    out = (C.c_void_p * nranks)()
    _check(lib().hpccg_hip_group_generate(nx, ny, nz, int(use_7pt), nranks, _ints(devices), out),
           "group_generate")
    return [Matrix(C.c_void_p(out[r])) for r in range(nranks)]


def group_from_csr(parts, total_nrow, devices=None) -> list:
    """parts[r] = (row_ptr, cols, vals, start_row) of rank r (global columns)."""
    P = len(parts)
    keep = []
    rps, cls, vls = (C.c_void_p * P)(), (C.c_void_p * P)(), (C.c_void_p * P)()
    for r, (rp, cols, vals, _) in enumerate(parts):
        rp = np.ascontiguousarray(rp, np.int64)
        cols = np.ascontiguousarray(cols, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        keep += [rp, cols, vals]
        rps[r], cls[r], vls[r] = rp.ctypes.data, cols.ctypes.data, vals.ctypes.data
    nrow = _ints([len(p[0]) - 1 for p in parts])
    start = _ints([p[3] for p in parts])
    out = (C.c_void_p * P)()
    _check(lib().hpccg_hip_group_create_csr(P, _ints(devices), nrow, start, total_nrow, rps, cls, vls,
                                            out), "group_from_csr")
    return [Matrix(C.c_void_p(out[r])) for r in range(P)]


def group_HPCCG(Ms: list, bs, xs, max_iter: int = 500, tolerance: float = 0.0):
    """HPCCG() over an in-process group; bs[r], xs[r]: rank r's device vectors
    (xs updated in place). Returns (ierr, niters, normr, times)."""
    P = len(Ms)
    hs = _handles(Ms)
    bp = (C.c_void_p * P)(*[_ptr(b) for b in bs])
    xp = (C.c_void_p * P)(*[_ptr(x) for x in xs])
    it = C.c_int(0)
    nr = C.c_double(0.0)
    times = np.zeros(7, np.float64)
    rc = lib().hpccg_hip_group_solve(hs, P, bp, xp, max_iter, tolerance, C.byref(it), C.byref(nr),
                                     times.ctypes.data_as(C.POINTER(C.c_double)))
    _check(rc, "group_HPCCG")
    return rc, it.value, nr.value, times


# ---------------------------------------------------------------------------
# batched solve over an in-process group (include/hpccg_hip_batch_group.h)
# ---------------------------------------------------------------------------
def _group_cols(As, nrhs, lds, what):
    """Per member (pointer, nrhs, ld) of its column set (see _cols); lds: one
    leading dimension for all, one per member, or None."""
    P = len(As)
    if lds is None or isinstance(lds, int):
        lds = [lds] * P
    got = [_cols(a, nrhs, ld, f"{what}[{r}]") for r, (a, ld) in enumerate(zip(As, lds))]
    if len({g[1] for g in got}) > 1:
        raise HPCCGError(f"{what}: the members hold different numbers of columns {[g[1] for g in got]}")
    ptrs = (C.c_void_p * P)(*[g[0] for g in got])
    ld = (C.c_longlong * P)(*[g[2] for g in got])
    return ptrs, (got[0][1] if got else 0), ld


def _handles(Ms):
    return (C.c_void_p * len(Ms))(*[M.h for M in Ms])


def _group_operands(Ms, Bs, Xs, nrhs, ldb, ldx):
    """What every group solve takes first -- the handles, P, nrhs, the column
    sets of B and of X with their leading dimensions -- with the counts of
    column sets and of columns checked."""
    P = len(Ms)
    if len(Bs) != P or len(Xs) != P:
        raise HPCCGError(f"{P} members, {len(Bs)} B and {len(Xs)} X column sets")
    bp, nb, ldb_ = _group_cols(Bs, nrhs, ldb, "Bs")
    xp, nx_, ldx_ = _group_cols(Xs, nrhs, ldx, "Xs")
    if nb != nx_:
        raise HPCCGError(f"Bs holds {nb} columns, Xs {nx_}")
    return _handles(Ms), P, nb, bp, ldb_, xp, ldx_


def _group_call(what, solve, operands, *rest):
    """The call of a group library's solve_device (rest: its arguments between
    ldx and niters) and the result (niters[nrhs], normr[nrhs], times)."""
    nb = operands[2]
    it = np.zeros(max(nb, 1), np.int32)
    nr = np.zeros(max(nb, 1), np.float64)
    times = np.zeros(7, np.float64)
    rc = solve(*operands, *rest, it.ctypes.data_as(C.POINTER(C.c_int)), nr.ctypes.data_as(C.POINTER(C.c_double)),
               times.ctypes.data_as(C.POINTER(C.c_double)))
    _check(rc, what)
    return it[:nb], nr[:nb], times


def _group_minvs(Ms, minvs):
    """The array of the members' device m pointers (None: Jacobi)."""
    if minvs is None:
        return None
    P = len(Ms)
    if len(minvs) != P:
        raise HPCCGError(f"{P} members, {len(minvs)} minv vectors")
    ptrs = []
    for r, (M, m) in enumerate(zip(Ms, minvs)):
        nrow = int(M.info()["nrow"])
        if not isinstance(m, int) and (m.dim() != 1 or m.shape[0] < nrow or (m.shape[0] > 1 and m.stride(0) != 1)):
            raise HPCCGError(f"minvs[{r}]: a contiguous 1-D tensor of {nrow} entries")
        ptrs.append(_ptr(m))
    return (C.c_void_p * P)(*ptrs)


class _halo_copies_env:
    """A library's halo-by-copies switch set (or cleared) for one call."""

    def __init__(self, on, name):
        self.on = on
        self.name = name

    def __enter__(self):
        self.saved = os.environ.pop(self.name, None)
        if self.on:
            os.environ[self.name] = "1"

    def __exit__(self, *exc):
        os.environ.pop(self.name, None)
        if self.saved is not None:
            os.environ[self.name] = self.saved


def _group_solve(what, solve, env, Ms, Bs, Xs, minvs, nrhs, ldb, ldx, halo_copies, *rest):
    """What the preconditioned group solves share: _group_operands, the
    members' minvs, the library's halo-by-copies switch env around the call of
    solve (rest: its arguments between minv and niters) and the result
    (niters[nrhs], normr[nrhs], times)."""
    operands = _group_operands(Ms, Bs, Xs, nrhs, ldb, ldx)
    mp = _group_minvs(Ms, minvs)
    with _halo_copies_env(halo_copies, env):
        return _group_call(what, solve, operands, mp, *rest)


def _group_last_trace(what, last_trace, Ms, col, cap):
    out = np.zeros(cap, np.float64)
    n = last_trace(_handles(Ms), len(Ms), int(col), out.ctypes.data_as(C.POINTER(C.c_double)), cap)
    if n < 0:
        _check(n, what)
    return out[:n]


def _group_bound(what, bound, Ms, minvs):
    v = C.c_double(0.0)
    _check(bound(_handles(Ms), len(Ms), _group_minvs(Ms, minvs), C.byref(v)), what)
    return v.value


def _group_last_spectrum(what, last_spectrum, Ms):
    lo, hi = C.c_double(0.0), C.c_double(0.0)
    _check(last_spectrum(_handles(Ms), len(Ms), C.byref(lo), C.byref(hi)), what)
    return lo.value, hi.value


def group_HPCCG_batch(Ms: list, Bs, Xs, max_iter: int = 500, tolerance: float = 0.0, nrhs=None, ldb=None,
                      ldx=None):
    """nrhs CG solves over an in-process group in one pass over the matrix per
    iteration (hpccg_hip_group_batch_solve_device); column c is bitwise
    group_HPCCG of that column alone. Bs[r], Xs[r]: member r's rows of every
    column on its device, shape (nrhs, ld) with row c holding column c
    (ld >= the member's nrow) -- tensors, or device pointers with nrhs and the
    leading dimensions. Xs is updated in place. Returns
    (niters[nrhs], normr[nrhs], times)."""
    solve = batch_lib().hpccg_hip_group_batch_solve_device
    return _group_call("group_HPCCG_batch", solve, _group_operands(Ms, Bs, Xs, nrhs, ldb, ldx), max_iter, tolerance)


def group_sparsemv_batch(Ms: list, Xs, Ys, nrhs=None, ldx=None, ldy=None) -> int:
    """Ys[r][c] = member r's rows of A Xs[:][c] for every column (the global
    matrix; the halo of X is exchanged inside)."""
    P = len(Ms)
    if len(Xs) != P or len(Ys) != P:
        raise HPCCGError(f"{P} members, {len(Xs)} X and {len(Ys)} Y column sets")
    hs = _handles(Ms)
    xp, nx_, ldx_ = _group_cols(Xs, nrhs, ldx, "Xs")
    yp, ny_, ldy_ = _group_cols(Ys, nrhs, ldy, "Ys")
    if nx_ != ny_:
        raise HPCCGError(f"Xs holds {nx_} columns, Ys {ny_}")
    _check(batch_lib().hpccg_hip_group_batch_sparsemv(hs, P, nx_, xp, ldx_, yp, ldy_), "group_sparsemv_batch")
    return 0


def group_last_trace_batch(Ms: list, col: int, cap: int = 100000) -> np.ndarray:
    """Residual trace of column col of the last group_HPCCG_batch on Ms."""
    return _group_last_trace("group_last_trace_batch", batch_lib().hpccg_hip_group_batch_last_trace, Ms, col, cap)


# ---------------------------------------------------------------------------
# preconditioned solve over an in-process group (include/hpccg_hip_pcg_group.h)
# ---------------------------------------------------------------------------

def group_HPCCG_pcg(Ms: list, Bs, Xs, max_iter: int = 500, tolerance: float = 0.0, minvs=None, nrhs=None, ldb=None,
                    ldx=None, halo_copies: bool = False):
    """nrhs preconditioned CG solves over an in-process group with
    M^-1 = diag(minv) (hpccg_hip_group_pcg_solve_device); minvs None is Jacobi,
    1 / a_ii of every member's own rows, else minvs[r] is member r's nrow
    entries (a contiguous 1-D device tensor or a device pointer), all finite
    and > 0. The loop test, niters and normr are on the 2-norm of r, as in
    group_HPCCG. Bs[r], Xs[r]: as group_HPCCG_batch (shape (nrhs, ld), row c
    holding column c). Xs is updated in place. halo_copies (diagnostic): move
    the ghost planes by one copy per column and side, as the group batch does,
    instead of one kernel launch per member; the bits are the same. Returns
    (niters[nrhs], normr[nrhs], times)."""
    return _group_solve("group_HPCCG_pcg", pcg_group_lib().hpccg_hip_group_pcg_solve_device,
                        "HPCCG_GROUP_PCG_HALO_COPIES", Ms, Bs, Xs, minvs, nrhs, ldb, ldx, halo_copies, max_iter,
                        tolerance)


def group_pcg_diagonal(Ms: list) -> list:
    """Per member the diagonal of its rows as the group preconditioned solve
    reads it from the member's device image (0.0 where a row stores none)."""
    import torch
    P = len(Ms)
    hs = _handles(Ms)
    ns = [int(M.info()["nrow"]) for M in Ms]
    ds = [torch.zeros(max(n, 1), dtype=torch.float64, device="cuda") for n in ns]
    dp = (C.c_void_p * P)(*[_ptr(d) for d in ds])
    _check(pcg_group_lib().hpccg_hip_group_pcg_diagonal(hs, P, dp), "group_pcg_diagonal")
    return [d.cpu().numpy()[:n].copy() for d, n in zip(ds, ns)]


def group_last_trace_pcg(Ms: list, col: int, cap: int = 100000) -> np.ndarray:
    """Residual trace (norm of r) of column col of the last group_HPCCG_pcg on Ms."""
    return _group_last_trace("group_last_trace_pcg", pcg_group_lib().hpccg_hip_group_pcg_last_trace, Ms, col, cap)


def group_pcg_workspace_bytes(M: Matrix) -> int:
    """Device bytes member M's group pcg workspace holds (0: none)."""
    return _workspace_bytes("pcg_group", "group_pcg_workspace_bytes", M.h)


def group_pcg_release(M: Matrix) -> None:
    """Free member M's group pcg workspace (with its cached 1 / a_ii) now (close() does it too)."""
    _release("pcg_group", "group_pcg_release", M.h)


def group_pcg_live_workspaces() -> int:
    """Matrices that hold a group pcg workspace (0 when the library was never loaded)."""
    return _live("pcg_group", "group_pcg_live_workspaces")


# ---------------------------------------------------------------------------
# polynomial preconditioned solve over an in-process group (include/hpccg_hip_poly_group.h)
# ---------------------------------------------------------------------------
def group_HPCCG_poly(Ms: list, Bs, Xs, degree: int = 2, lmin=None, lmax=None, minvs=None, max_iter: int = 500,
                     tolerance: float = 0.0, nrhs=None, ldb=None, ldx=None, halo_copies: bool = False):
    """nrhs CG solves over an in-process group preconditioned by the Chebyshev
    polynomial of `degree` steps in diag(minv) A on [lmin, lmax]
    (hpccg_hip_group_poly_solve_device); minvs None is Jacobi, lmax None the
    symmetric Gershgorin bound of the global matrix, lmin None lmax / 30. Degree
    0 is group_HPCCG_pcg bit for bit; a group of one is HPCCG_poly bit for bit.
    Bs, Xs, minvs: as group_HPCCG_pcg. Xs is updated in place. halo_copies
    (diagnostic): move every ghost plane of z and p by one copy per column and
    side instead of one kernel launch per member; the bits are the same.
    Returns (niters[nrhs], normr[nrhs], times)."""
    return _group_solve("group_HPCCG_poly", poly_group_lib().hpccg_hip_group_poly_solve_device,
                        "HPCCG_GROUP_POLY_HALO_COPIES", Ms, Bs, Xs, minvs, nrhs, ldb, ldx, halo_copies,
                        *_interval(degree, lmin, lmax), max_iter, tolerance)


def group_poly_bound(Ms: list, minvs=None) -> float:
    """The symmetric Gershgorin bound of the group's global matrix that
    group_HPCCG_poly takes for lmax; minvs: per member a device tensor / pointer
    of its nrow entries, or None for Jacobi."""
    return _group_bound("group_poly_bound", poly_group_lib().hpccg_hip_group_poly_bound, Ms, minvs)


def group_last_trace_poly(Ms: list, col: int, cap: int = 100000) -> np.ndarray:
    """Residual trace (norm of r) of column col of the last group_HPCCG_poly on Ms."""
    return _group_last_trace("group_last_trace_poly", poly_group_lib().hpccg_hip_group_poly_last_trace, Ms, col, cap)


def group_last_spectrum_poly(Ms: list) -> tuple:
    """(lmin, lmax) the last group_HPCCG_poly on Ms used."""
    return _group_last_spectrum("group_last_spectrum_poly", poly_group_lib().hpccg_hip_group_poly_last_spectrum, Ms)


def group_poly_workspace_bytes(M: Matrix) -> int:
    """Device bytes member M's group poly workspace holds (0: none)."""
    return _workspace_bytes("poly_group", "group_poly_workspace_bytes", M.h)


def group_poly_release(M: Matrix) -> None:
    """Free member M's group poly workspace (with its caches) now (close() does it too)."""
    _release("poly_group", "group_poly_release", M.h)


def group_poly_live_workspaces() -> int:
    """Matrices that hold a group poly workspace (0 when the library was never loaded)."""
    return _live("poly_group", "group_poly_live_workspaces")


# ---------------------------------------------------------------------------
# ... with the steps streamed from the members' fp32 images (include/hpccg_hip_poly32_group.h)
# ---------------------------------------------------------------------------
def group_HPCCG_poly32(Ms: list, Bs, Xs, degree: int = 2, lmin=None, lmax=None, minvs=None, max_iter: int = 500,
                       tolerance: float = 0.0, nrhs=None, ldb=None, ldx=None, halo_copies: bool = False):
    """group_HPCCG_poly with every member's polynomial steps streamed from an
    fp32 image of its rows (hpccg_hip_group_poly32_solve_device); the system
    solved is the fp64 one. Where every member's image is exact
    (group_poly32_info) every column is group_HPCCG_poly bit for bit; degree 0 is
    group_HPCCG_pcg bit for bit on any matrix; a group of one is HPCCG_poly32 bit
    for bit. The arguments and the result are group_HPCCG_poly's."""
    return _group_solve("group_HPCCG_poly32", poly32_group_lib().hpccg_hip_group_poly32_solve_device,
                        "HPCCG_GROUP_POLY32_HALO_COPIES", Ms, Bs, Xs, minvs, nrhs, ldb, ldx, halo_copies,
                        *_interval(degree, lmin, lmax), max_iter, tolerance)


def group_poly32_bound(Ms: list, minvs=None) -> float:
    """The symmetric Gershgorin bound of the group's global fp64 matrix that
    group_HPCCG_poly32 takes for lmax (group_poly_bound's value); minvs: per
    member a device tensor / pointer of its nrow entries, or None for Jacobi."""
    return _group_bound("group_poly32_bound", poly32_group_lib().hpccg_hip_group_poly32_bound, Ms, minvs)


def group_poly32_info(Ms: list) -> list:
    """The members' fp32 images of the group poly32 library (built on first
    use), one dict per member: exact (every value of the member's rows survives
    double -> float -> double), image_bytes, inexact_values."""
    P = len(Ms)
    hs = _handles(Ms)
    a = (C.c_longlong * (4 * P))()
    _check(poly32_group_lib().hpccg_hip_group_poly32_info(hs, P, a), "group_poly32_info")
    return [{"exact": int(a[4 * r]),"image_bytes": int(a[4 * r + 1]), "inexact_values": int(a[4 * r + 2])}
            for r in range(P)]


def group_last_trace_poly32(Ms: list, col: int, cap: int = 100000) -> np.ndarray:
    """Residual trace (norm of r) of column col of the last group_HPCCG_poly32 on Ms."""
    return _group_last_trace("group_last_trace_poly32", poly32_group_lib().hpccg_hip_group_poly32_last_trace, Ms, col,
                             cap)


def group_last_spectrum_poly32(Ms: list) -> tuple:
    """(lmin, lmax) the last group_HPCCG_poly32 on Ms used."""
    return _group_last_spectrum("group_last_spectrum_poly32", poly32_group_lib().hpccg_hip_group_poly32_last_spectrum,
                                Ms)


def group_poly32_workspace_bytes(M: Matrix) -> int:
    """Device bytes member M's group poly32 workspace holds, its fp32 image included (0: none)."""
    return _workspace_bytes("poly32_group", "group_poly32_workspace_bytes", M.h)


def group_poly32_release(M: Matrix) -> None:
    """Free member M's group poly32 workspace (with its caches and its fp32 image) now (close() does it too)."""
    _release("poly32_group", "group_poly32_release", M.h)


def group_poly32_live_workspaces() -> int:
    """Matrices that hold a group poly32 workspace (0 when the library was never loaded)."""
    return _live("poly32_group", "group_poly32_live_workspaces")


# ---------------------------------------------------------------------------
# single-reduction preconditioned solve over an in-process group (include/hpccg_hip_srcg_group.h)
# ---------------------------------------------------------------------------
def group_HPCCG_srcg(Ms: list, Bs, Xs, max_iter: int = 500, tolerance: float = 0.0, minvs=None, nrhs=None, ldb=None,
                     ldx=None, halo_copies: bool = False):
    """nrhs single-reduction preconditioned CG solves over an in-process group
    with M^-1 = diag(minv) (hpccg_hip_group_srcg_solve_device): group_HPCCG_pcg's
    method with one sum over the members per iteration instead of two. The
    first iteration (max_iter <= 2) is group_HPCCG_pcg bit for bit; a group of
    one is HPCCG_srcg bit for bit. Ms, Bs, Xs, minvs: as group_HPCCG_pcg. Xs is
    updated in place. halo_copies (diagnostic): move the ghost planes of u by
    one copy per column and side instead of one kernel launch per member; the
    bits are the same. Returns (niters[nrhs], normr[nrhs], times)."""
    return _group_solve("group_HPCCG_srcg", srcg_group_lib().hpccg_hip_group_srcg_solve_device,
                        "HPCCG_GROUP_SRCG_HALO_COPIES", Ms, Bs, Xs, minvs, nrhs, ldb, ldx, halo_copies, max_iter,
                        tolerance)


def group_last_trace_srcg(Ms: list, col: int, cap: int = 100000) -> np.ndarray:
    """Residual trace (norm of r) of column col of the last group_HPCCG_srcg on Ms."""
    return _group_last_trace("group_last_trace_srcg", srcg_group_lib().hpccg_hip_group_srcg_last_trace, Ms, col, cap)


def group_srcg_workspace_bytes(M: Matrix) -> int:
    """Device bytes member M's group srcg workspace holds (0: none)."""
    return _workspace_bytes("srcg_group", "group_srcg_workspace_bytes", M.h)


def group_srcg_release(M: Matrix) -> None:
    """Free member M's group srcg workspace (with its cached 1 / a_ii) now (close() does it too)."""
    _release("srcg_group", "group_srcg_release", M.h)


def group_srcg_live_workspaces() -> int:
    """Matrices that hold a group srcg workspace (0 when the library was never loaded)."""
    return _live("srcg_group", "group_srcg_live_workspaces")


# ---------------------------------------------------------------------------
# ... with the polynomial preconditioner (include/hpccg_hip_srpoly_group.h)
# ---------------------------------------------------------------------------
def group_HPCCG_srpoly(Ms: list, Bs, Xs, degree: int = 2, lmin=None, lmax=None, minvs=None, max_iter: int = 500,
                       tolerance: float = 0.0, nrhs=None, ldb=None, ldx=None, halo_copies: bool = False):
    """group_HPCCG_poly in the single-reduction form
    (hpccg_hip_group_srpoly_solve_device): degree + 1 halos per iteration, as
    there, and one sum over the members instead of two. Degree 0 is
    group_HPCCG_srcg bit for bit; the first iteration (max_iter <= 2) is
    group_HPCCG_poly bit for bit; a group of one is HPCCG_srpoly bit for bit.
    The arguments and the result are group_HPCCG_poly's. halo_copies
    (diagnostic): move every ghost plane of z and u by one copy per column and
    side instead of one kernel launch per member; the bits are the same."""
    return _group_solve("group_HPCCG_srpoly", srpoly_group_lib().hpccg_hip_group_srpoly_solve_device,
                        "HPCCG_GROUP_SRPOLY_HALO_COPIES", Ms, Bs, Xs, minvs, nrhs, ldb, ldx, halo_copies,
                        *_interval(degree, lmin, lmax), max_iter, tolerance)


def group_srpoly_bound(Ms: list, minvs=None) -> float:
    """The symmetric Gershgorin bound of the group's global matrix that
    group_HPCCG_srpoly takes for lmax (group_poly_bound's value); minvs: per
    member a device tensor / pointer of its nrow entries, or None for Jacobi."""
    return _group_bound("group_srpoly_bound", srpoly_group_lib().hpccg_hip_group_srpoly_bound, Ms, minvs)


def group_last_trace_srpoly(Ms: list, col: int, cap: int = 100000) -> np.ndarray:
    """Residual trace (norm of r) of column col of the last group_HPCCG_srpoly on Ms."""
    return _group_last_trace("group_last_trace_srpoly", srpoly_group_lib().hpccg_hip_group_srpoly_last_trace, Ms, col,
                             cap)


def group_last_spectrum_srpoly(Ms: list) -> tuple:
    """(lmin, lmax) the last group_HPCCG_srpoly on Ms used."""
    return _group_last_spectrum("group_last_spectrum_srpoly", srpoly_group_lib().hpccg_hip_group_srpoly_last_spectrum,
                                Ms)


def group_srpoly_workspace_bytes(M: Matrix) -> int:
    """Device bytes member M's group srpoly workspace holds (0: none)."""
    return _workspace_bytes("srpoly_group", "group_srpoly_workspace_bytes", M.h)


def group_srpoly_release(M: Matrix) -> None:
    """Free member M's group srpoly workspace (with its caches) now (close() does it too)."""
    _release("srpoly_group", "group_srpoly_release", M.h)


def group_srpoly_live_workspaces() -> int:
    """Matrices that hold a group srpoly workspace (0 when the library was never loaded)."""
    return _live("srpoly_group", "group_srpoly_live_workspaces")


def HPC_sparsemv(M: Matrix, x, y) -> int:
    _check(lib().hpccg_hip_sparsemv(M.h, _ptr(x), _ptr(y)), "HPC_sparsemv")
    return 0


def ddot(n: int, x, y) -> float:
    r = C.c_double(0.0)
    _check(lib().hpccg_hip_ddot(n, _ptr(x), _ptr(y), C.byref(r)), "ddot")
    return r.value


def waxpby(n: int, alpha: float, x, beta: float, y, w) -> int:
    _check(lib().hpccg_hip_waxpby(n, alpha, _ptr(x), beta, _ptr(y), _ptr(w)), "waxpby")
    return 0


def device_count() -> int:
    c = C.c_int(0)
    lib().hpccg_hip_device_count(C.byref(c))
    return c.value


def set_device(d: int) -> None:
    _check(lib().hpccg_hip_set_device(d), "set_device")


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(lib().hpccg_hip_comm_unique_id(buf), "comm_unique_id")
    return buf.raw


def comm_init(uid: bytes, nranks: int, rank: int) -> None:
    _check(lib().hpccg_hip_comm_init(uid, nranks, rank), "comm_init")


def comm_allreduce_host(vals, op: str = "sum") -> np.ndarray:
    """All-reduce a few host doubles over the RCCL communicator (sum/min/max)."""
    a = np.ascontiguousarray(vals, np.float64).copy()
    _check(lib().hpccg_hip_comm_allreduce_host(a.ctypes.data_as(C.POINTER(C.c_double)), len(a),
                                               {"sum": 0, "min": 1, "max": 2}[op]),
           "comm_allreduce_host")
    return a


def transport_verdict(local) -> list:
    """The job's in-kernel transport verdicts [peer all-reduce, halo pull,
    protocol] from this rank's own self-test results (collective over the
    communicator; what matrix creation decides with)."""
    a = (C.c_int * 3)(*[int(bool(v)) for v in local])
    out = (C.c_int * 3)()
    _check(lib().hpccg_hip_transport_verdict(a, out), "transport_verdict")
    return list(out)


def torch_allgather(data: bytes) -> list:
    """Every rank's `data` (same length everywhere) in rank order over the
    default torch.distributed group (gloo in this package's launchers)."""
    import torch
    import torch.distributed as dist
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    outs = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(outs, t)
    return [o.numpy().tobytes() for o in outs]


def comm_init_host(nranks: int, rank: int, allgather=None) -> None:
    """Host-bootstrapped communicator (hpccg_hip_comm_init_host): the setup
    exchanges go through allgather(bytes) -> [bytes of every rank] (default:
    torch.distributed's default group), no RCCL; the CG iteration runs the
    in-kernel peer all-reduce and the halo pull. Several ranks may share a GPU."""
    global _host_allgather
    ag = allgather or torch_allgather

    def cb(send, recv, nbytes, ctx):
        try:
            n = int(nbytes)
            parts = ag(C.string_at(send, n))
            if len(parts) != nranks:
                return 1
            for q, part in enumerate(parts):
                if len(part) != n:
                    return 1
                C.memmove(recv + q * n, part, n)
            return 0
        except BaseException:  # reported, and the library sees a failed exchange
            import traceback
            traceback.print_exc()
            return 1

    fn = ALLGATHER_FN(cb)
    _check(lib().hpccg_hip_comm_init_host(nranks, rank, fn, None), "comm_init_host")
    _host_allgather = fn


def comm_mode() -> str:
    """'none' (one rank), 'rccl' or 'host' (hpccg_hip_comm_init_host)."""
    m = C.c_int(0)
    _check(lib().hpccg_hip_comm_mode(C.byref(m)), "comm_mode")
    return {0: "none", 1: "rccl", 2: "host"}[m.value]


def canary_check() -> tuple:
    """(enabled, tripped canaries, report) -- canary mode is HPCCG_CANARY=1
    when the library first allocates (hpccg_hip_diag_canary_check)."""
    en = C.c_int(0)
    buf = C.create_string_buffer(4096)
    n = lib().hpccg_hip_diag_canary_check(C.byref(en), buf, 4096)
    return bool(en.value), n, buf.value.decode(errors="replace")


def comm_destroy() -> None:
    global _host_allgather
    lib().hpccg_hip_comm_destroy()
    _host_allgather = None


def runtime_info() -> dict:
    """What this process runs on: RCCL's own rank count (ncclCommCount) and
    rank, RCCL / HIP versions, the device's PCI bus id, and the shared objects
    the library's RCCL and HIP symbols resolved to."""
    ints = (C.c_int * 6)()
    pci = C.create_string_buffer(64)
    rccl, hip = C.create_string_buffer(512), C.create_string_buffer(512)
    _check(lib().hpccg_hip_runtime_info(ints, pci, 64, rccl, hip, 512), "runtime_info")
    v = ints[2]
    return {"rccl_nranks": ints[0], "rccl_rank": ints[1],
            "rccl_version": f"{v // 10000}.{v // 100 % 100}.{v % 100}" if v >= 10000 else str(v),
            "hip_runtime_version": ints[3], "hip_driver_version": ints[4], "device": ints[5],
            "pci_bus_id": pci.value.decode(), "rccl_lib": rccl.value.decode(), "hip_lib": hip.value.decode()}


def device_name() -> tuple[str, int]:
    buf = C.create_string_buffer(256)
    cus = C.c_int(0)
    _check(lib().hpccg_hip_device_name(buf, 256, C.byref(cus)), "device_name")
    return buf.value.decode(), cus.value


# ---------------------------------------------------------------------------
# host-only helpers (no GPU)
# ---------------------------------------------------------------------------
SLICE_ROWS = 512


def sell_build(row_ptr, cols, vals, col_base=0, ncol_ext=None):
    """SELL-512 image the device uses: (slice_base, sell_cols, sell_vals)."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int64)
    cols = np.ascontiguousarray(cols, np.int32)
    vals = np.ascontiguousarray(vals, np.float64)
    n = len(row_ptr) - 1
    ncol_ext = n if ncol_ext is None else ncol_ext
    ns = (n + SLICE_ROWS - 1) // SLICE_ROWS
    sb = np.zeros(ns + 1, np.uint32)
    L = lib()
    slots = L.hpccg_sell_build(n, col_base, ncol_ext, row_ptr.ctypes.data, cols.ctypes.data,
                               vals.ctypes.data, sb.ctypes.data, None, None)
    sc = np.zeros(max(int(slots), 1), np.int32)
    sv = np.zeros(max(int(slots), 1), np.float64)
    r = L.hpccg_sell_build(n, col_base, ncol_ext, row_ptr.ctypes.data, cols.ctypes.data,
                           vals.ctypes.data, sb.ctypes.data, sc.ctypes.data, sv.ctypes.data)
    if r < 0:
        raise HPCCGError("sell_build: column outside the halo plan")
    return sb, sc[:slots], sv[:slots]


def slot_plan(units: int, grid: int, spu: int = 1, rev: bool = False):
    """The folded dot completion's plan for one launch shape (host only): per
    group of 64 slices the unit whose block waits for the group, and the top
    group (hpccg_hip_diag_slot_plan)."""
    cap = (units * spu + 63) // 64
    out = (C.c_int * max(cap, 1))()
    top = C.c_int(-1)
    n = lib().hpccg_hip_diag_slot_plan(units, grid, spu, int(rev), out, cap, C.byref(top))
    _check(n if n < 0 else 0, "diag_slot_plan")
    return list(out[:n]), top.value


def halo_plan(row_ptr, cols, start_row, total_nrow):
    row_ptr = np.ascontiguousarray(row_ptr, np.int64)
    cols = np.ascontiguousarray(cols, np.int32)
    out = (C.c_int * 4)()
    _check(lib().hpccg_halo_plan(len(row_ptr) - 1, start_row, total_nrow, row_ptr.ctypes.data,
                                 cols.ctypes.data, out), "halo_plan")
    return {"ghost_lo": out[0], "ghost_hi": out[1], "min_col": out[2], "max_col": out[3]}


def gather_plan(nranks: int, info, row_ptr, cols, start_row: int) -> dict:
    """Local half of the gather plan: external columns in local order and the
    receive runs per owner (make_local_matrix.cpp:96-200)."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int64)
    cols = np.ascontiguousarray(cols, np.int32)
    arr = (C.c_int * (4 * nranks))(*[int(v) for v in np.asarray(info).ravel()])
    ne, nr = C.c_int(0), C.c_int(0)
    L = lib()
    n = len(row_ptr) - 1
    _check(L.hpccg_gather_plan(nranks, arr, n, start_row, row_ptr.ctypes.data, cols.ctypes.data, 0, None,
                               C.byref(ne), C.byref(nr), None, None, None), "gather_plan")
    cap = max(ne.value, nr.value, 1)
    ext = (C.c_int * cap)()
    rr, ro, rc = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
    _check(L.hpccg_gather_plan(nranks, arr, n, start_row, row_ptr.ctypes.data, cols.ctypes.data, cap, ext,
                               C.byref(ne), C.byref(nr), rr, ro, rc), "gather_plan")
    return {"ext_global": np.array(ext[:ne.value], np.int64),
            "recv": [(rr[i], ro[i], rc[i]) for i in range(nr.value)]}


def slab_plan(nranks: int, rank: int, info) -> tuple[int, int]:
    """(rows sent to rank-1, rows sent to rank+1) from all ranks' 4-int info."""
    arr = (C.c_int * (4 * nranks))(*[int(v) for v in np.asarray(info).ravel()])
    out = (C.c_int * 2)()
    _check(lib().hpccg_slab_plan(nranks, rank, arr, out), "slab_plan")
    return out[0], out[1]


def load():
    """Return this module (for callers that import the package by path)."""
    import sys
    return sys.modules[__name__]
