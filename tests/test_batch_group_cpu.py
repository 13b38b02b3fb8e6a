"""CPU-only checks of the group batch interface (include/hpccg_hip_batch_group.h,
implemented in lib/libhpccg_hip_batch.so): the batch library exports what the
new header declares and the main library none of it, the old batch header and
the main ABI are unchanged, and bad arguments are refused before HIP is
touched, with hpccg_hip_last_error() naming the argument.
"""
import ctypes as C
import os
import subprocess

EINVAL = -1


def test_batch_library_exports_the_group_functions(hp):
    declared = hp.group_batch_exported_symbols()
    assert declared == ["hpccg_hip_group_batch_abi_version", "hpccg_hip_group_batch_last_trace",
                        "hpccg_hip_group_batch_solve_device", "hpccg_hip_group_batch_sparsemv"]
    out = subprocess.run(["nm", "-D", "--defined-only", hp.BATCH_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    L = hp.batch_lib()
    for s in declared:
        assert hasattr(L, s), s
    main = subprocess.run(["nm", "-D", "--defined-only", hp.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    assert "hpccg_hip_group_batch" not in main
    assert "group_batch" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    # the old header keeps its eight functions, none of them the new ones
    old = hp.batch_exported_symbols()
    assert len(old) == 8 and not set(old) & set(declared)


def test_abi_version(hp):
    assert hp.batch_lib().hpccg_hip_group_batch_abi_version() == 1
    assert hp.batch_lib().hpccg_hip_batch_abi_version() == 1
    assert hp.lib().hpccg_hip_abi_version() == 2


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.batch_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    # never dereferenced: these argument checks come before the members are looked at
    Ms = (C.c_void_p * 17)(*([p] * 17))
    cols = (C.c_void_p * 17)(*([p] * 17))
    ld = (C.c_longlong * 17)(*([4] * 17))

    def solve(ms=Ms, nranks=2, nrhs=2, max_iter=10):
        return L.hpccg_hip_group_batch_solve_device(ms, nranks, nrhs, cols, ld, cols, ld, max_iter, 0.0, it, nr, None)

    def spmv(ms=Ms, nranks=2, nrhs=2):
        return L.hpccg_hip_group_batch_sparsemv(ms, nranks, nrhs, cols, ld, cols, ld)

    assert solve(ms=None) == EINVAL
    assert b"Ms" in err() and b"NULL" in err()
    assert spmv(ms=None) == EINVAL
    assert b"Ms" in err()
    assert L.hpccg_hip_group_batch_last_trace(None, 2, 0, buf, 8) == EINVAL
    assert b"Ms" in err()
    for nranks in (0, 17):
        assert solve(nranks=nranks) == EINVAL
        assert b"nranks" in err()
        assert spmv(nranks=nranks) == EINVAL
        assert b"nranks" in err()
        assert L.hpccg_hip_group_batch_last_trace(Ms, nranks, 0, buf, 8) == EINVAL
        assert b"nranks" in err()
    for nrhs in (0, -3):
        assert solve(nrhs=nrhs) == EINVAL
        assert b"nrhs" in err()
        assert spmv(nrhs=nrhs) == EINVAL
        assert b"nrhs" in err()
    assert solve(max_iter=-1) == EINVAL
    assert b"max_iter" in err()
    # NULL members and NULL column tables, still without a device
    null_ms = (C.c_void_p * 2)(None, None)
    assert solve(ms=null_ms) == EINVAL
    assert b"Ms[0]" in err()
    assert L.hpccg_hip_group_batch_solve_device(Ms, 2, 2, None, ld, cols, ld, 10, 0.0, it, nr, None) == EINVAL
    assert b"NULL" in err()
    assert hp.batch_live_workspaces() == 0
