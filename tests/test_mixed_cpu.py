"""CPU-only checks of the mixed-precision library (lib/libhpccg_hip_mixed.so,
include/hpccg_hip_mixed.h): it is built beside the main library, exports what
its header declares, refuses bad arguments before touching HIP, and its
kernels keep their budget (read from its gfx950 code object): no spills,
scratch <= 32 B, the SpMM kernels <= 128 VGPRs, the light kernels <= 64. The
main library knows nothing of it.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes

EINVAL = -1


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.MIXED_LIB_PATH), "run build(): libhpccg_hip_mixed.so is missing"
    declared = hp.mixed_exported_symbols()
    assert len(declared) == 10, declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.MIXED_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    L = hp.mixed_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the mixed entry points live in the third library only
    assert "hpccg_hip_mixed" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    main = subprocess.run(["nm", "-D", "--defined-only", hp.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    assert "hpccg_hip_mixed" not in main


def test_abi_version(hp):
    assert hp.mixed_lib().hpccg_hip_mixed_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.MIXED_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.mixed_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    ib = (C.c_int * 8)()
    ll = (C.c_longlong * 4)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first

    def solve(f, h=fake, nrhs=2, b=p, x=p, max_iter=10, sweeps=8, rtol=-1.0, its=it, nrs=nr):
        return f(h, nrhs, b, 4, x, 4, max_iter, 0.0, sweeps, rtol, its, nrs, None)

    for f in (L.hpccg_hip_mixed_solve_device, L.hpccg_hip_mixed_solve):
        for kw in (dict(h=None), dict(b=None), dict(x=None), dict(its=None), dict(nrs=None)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"NULL" in err()
        for nrhs in (0, -3):
            assert solve(f, nrhs=nrhs) == EINVAL
            assert b"nrhs" in err()
        assert solve(f, max_iter=-1) == EINVAL
        assert b"max_iter" in err()
        for sweeps in (0, -2):
            assert solve(f, sweeps=sweeps) == EINVAL
            assert b"max_sweeps" in err()
        for rtol in (1.0, 2.5, float("nan")):
            assert solve(f, rtol=rtol) == EINVAL
            assert b"inner_rtol" in err()
    assert L.hpccg_hip_mixed_sparsemv(None, 2, p, 4, p, 4) == EINVAL
    assert L.hpccg_hip_mixed_sparsemv(fake, 2, None, 4, p, 4) == EINVAL
    for nrhs in (0, -3):
        assert L.hpccg_hip_mixed_sparsemv(fake, nrhs, p, 4, p, 4) == EINVAL
        assert b"nrhs" in err()
    assert L.hpccg_hip_mixed_info(None, ll) == EINVAL
    assert L.hpccg_hip_mixed_info(fake, None) == EINVAL
    assert L.hpccg_hip_mixed_release(None) == EINVAL
    assert L.hpccg_hip_mixed_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_mixed_last_trace(fake, 0, buf, 8) == EINVAL  # (no solve ran on it: the records are searched only)
    assert b"no trace" in err()
    assert L.hpccg_hip_mixed_last_sweeps(None, 0, ib, buf, 8) == EINVAL
    assert L.hpccg_hip_mixed_last_sweeps(fake, 0, ib, buf, 8) == EINVAL
    assert L.hpccg_hip_mixed_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_mixed_workspace_bytes(fake, ll) == 0 and ll[0] == 0
    assert L.hpccg_hip_mixed_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_mixed_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.mixed_live_workspaces() == 0


def test_a_strided_one_column_is_refused(hp):
    """A 1-D B or X is one column through a view; a strided one would be solved in a copy."""
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_mixed(None, np.zeros(8), np.zeros(16)[::2])
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_mixed(None, np.zeros(16)[::2], np.zeros(8))


def test_kernel_budgets(hp):
    ks = _kernels(hp.MIXED_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_mixed_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    spmm = {n: r for n, r in ks.items() if "k_mixed_spmm_" in n}
    # widths 27, 7 and per-slice; one, two and four columns each; the int32-column form likewise;
    # each with plain and with non-temporal value loads (a template parameter: chosen on the host)
    frags = [f"k_mixed_spmm_a<{w}, {nt}, {r}>" for w in (27, 7, 0) for nt in ("false", "true") for r in (1, 2, 4)]
    frags += [f"k_mixed_spmm_sell<{nt}, {r}>" for nt in ("false", "true") for r in (1, 2, 4)]
    for frag in frags:
        assert any(frag in n for n in spmm), frag
    assert len(spmm) == len(frags), sorted(spmm)
    for n, r in spmm.items():
        assert r["vgpr_count"] <= 128, (n, r)
    light = {n: r for n, r in ks.items() if n not in spmm}
    for frag in ["k_mixed_convert", "k_mixed_residual", "k_mixed_finalize"] + \
            [f"k_mixed_{k}<{r}>" for k in ("p", "update") for r in (1, 2, 4)]:
        assert any(frag in n for n in light), frag
    assert len(light) == 9, sorted(light)
    for n, r in light.items():
        assert r["vgpr_count"] <= 64, (n, r)
