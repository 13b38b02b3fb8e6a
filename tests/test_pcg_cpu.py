"""CPU-only checks of the preconditioned-CG library (lib/libhpccg_hip_pcg.so,
include/hpccg_hip_pcg.h): it is built beside the main library, exports what
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
    assert os.path.exists(hp.PCG_LIB_PATH), "run build(): libhpccg_hip_pcg.so is missing"
    declared = hp.pcg_exported_symbols()
    assert declared == sorted("hpccg_hip_pcg_" + s for s in (
        "abi_version", "solve_device", "solve", "diagonal", "last_trace", "release", "workspace_bytes",
        "live_workspaces")), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.PCG_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the eight
    L = hp.pcg_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the fourth library only
    assert "hpccg_hip_pcg" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    for other in (hp.LIB_PATH, hp.BATCH_LIB_PATH, hp.MIXED_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "hpccg_hip_pcg" not in syms, other


def test_abi_version(hp):
    assert hp.pcg_lib().hpccg_hip_pcg_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.PCG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.pcg_lib()
    err = hp.lib().hpccg_hip_last_error
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    ll = (C.c_longlong * 1)()
    p = C.addressof(buf)
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first

    def solve(f, h=fake, nrhs=2, b=p, ldb=4, x=p, ldx=4, minv=None, max_iter=10, its=it, nrs=nr):
        return f(h, nrhs, b, ldb, x, ldx, minv, max_iter, 0.0, its, nrs, None)

    for f in (L.hpccg_hip_pcg_solve_device, L.hpccg_hip_pcg_solve):
        for kw in (dict(h=None), dict(b=None), dict(x=None), dict(its=None), dict(nrs=None)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"NULL" in err()
        for nrhs in (-1, -3, 0):
            assert solve(f, nrhs=nrhs) == EINVAL
            assert b"nrhs" in err()
        assert solve(f, max_iter=-1) == EINVAL
        assert b"max_iter" in err()
        # a leading dimension below every row count (one below this matrix's
        # rows needs the matrix: test_gpu_pcg.py)
        for kw in (dict(ldb=-1), dict(ldx=-1)):
            assert solve(f, **kw) == EINVAL, kw
            assert b"leading dimension" in err()
    assert L.hpccg_hip_pcg_diagonal(None, p) == EINVAL
    assert L.hpccg_hip_pcg_diagonal(fake, None) == EINVAL
    assert L.hpccg_hip_pcg_release(None) == EINVAL
    assert L.hpccg_hip_pcg_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_pcg_last_trace(fake, 0, None, 8) == EINVAL
    assert L.hpccg_hip_pcg_last_trace(fake, 0, buf, 8) == EINVAL  # (no solve ran on it: the records are searched only)
    assert b"no trace" in err()
    assert L.hpccg_hip_pcg_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_pcg_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_pcg_workspace_bytes(fake, ll) == 0 and ll[0] == 0
    assert L.hpccg_hip_pcg_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_pcg_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.pcg_live_workspaces() == 0


def test_a_strided_one_column_is_refused(hp):
    """A 1-D B or X is one column through a view; a strided one would be solved in a copy."""
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_pcg(None, np.zeros(8), np.zeros(16)[::2])
    with pytest.raises(hp.HPCCGError, match="contiguous"):
        hp.HPCCG_pcg(None, np.zeros(16)[::2], np.zeros(8))


def _nt_value_loads(lib_path):
    """demangled kernel name -> 16-byte global loads carrying the non-temporal
    hint in the library's gfx950 code object (its disassembly)."""
    import shutil
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    for tool in ("clang-offload-bundler", "llvm-objdump"):
        assert os.path.exists(os.path.join(llvm, tool)), f"{tool} not in {llvm}"
    assert shutil.which("objcopy") and shutil.which("c++filt"), "binutils missing"
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb.bin"), os.path.join(d, "co.elf")
        subprocess.run(["objcopy", f"--dump-section=.hip_fatbin={fb}", lib_path, os.path.join(d, "lib.copy")],
                       check=True, capture_output=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fb}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True,
                       capture_output=True)
        asm = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", co], check=True, capture_output=True,
                             text=True).stdout
    counts, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"[0-9a-f]+ <(\w+)>:$", line)
        if m:
            cur = m.group(1)
            counts[cur] = 0
        elif cur is not None and re.match(r"\s+global_load_dwordx4 .* nt\s", line):
            counts[cur] += 1
    names = list(counts)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return {d.replace("hpccg::(anonymous namespace)::", ""): counts[n] for n, d in zip(names, dem.splitlines())}


def test_every_a_image_spmm_keeps_its_non_temporal_loads(hp):
    """The SpMM bodies branch on the view's nt flag inside the kernel, and the
    two arms differ in the loads' hint alone; merged by the optimiser, the hint
    is lost without a trace in the results (csrc/hpccg_spmm.h: arm). Every
    SELL-512-A form of both libraries over the shared loops keeps hinted loads
    (lost, a form has none at all)."""
    for path, prefix in ((hp.PCG_LIB_PATH, "k_pcg_spmm_a<"), (hp.BATCH_LIB_PATH, "k_batch_spmm_a<")):
        nt = {n: c for n, c in _nt_value_loads(path).items() if prefix in n}
        assert len(nt) == (10 if "pcg" in prefix else 7), sorted(nt)
        for n, c in nt.items():
            assert c >= 1, (n, c)


def test_kernel_budgets(hp):
    ks = _kernels(hp.PCG_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_pcg_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    spmm = {n: r for n, r in ks.items() if "k_pcg_spmm_" in n}
    # widths 27, 7 and per-slice; one, two and four columns each; the int32-column form likewise; the
    # 27-wide four-column form also compiled for five waves per SIMD (the batch library's plan choices)
    frags = [f"k_pcg_spmm_a<{w}, {r}, 4>" for w in (27, 7, 0) for r in (1, 2, 4)]
    frags += ["k_pcg_spmm_a<27, 4, 5>"] + [f"k_pcg_spmm_sell<{r}>" for r in (1, 2, 4)]
    for frag in frags:
        assert any(frag in n for n in spmm), frag
    assert len(spmm) == len(frags), sorted(spmm)
    for n, r in spmm.items():
        assert r["vgpr_count"] <= 128, (n, r)
    light = {n: r for n, r in ks.items() if "k_pcg_p<" in n or "k_pcg_update<" in n or "k_pcg_finalize" in n}
    for frag in ["k_pcg_finalize"] + [f"k_pcg_{k}<{r}>" for k in ("p", "update") for r in (1, 2, 4)]:
        assert any(frag in n for n in light), frag
    assert len(light) == 7, sorted(light)
    for n, r in light.items():
        assert r["vgpr_count"] <= 64, (n, r)
    # every SpMM form of the batch library has its twin here (one source, two wrappers)
    kb = _kernels(hp.BATCH_LIB_PATH)
    for n, r in kb.items():
        if "k_batch_spmm_" in n:
            twin = n.replace("k_batch_", "k_pcg_").replace("BatchArgs", "PcgArgs")
            assert twin in ks, twin
