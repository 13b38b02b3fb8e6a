"""CPU-only checks of the batch library (lib/libhpccg_hip_batch.so,
include/hpccg_hip_batch.h): it is built beside the main library, exports what
its header declares, refuses bad arguments before touching HIP, and its
kernels keep their budget (read from its gfx950 code object): at most 16
kernels, no spills, scratch <= 32 B, the SpMM kernels <= 128 VGPRs, the p and
update kernels <= 64. The main library's own ABI is unchanged.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
EINVAL = -1


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.BATCH_LIB_PATH), "run build(): libhpccg_hip_batch.so is missing"
    declared = hp.batch_exported_symbols()
    assert len(declared) == 8, declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.BATCH_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    L = hp.batch_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the batch entry points live in the second library only
    assert "hpccg_hip_batch" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    main = subprocess.run(["nm", "-D", "--defined-only", hp.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout
    assert "hpccg_hip_batch" not in main
    for s in ("hpccg_hip_internal_view", "hpccg_hip_internal_on_destroy"):
        assert f" T {s}" in main, s


def test_abi_versions(hp):
    assert hp.batch_lib().hpccg_hip_batch_abi_version() == 1
    assert hp.lib().hpccg_hip_abi_version() == 2


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.BATCH_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.batch_lib()
    it = (C.c_int * 4)()
    nr = (C.c_double * 4)()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert L.hpccg_hip_batch_solve_device(None, 2, p, 4, p, 4, 10, 0.0, it, nr, None) == EINVAL
    assert b"NULL" in hp.lib().hpccg_hip_last_error()
    assert L.hpccg_hip_batch_solve(None, 2, p, 4, p, 4, 10, 0.0, it, nr, None) == EINVAL
    fake = C.c_void_p(p)  # never dereferenced: the argument checks come first
    for nrhs in (0, -3):
        assert L.hpccg_hip_batch_solve_device(fake, nrhs, p, 4, p, 4, 10, 0.0, it, nr, None) == EINVAL
        assert b"nrhs" in hp.lib().hpccg_hip_last_error()
        assert L.hpccg_hip_batch_sparsemv(fake, nrhs, p, 4, p, 4) == EINVAL
    assert L.hpccg_hip_batch_solve_device(fake, 2, p, 4, p, 4, -1, 0.0, it, nr, None) == EINVAL
    assert b"max_iter" in hp.lib().hpccg_hip_last_error()
    assert L.hpccg_hip_batch_sparsemv(None, 2, p, 4, p, 4) == EINVAL
    assert L.hpccg_hip_batch_release(None) == EINVAL
    assert L.hpccg_hip_batch_last_trace(None, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_batch_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_batch_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.batch_live_workspaces() == 0


def _kernels(lib_path):
    """name -> resources of every kernel of the library's gfx950 code object
    (this file's own reader of the code object's notes)."""
    for tool in ("clang-offload-bundler", "llvm-readelf"):
        assert os.path.exists(os.path.join(LLVM, tool)), f"{tool} not in {LLVM}"
    assert shutil.which("objcopy") and shutil.which("c++filt"), "binutils missing"
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb.bin"), os.path.join(d, "co.elf")
        subprocess.run(["objcopy", f"--dump-section=.hip_fatbin={fb}", lib_path, os.path.join(d, "lib.copy")],
                       check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fb}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True,
                       capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                               capture_output=True, text=True).stdout
    # (the keys read here follow .name within a kernel's entry)
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)",
                     line)
        if not m:
            continue
        k, v = m.groups()
        if k == "name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k] = int(v)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return {d.replace("hpccg::(anonymous namespace)::", ""): out[n] for n, d in zip(names, dem.splitlines())}


def test_kernel_budgets(hp):
    ks = _kernels(hp.BATCH_LIB_PATH)
    assert 0 < len(ks) <= 16, sorted(ks)
    for n, r in ks.items():
        assert "k_batch_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] <= 32, (n, r)
    spmm = {n: r for n, r in ks.items() if "k_batch_spmm_" in n}
    # widths 27, 7 and per-slice, two and four columns each; the int32-column form likewise
    # (the 27-wide four-column form also compiled for five waves per SIMD: the HBM-streamed images)
    for frag in ("k_batch_spmm_a<27, 2, 4>", "k_batch_spmm_a<27, 4, 4>", "k_batch_spmm_a<27, 4, 5>",
                 "k_batch_spmm_a<7, 2, 4>", "k_batch_spmm_a<7, 4, 4>", "k_batch_spmm_a<0, 2, 4>",
                 "k_batch_spmm_a<0, 4, 4>", "k_batch_spmm_sell<2>", "k_batch_spmm_sell<4>"):
        assert any(frag in n for n in spmm), frag
    for n, r in spmm.items():
        assert r["vgpr_count"] <= 128, (n, r)
    light = {n: r for n, r in ks.items() if "k_batch_update<" in n or "k_batch_p<" in n}
    assert len(light) == 4, sorted(light)
    for n, r in light.items():
        assert r["vgpr_count"] <= 64, (n, r)
    assert any("k_batch_finalize" in n for n in ks)
