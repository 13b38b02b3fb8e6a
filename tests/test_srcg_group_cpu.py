"""CPU-only checks of the group single-reduction CG library
(lib/libhpccg_hip_srcg_group.so, include/hpccg_hip_srcg_group.h): it is built
beside the ten others, exports exactly what its header declares, refuses bad
arguments before touching HIP, and its kernels (read from its gfx950 code
object) have no scratch and no spills, every SpMM form with the registers and
the non-temporal loads of its twin in the group pcg library. No other library
knows of it.

The restatement the GPU tests hold the solver to -- test_gpu_srcg.restated_sr
with the group's dot, the members' sequential sums added in rank order -- is
pinned here against the classic one (test_gpu_pcg_group.restated) and against
itself under the sequential dot, on the six p10_ group shapes and on the 32
groups of tests/columns_fuzz.py.

Measured margins of the restatement on the p10_ shapes (MAX_ITER 60; the bar is
RTRANS_RTOL_MULTI / 10 = 1e-8):
  shape        against the classic form   points checked
  2x8c         5.2e-13                    29
  8x16c        1.5e-13                    49
  3x33x17x9    8.5e-13                    47
  4x7x5x1      4.7e-11                    17
  7-pt         2.0e-14                    11
  csr3         1.4e-14                    26
and 8.2e-11 at worst against the other dot order. Over the 32 fuzz groups the
two dot orders differ by 1.6e-11 at most on the trace and by 2.6e-12 of
max(1, max|x|) on x.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import columns_fuzz as cf
import test_gpu_pcg_group as tpg
from conftest import RTRANS_RTOL_MULTI, check_trace
from test_batch_cpu import _kernels  # the reader of a library's gfx950 code object notes
from test_columns_fuzz_cpu import trace_spread
from test_gpu_poly32_group import rank_dot
from test_gpu_srcg import restated_sr
from test_pcg_cpu import _nt_value_loads

EINVAL = -1
MAX_MEMBERS = 16

NAMES = ("abi_version", "solve_device", "last_trace", "release", "workspace_bytes", "live_workspaces")


def test_library_exports_every_declared_symbol(hp):
    assert os.path.exists(hp.SRCG_GROUP_LIB_PATH), "run build(): libhpccg_hip_srcg_group.so is missing"
    declared = hp.group_srcg_exported_symbols()
    assert declared == sorted("hpccg_hip_group_srcg_" + s for s in NAMES), declared
    out = subprocess.run(["nm", "-D", "--defined-only", hp.SRCG_GROUP_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for s in declared:
        assert f" T {s}" in out, s
    exported = sorted(set(re.findall(r" T (hpccg_\w+)", out)))
    assert exported == declared, exported  # exactly the six
    L = hp.srcg_group_lib()
    for s in declared:
        assert hasattr(L, s), s
    # the entry points live in the eleventh library only
    assert "hpccg_hip_group_srcg" not in open(os.path.join(hp.ROOT, "include", "hpccg_hip.h")).read()
    others = (hp.LIB_PATH, hp.BATCH_LIB_PATH, hp.MIXED_LIB_PATH, hp.PCG_LIB_PATH, hp.PCG_GROUP_LIB_PATH,
              hp.POLY_LIB_PATH, hp.POLY_GROUP_LIB_PATH, hp.POLY32_LIB_PATH, hp.POLY32_GROUP_LIB_PATH, hp.SRCG_LIB_PATH)
    assert len(set(others)) == 10 and hp.SRCG_GROUP_LIB_PATH not in others
    for other in others:
        syms = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert "hpccg_hip_group_srcg" not in syms, other


def test_abi_version(hp):
    assert hp.srcg_group_lib().hpccg_hip_group_srcg_abi_version() == 1


def test_linked_against_the_main_library_beside_it(hp):
    out = subprocess.run(["readelf", "-d", hp.SRCG_GROUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"NEEDED.*\[libhpccg_hip\.so\]", out), out
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", out), out


def test_bad_arguments_are_refused_without_a_device(hp):
    L = hp.srcg_group_lib()
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
        return L.hpccg_hip_group_srcg_solve_device(Ms, nranks, nrhs, b, ldb, x, ldx, minv, max_iter, 0.0, its, nrs,
                                                   None)

    for kw in (dict(Ms=None), dict(b=None), dict(ldb=None), dict(x=None), dict(ldx=None), dict(its=None),
               dict(nrs=None)):
        assert solve(**kw) == EINVAL, kw
        assert b"NULL" in err() and err().startswith(b"group srcg:"), (kw, err())
    for nranks in (0, -1, MAX_MEMBERS + 1):
        assert solve(Ms=big, nranks=nranks) == EINVAL, nranks
        assert b"nranks" in err() and err().startswith(b"group srcg:")
    for nrhs in (0, -1, -3):
        assert solve(nrhs=nrhs) == EINVAL
        assert b"nrhs" in err() and err().startswith(b"group srcg:")
    assert solve(max_iter=-1) == EINVAL
    assert b"max_iter" in err() and err().startswith(b"group srcg:")
    # the group pcg's order: nranks, nrhs, max_iter, then the NULL arrays
    assert solve(nranks=0, nrhs=0, max_iter=-1, b=None) == EINVAL and b"nranks" in err()
    assert solve(nrhs=0, max_iter=-1, b=None) == EINVAL and b"nrhs" in err()
    assert solve(max_iter=-1, b=None) == EINVAL and b"max_iter" in err()
    # a caller's m for one member only
    for holes in ((None, p), (p, None)):
        assert solve(minv=(C.c_void_p * 2)(*holes)) == EINVAL, holes
        assert b"minv_dev" in err() and b"NULL" in err()
    for r, holes in enumerate(((None, p), (p, None))):
        assert solve(b=(C.c_void_p * 2)(*holes)) == EINVAL
        assert f"B_dev[{r}]".encode() in err()
        assert solve(x=(C.c_void_p * 2)(*holes)) == EINVAL
    assert solve(Ms=(C.c_void_p * 2)(None, None)) == EINVAL  # (a NULL handle: nothing is dereferenced)
    assert b"Ms[0]" in err() and err().startswith(b"group srcg:")

    assert L.hpccg_hip_group_srcg_last_trace(None, 2, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_srcg_last_trace(two, MAX_MEMBERS + 1, 0, buf, 8) == EINVAL
    assert L.hpccg_hip_group_srcg_last_trace(two, 2, 0, None, 8) == EINVAL
    assert L.hpccg_hip_group_srcg_release(None) == EINVAL
    ll = (C.c_longlong * 1)()
    assert L.hpccg_hip_group_srcg_workspace_bytes(None, ll) == EINVAL
    assert L.hpccg_hip_group_srcg_workspace_bytes(fake, None) == EINVAL
    assert L.hpccg_hip_group_srcg_workspace_bytes(fake, ll) == 0 and ll[0] == 0  # (the records are searched only)
    assert L.hpccg_hip_group_srcg_release(fake) == 0  # (no record: nothing to free)
    assert L.hpccg_hip_group_srcg_live_workspaces(None) == EINVAL
    n = C.c_int(-1)
    assert L.hpccg_hip_group_srcg_live_workspaces(C.byref(n)) == 0 and n.value == 0
    assert hp.group_srcg_live_workspaces() == 0


def _twin(name):
    return name.replace("k_pcg_group_", "k_srcg_group_").replace("PcgArgs", "SrcgArgs")


def test_kernel_list_and_budgets(hp):
    ks = _kernels(hp.SRCG_GROUP_LIB_PATH)
    assert ks
    for n, r in ks.items():
        assert "k_srcg_group_" in n, n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["private_segment_fixed_size"] == 0, (n, r)  # no scratch
    spmm = {n: r for n, r in ks.items() if "k_srcg_group_spmm_" in n}
    # the group pcg's thirteen forms: widths 27, 7 and per-slice, one, two and four columns each; the int32-column
    # form likewise; the 27-wide four-column form also compiled for five waves per SIMD
    frags = [f"k_srcg_group_spmm_a<{w}, {r}, 4>" for w in (27, 7, 0) for r in (1, 2, 4)]
    frags += ["k_srcg_group_spmm_a<27, 4, 5>"] + [f"k_srcg_group_spmm_sell<{r}>" for r in (1, 2, 4)]
    for frag in frags:
        assert sum(frag in n for n in spmm) == 1, frag
    assert len(spmm) == len(frags) == 13, sorted(spmm)
    rest = {n: r for n, r in ks.items() if n not in spmm}
    want = ["k_srcg_group_init", "k_srcg_group_finalize", "k_srcg_group_sum", "k_srcg_group_halo",
            "k_srcg_group_diag", "k_srcg_group_check"] + [f"k_srcg_group_{k}<{r}>" for k in ("step", "t")
                                                          for r in (1, 2, 4)]
    for frag in want:
        assert sum(frag in n for n in rest) == 1, frag
    assert len(rest) == len(want) == 12, sorted(rest)
    for n, r in rest.items():
        assert r["vgpr_count"] <= 64, (n, r)
    # each SpMM form beside its twin of the group pcg library: one source, two wrappers, the same registers
    kp = {_twin(n): r for n, r in _kernels(hp.PCG_GROUP_LIB_PATH).items() if "k_pcg_group_spmm_" in n}
    assert sorted(kp) == sorted(spmm), (sorted(kp), sorted(spmm))
    for n, r in spmm.items():
        assert r["vgpr_count"] == kp[n]["vgpr_count"] <= 128, (n, r, kp[n])
    # the step, t and the finalize are the one-rank srcg library's bodies: its registers
    k1 = {n.replace("k_srcg_", "k_srcg_group_"): r for n, r in _kernels(hp.SRCG_LIB_PATH).items()
          if any(f in n for f in ("k_srcg_step<", "k_srcg_t<", "k_srcg_finalize"))}
    assert len(k1) == 7, sorted(k1)
    for n, r in k1.items():
        assert n in rest, n
        assert rest[n]["vgpr_count"] == r["vgpr_count"], (n, rest[n], r)


def test_every_a_image_spmm_keeps_its_non_temporal_loads(hp):
    """The two arms of the SpMM bodies' branch on nt differ in the value loads'
    hint alone (csrc/hpccg_spmm.h: arm); every SELL-512-A form here keeps as
    many hinted loads as its twin of the group pcg library."""
    mine = {n: c for n, c in _nt_value_loads(hp.SRCG_GROUP_LIB_PATH).items() if "k_srcg_group_spmm_a<" in n}
    twins = {_twin(n): c for n, c in _nt_value_loads(hp.PCG_GROUP_LIB_PATH).items() if "k_pcg_group_spmm_a<" in n}
    assert len(mine) == 10, sorted(mine)
    assert mine == twins, (mine, twins)
    assert min(mine.values()) >= 1, mine


# ---------------------------------------------------------------------------
# the group restatement
# ---------------------------------------------------------------------------
MAX_ITER = 60
_globals = {}


def p10_group(shape):
    """(the p10_ global matrix of a group shape, the members' row ranges), as test_gpu_pcg_group.Case builds them."""
    if shape not in _globals:
        A0, counts = tpg.global_matrix(shape)
        A = tpg.scaled(A0, tpg.scale_of("p10", A0.nrow))
        rows, s = [], 0
        for n in counts:
            rows.append(slice(s, s + n))
            s += n
        _globals[shape] = (A, rows)
    return _globals[shape]


@pytest.mark.parametrize("shape", tpg.SHAPES)
def test_the_group_restatement_follows_the_classic_one(shape):
    """restated_sr with the members' sequential dots added in rank order: its
    r.r history within RTRANS_RTOL_MULTI / 10 of the classic restatement's and
    of its own under the sequential dot, over at least 10 points; equal niters."""
    A, rows = p10_group(shape)
    minv = 1.0 / tpg.csr_diagonal(A)
    gdot = rank_dot(rows)
    sr = restated_sr(A, A.b, minv, MAX_ITER, dot=gdot)
    classic = tpg.restated(A, A.b, minv, MAX_ITER)  # (its own dot: the sequential sum)
    seq = restated_sr(A, A.b, minv, MAX_ITER)
    bar = RTRANS_RTOL_MULTI / 10
    n1 = check_trace(sr[3], classic[3], bar)
    n2 = check_trace(sr[3], seq[3], bar)
    print(f"p10_{shape}: against the classic form {trace_spread(classic[3], sr[3]):.1e} over {n1} points, "
          f"against the sequential dot {trace_spread(seq[3], sr[3]):.1e} over {n2}")
    assert n1 >= 10 and n2 >= 10, (n1, n2)
    assert sr[1] == classic[1] == seq[1], (sr[1], classic[1], seq[1])


GROUPS = cf.cases("group")


@pytest.mark.parametrize("case", GROUPS, ids=lambda c: c["name"])
def test_fuzz_groups_are_admissible_for_srcg(case):
    """What tests/test_gpu_srcg_group_fuzz.py relies on, for each of the 32
    groups: the srcg restatement under the sequential dot and under the group's
    agrees with itself at a tenth of the GPU bars and gives equal niters, which
    are the pcg restatement's; the case's tolerance is at least 1 % away from
    every residual of the srcg restatement."""
    A = cf.matrix(case)
    assert not cf.fully_diagonal(A)
    tol = cf.tolerance(case)
    first = cf.case_reference(case, "srcg", tol)
    second = cf.case_reference(case, "srcg", tol, cf.second_dot(case))
    pcg = cf.case_reference(case, "pcg", tol)
    assert len(first) == len(second) == len(pcg) == max(case["nrhs_a"], case["nrhs"])
    worst_t = worst_x = 0.0
    for c, (a, b, p) in enumerate(zip(first, second, pcg)):
        assert a[1] == b[1] == p[1], (c, a[1], b[1], p[1])
        assert len(a[3]) == len(b[3]), c
        ts = trace_spread(a[3], b[3])
        xs = float(np.max(np.abs(a[0] - b[0]))) / max(1.0, float(np.max(np.abs(a[0]))))
        worst_t, worst_x = max(worst_t, ts), max(worst_x, xs)
        assert ts <= 0.1 * RTRANS_RTOL_MULTI, (c, ts)
        assert xs <= 0.1 * 1e-9, (c, xs)
    print(f"{case['name']}: trace {worst_t:.1e}, x {worst_x:.1e}")
    if tol > 0.0:
        for c, r in enumerate(cf.case_reference(case, "srcg", 0.0)):
            res = np.asarray(r[3], np.float64)
            res = res[np.isfinite(res)]
            assert not np.any(np.abs(res - tol) < 0.01 * tol), (c, tol)
