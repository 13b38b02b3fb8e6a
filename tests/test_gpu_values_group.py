"""The multi-rank forms of the single solve on matrices with distinct values
(the 32 groups of tests/values_cases.py; tests/test_values_cpu.py holds what is
relied on here).

tests/test_gpu_group_fuzz.py runs generated stencils in equal slabs, where
every off-diagonal is -1.0. Here the global matrix has the stencil's structure
and a value of its own at every entry (half of them not symmetric), and it is
cut on plane boundaries into slabs whose plane counts are drawn independently
per member (group_from_csr; group_generate cannot make unequal slabs).

One test per group: group_HPCCG with the plainest form (SELL-512, nothing
fused, no graph), the defaults and the drawn option set (an option some member
refuses is kept by all) -- bitwise equal on every member, every member holding
the same trace -- and against the oracle's serial solve of the global CSR:
niters equal, rtrans within RTRANS_RTOL_MULTI, x within 1e-9 relative.
Groups of equal slabs must be on the z-slab plan (halo_mode 1); for unequal
slabs the plan the library chose goes into the census, and test_census (last)
requires at least eight of them on the slab plan and every SpMV kernel on a
member at least three times.
"""
import numpy as np
import pytest

import values_cases as vc
from conftest import RTRANS_RTOL_MULTI, check_trace
from test_gpu_parity import keep_sell  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

PLAIN = {"spmv_kernel": 0, "fuse_p": 0, "fold": 0, "x_defer": 0, "use_graph": 0}
# the options of vc.GROUP_OPTIONS as a new member holds them
DEFAULTS = {"spmv_kernel": -1, "fuse_p": -1, "fold": -1, "x_defer": 2, "x_ring": -1, "use_graph": 1, "a2_ring": -1}
CENSUS_KEYS = ("spmv_kernel", "a2_ring", "fuse_p", "fuse_update", "resident_update", "x_defer", "nt")

_census = {"halo": [], "members": []}  # (case, equal slabs, halo_mode); the members' effective option tuples


def effective(Ms):
    return [tuple(M.get_option(k) for k in CENSUS_KEYS) for M in Ms]


def apply(hp, Ms, opts):
    applied = {}
    for k, v in opts.items():
        prev = [M.get_option(k) for M in Ms]
        try:
            for M in Ms:
                M.set_option(k, v)
            applied[k] = v
        except hp.HPCCGError:  # not available on some slab (e.g. no uniform width): all keep theirs
            for M, pv in zip(Ms, prev):
                M.set_option(k, pv)
    return applied


def solve(hp, gpu, Ms, bs, x0s, max_iter):
    import torch
    _census["members"] += effective(Ms)
    bd = [torch.from_numpy(b.copy()).to(gpu) for b in bs]
    xd = [torch.from_numpy(x.copy()).to(gpu) for x in x0s]
    ierr, niters, normr, _ = hp.group_HPCCG(Ms, bd, xd, max_iter=max_iter)
    assert ierr == 0
    trace = Ms[0].last_trace().copy()
    for M in Ms[1:]:
        assert M.last_trace().tobytes() == trace.tobytes()  # one set of all-reduced scalars
    return [x.cpu().numpy() for x in xd], niters, normr, trace


def same_bits(got, base, what):
    assert got[1] == base[1] and got[2] == base[2], (what, got[1:3], base[1:3])
    assert got[3].tobytes() == base[3].tobytes(), what
    for r, (a, b) in enumerate(zip(got[0], base[0])):
        assert a.tobytes() == b.tobytes(), (what, r)


@pytest.mark.parametrize("case", vc.cases("group"), ids=lambda c: c["name"])
def test_group(hp, gpu, keep_sell, case):
    A = vc.matrix(case)
    b, x0 = vc.columns(case, A)
    ref = vc.reference(case)
    rows = vc.rows_of_members(case)
    bs, x0s = [b[rw] for rw in rows], [x0[rw] for rw in rows]
    max_iter = case["max_iter"]
    Ms = hp.group_from_csr(vc.csr_parts(A, vc.counts(case)), A.nrow)
    try:
        halo = {M.get_option("halo_mode") for M in Ms}
        equal = len(set(case["planes"])) == 1
        assert len(halo) == 1
        if equal:
            assert halo == {1}, halo
        _census["halo"].append((case["name"], equal, halo.pop()))
        fresh = effective(Ms)
        # (SELL-512 is kept on every member, so the plainest form is available to all)
        assert apply(hp, Ms, PLAIN) == PLAIN
        assert all(e[:3] == (0, 0, 0) for e in effective(Ms))
        plain = solve(hp, gpu, Ms, bs, x0s, max_iter)
        assert apply(hp, Ms, DEFAULTS) == DEFAULTS and effective(Ms) == fresh
        default = solve(hp, gpu, Ms, bs, x0s, max_iter)
        applied = apply(hp, Ms, case["opts"])
        drawn = solve(hp, gpu, Ms, bs, x0s, max_iter)
    finally:
        for M in Ms:
            M.close()
    same_bits(default, plain, ("defaults", fresh))
    same_bits(drawn, plain, applied)
    assert plain[1] == ref["niters"], (plain[1], ref["niters"])
    check_trace(plain[3], ref["trace"], RTRANS_RTOL_MULTI)
    assert vc.x_spread(ref["x"], np.concatenate(plain[0])) <= 1e-9


def test_census():
    """Over the module (it runs last, after the groups above)."""
    unequal = [h for h in _census["halo"] if not h[1]]
    on_slab = [h for h in unequal if h[2] == 1]
    print(f"\n{len(_census['halo'])} groups, {len(unequal)} of unequal slabs, {len(on_slab)} of those on the slab plan;"
          f" others: {[h for h in unequal if h[2] != 1]}")
    assert len(on_slab) >= 8, (len(unequal), len(on_slab))
    kernels = [e[0] for e in _census["members"]]
    for k in (0, 1, 2):
        print(f"spmv_kernel {k}: {kernels.count(k)} member solves")
        assert kernels.count(k) >= 3, (k, kernels.count(k))
    for key, values in (("a2_ring", (0, 3)), ("fuse_p", (0, 1)), ("x_defer", (0, 1, 2))):
        col = [e[CENSUS_KEYS.index(key)] for e in _census["members"]]
        for v in values:
            assert col.count(v) >= 3, (key, v, col.count(v))
