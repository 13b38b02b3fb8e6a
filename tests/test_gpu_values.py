"""The single solve's kernel forms on matrices with distinct values (the tables
of tests/values_cases.py; tests/test_values_cpu.py holds what is relied on here).

tests/test_gpu_fuzz.py crosses the forms with the option sets on generated
stencils, where every off-diagonal is -1.0: a kernel that reads an entry's
value from another slot of its row or slice computes the same bits there. Here
every stored entry has its own value, half of the matrices are not symmetric,
and x0 is random in most cases (so the prologue's SpMV sees the values too).

  * test_spmv_and_solves (one per one-rank case): HPC_sparsemv with the
    SELL-512 kernel and, where there is an A image, the direct kernel in
    prologue mode, byte for byte oracle.sparsemv (rows ascending in the image:
    the sums round alike); then three solves -- the plainest form (SELL-512,
    nothing fused, no graph), the defaults, the drawn option set (a refused
    option keeps its previous value) -- bitwise equal in niters, normr, trace
    and x, and against oracle.hpccg on the same CSR: niters equal, rtrans
    within RTRANS_RTOL_1GPU, x within 1e-9 relative, termination by
    columns_fuzz.check_end (conftest.check_final where the reference ends in
    rounding noise);
  * test_pinned_cross (each pinned shape, a symmetric and a non-symmetric
    matrix): every kernel form -- SELL, direct, direct with the per-iteration
    resident launch, direct with the persistent launch, pairs with register
    loads, pairs with the LDS-DMA value ring -- crossed with fuse_p, x_defer
    and use_graph, and at 16x16x16 and 32x32x33 the option set a 200^3 27-pt
    matrix gets by default, each bitwise the plainest form; max_iter 25 from a
    random x0;
  * test_census (last): from the effective options read back before every
    solve, each kernel form ran on these matrices at least three times.
"""
import itertools

import numpy as np
import pytest

import columns_fuzz as cf
import oracle
import values_cases as vc
from conftest import RTRANS_RTOL_1GPU, check_trace
from test_gpu_parity import dev, host, keep_sell  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SELL, DIRECT, PAIRS = 0, 1, 2
PLAIN = {"spmv_kernel": SELL, "fuse_p": 0, "fold": 0, "x_defer": 0, "use_graph": 0, "fuse_update": 0,
         "resident_update": 0}
# the options as a new matrix holds them (test_spmv_and_solves checks that setting them changes nothing)
DEFAULTS = {"spmv_kernel": -1, "fuse_p": -1, "fold": -1, "x_defer": 2, "x_ring": -1, "use_graph": 1,
            "graph_chunk": 32, "a2_ring": -1, "fuse_update": -1, "resident_update": -1, "nt": -1}
# What a 200^3 27-pt matrix runs by default, read from the library's choices (csrc/hpccg_solver.cpp): its image
# of 8e6 x 27 x 8 B is beyond the 256 MB Infinity Cache, so choose_kernel takes the pair windows, nt_load_of the
# non-temporal loads and x_ring_effective (beyond 512 MB) the ring of 32; a2_ring_effective keeps the LDS-DMA
# ring of 3 at width 27; fuse_p_effective and fold_effective are on; x_defer 2 is carried by the ring kernel;
# fuse_update_effective and resident_of need the direct kernel, so both are off.
DEFAULT_200 = dict(DEFAULTS, spmv_kernel=PAIRS, a2_ring=3, x_ring=32, nt=1)
CENSUS_KEYS = ("spmv_kernel", "a2_ring", "fuse_p", "fuse_update", "resident_update", "x_defer", "nt")
RESIDENT_PERSIST = 8  # (what get_option reports for the persistent launch)
FORMS = {
    "sell": {"spmv_kernel": SELL},
    "direct": {"spmv_kernel": DIRECT, "resident_update": 0},
    "direct_resident": {"spmv_kernel": DIRECT, "resident_update": 1},
    "direct_persistent": {"spmv_kernel": DIRECT, "resident_update": -1},
    "pairs": {"spmv_kernel": PAIRS, "a2_ring": 0},
    "pairs_ring": {"spmv_kernel": PAIRS, "a2_ring": 3},
}

_census = {}  # form -> [the effective option tuples it ran with]


def effective(M):
    return tuple(M.get_option(k) for k in CENSUS_KEYS)


def form_of(eff):
    e = dict(zip(CENSUS_KEYS, eff))
    if e["spmv_kernel"] == SELL:
        return "sell"
    if e["spmv_kernel"] == PAIRS:
        return "pairs_ring" if e["a2_ring"] > 0 else "pairs"
    return {0: "direct", 1: "direct_resident", RESIDENT_PERSIST: "direct_persistent"}[e["resident_update"]]


def apply(hp, M, opts):
    """Set what the matrix accepts (a refused option keeps its previous value); the options that took."""
    applied = {}
    for k, v in opts.items():
        try:
            M.set_option(k, v)
            applied[k] = v
        except hp.HPCCGError:  # not available for this matrix (e.g. no A image)
            pass
    return applied


def solve(hp, M, b, x0, max_iter, tol=0.0):
    """(x, niters, normr, trace); the form that runs goes into the census."""
    eff = effective(M)
    _census.setdefault(form_of(eff), []).append(eff)
    x = x0.copy()
    ierr, it, nr, _ = hp.HPCCG(M, b, x, max_iter=max_iter, tolerance=tol)
    assert ierr == 0
    return x, it, nr, M.last_trace().copy()


def same_bits(got, base, what):
    assert got[1] == base[1] and got[2] == base[2], (what, got[1:3], base[1:3])
    assert got[3].tobytes() == base[3].tobytes(), what
    assert got[0].tobytes() == base[0].tobytes(), what


@pytest.mark.parametrize("case", vc.cases("one"), ids=lambda c: c["name"])
def test_spmv_and_solves(hp, gpu, keep_sell, case):
    import torch
    A = vc.matrix(case)
    b, x0 = vc.columns(case, A)
    tol, max_iter = vc.tolerance(case), case["max_iter"]
    ref = vc.reference(case)
    has_a, width, _ = vc.form(case)
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    try:
        assert M.get_option("has_sell") == 1 and M.get_option("has_a") == has_a
        if has_a:
            assert M.get_option("a_width") == width, (M.get_option("a_width"), width)
        fresh = effective(M)
        assert apply(hp, M, DEFAULTS) == DEFAULTS and effective(M) == fresh
        # the SpMV alone, bitwise
        v = np.random.default_rng(case["col_seed"] + 1).uniform(-1.0, 1.0, A.nrow)
        want = oracle.sparsemv(A, v)
        for kernel in (SELL, DIRECT) if has_a else (SELL,):
            M.set_option("spmv_kernel", kernel)
            assert M.get_option("spmv_kernel") == kernel
            y = torch.zeros(A.nrow, dtype=torch.float64, device=gpu)
            hp.HPC_sparsemv(M, dev(gpu, v), y)
            assert host(y).tobytes() == want.tobytes(), kernel
        # the three solves
        assert apply(hp, M, dict(DEFAULTS, **PLAIN)) == dict(DEFAULTS, **PLAIN)
        assert effective(M)[:5] == (SELL, 0, 0, 0, 0)
        plain = solve(hp, M, b, x0, max_iter, tol)
        apply(hp, M, DEFAULTS)
        assert effective(M) == fresh
        default = solve(hp, M, b, x0, max_iter, tol)
        applied = apply(hp, M, case["opts"])
        drawn = solve(hp, M, b, x0, max_iter, tol)
    finally:
        M.close()
    same_bits(default, plain, ("defaults", fresh))
    same_bits(drawn, plain, applied)
    assert plain[1] == ref["niters"], (plain[1], ref["niters"])
    check_trace(plain[3], ref["trace"], RTRANS_RTOL_1GPU)
    assert vc.x_spread(ref["x"], plain[0]) <= 1e-9
    cf.check_end(plain, (ref["x"], ref["niters"], ref["normr"], ref["trace"]), max_iter)


CROSS = [(name, dims, s7, sym) for name, dims, s7 in vc.PINNED for sym in (True, False)]


@pytest.mark.parametrize("shape", CROSS, ids=lambda s: f"{s[0]}-{'sym' if s[3] else 'nonsym'}")
def test_pinned_cross(hp, gpu, keep_sell, shape):
    name, dims, s7, sym = shape
    A = vc.dominant(*dims, s7, sym, False, 1000 + len(name))
    rng = np.random.default_rng(2000 + len(name))
    b, x0 = A.b, rng.uniform(-1.0, 1.0, A.nrow)
    max_iter = vc.PINNED_MAX_ITER
    ref = oracle.hpccg(A, b=b, x=x0, max_iter=max_iter)
    sets = dict(FORMS)
    if name in ("16x16x16", "32x32x33"):
        sets["default_200"] = DEFAULT_200
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    ran = {}
    try:
        assert M.get_option("has_a") == 1 and M.get_option("has_sell") == 1 and M.get_option("has_pairs") == 1
        assert M.get_option("a_width") == cf.form(A)[1]
        apply(hp, M, dict(DEFAULTS, **PLAIN))
        plain = solve(hp, M, b, x0, max_iter)
        for (form, opts), fuse_p, x_defer, use_graph in itertools.product(sets.items(), (0, -1), (0, 1, 2), (0, 1)):
            want = dict(DEFAULTS, **opts)
            if form != "default_200":
                want.update(fuse_p=fuse_p, x_defer=x_defer)
            want["use_graph"] = use_graph
            assert apply(hp, M, want) == want
            eff = effective(M) + (M.get_option("x_ring"), use_graph)
            # "where available": a form the matrix does not get (no ring at this width, not resident) runs as
            # another one of the list, and a cross entry that changes nothing for a form has run already
            if eff in ran:
                continue
            ran[eff] = form
            if form == "default_200":
                assert eff == (PAIRS, 3, 1, 0, 0, 2, 1, 32, use_graph), eff
            same_bits(solve(hp, M, b, x0, max_iter), plain, (form, want))
    finally:
        M.close()
    # every form the width allows did run (effective values)
    forms = {form_of(e[:len(CENSUS_KEYS)]) for e in ran}
    width = cf.form(A)[1]
    assert {"sell", "direct", "pairs"} <= forms, forms
    if width in (7, 27):
        assert "pairs_ring" in forms, forms
    if width == 27:
        assert {"direct_resident", "direct_persistent"} <= forms, forms
    assert plain[1] == ref["niters"] == max_iter - 1
    check_trace(plain[3], ref["trace"], RTRANS_RTOL_1GPU)
    assert vc.x_spread(ref["x"], plain[0]) <= 1e-9


def test_census():
    """Over the module (it runs last, after the tests above): every kernel
    form ran on a distinct-valued matrix at least three times, the fused forms
    and the non-temporal arm among them."""
    counts = {form: len(_census.get(form, ())) for form in FORMS}
    print()
    for form in FORMS:
        print(f"{form:18s} {counts[form]:5d} solves, {len(set(_census.get(form, ())))} effective option sets")
    assert all(n >= 3 for n in counts.values()), counts
    every = [dict(zip(CENSUS_KEYS, e)) for effs in _census.values() for e in effs]
    for key, values in (("fuse_p", (0, 1)), ("fuse_update", (0, 1)), ("x_defer", (0, 1, 2)), ("nt", (0, 1))):
        for v in values:
            assert sum(1 for e in every if e[key] == v) >= 3, (key, v)
