"""What tests/test_gpu_dot_shapes.py and tests/test_gpu_dot_shapes_group.py rely
on, pinned without a GPU (the table and references of tests/dot_shapes.py):

  * plan(n) of every table row gives the table's nslices and ng, and across the
    table every arm occurs: b = 0 alone and b >= 1 in a round, one and two
    rounds, one and two top passes, all three finalize_groups sizes and both top
    forms of the single solve (the global-memory arm, ng > 2048, is not in the
    table: DESIGN.md section 5);
  * reference spread: for g17 and g65 with every library (both m) and g257 with
    batch, pcg and srcg, and for both groups, the restatement under the second
    dot order (np.dot; for a group the members' sequential sums added in rank
    order) stays within a tenth of the GPU tests' bar on the checked part of the
    trace and within 1e-10 max(1, max|x|) on x;
  * sensitivity: for every dot the restatements of batch, pcg, srcg and poly
    form (r.r, r.z, p.Ap; all above the trace cutoff), the last slice's and the
    last group's part of the sum is at least 100 x RTRANS_RTOL_1GPU of it, so a
    completion that loses either misses the bar by two orders of magnitude;
  * the integer r0.r0 of the device-generated stencil is the oracle's at g17.

Measured (test_reference_spread's and test_shares_are_reported's output; the
bars are 1e-9 on rtrans, 1e-8 for a group, and 1e-10 on x; the shares against
1e-6), with the factors and max_iter of dot_shapes.TABLE (g17: 2^8 and 5; g65:
2^12 and 3; g257: 2^16 and 4, column 0; its comment has what 2^8 gave):
  g17 caller's m   spread rtrans 2.8e-13, x 5.5e-14; Jacobi 1.7e-13, 9.3e-16
  g65 caller's m   spread rtrans 2.8e-13, x 1.3e-13; Jacobi 1.1e-13, 1.6e-14
  g257 caller's m  spread rtrans 3.6e-13, x 6.1e-14
  csr_g65_g17      spread rtrans 2.4e-13, x 3.2e-14
  gen_g65_g65      spread rtrans 4.4e-13, x 1.4e-13
  smallest share of a dot in the last slice / in the last group:
  g17 1.2e-3 / 2.1e-3, g65 1.7e-4 / 1.7e-4, g257 1.9e-5 / 1.9e-5 (one row each).
"""
import numpy as np
import pytest

import columns_fuzz as cf
import dot_shapes as ds
import oracle
from conftest import RTRANS_CUTOFF, RTRANS_RTOL_1GPU, RTRANS_RTOL_MULTI
from test_columns_fuzz_cpu import trace_spread
from test_gpu_poly32_group import rank_dot

_shares = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    ds.release()


def test_plan_restates_the_table_and_every_arm_occurs():
    plans = {}
    for name, (dims, nslices, ng, max_iter, _, _, _) in ds.TABLE.items():
        p = plans[name] = ds.plan(ds.nrows(name))
        assert (p.nslices, p.ng) == (nslices, ng), (name, p)
        assert 3 <= max_iter <= 5
    P = ds.Plan
    assert plans["g17"] == P(1026, 17, 1, 2, 2, 1, True, 4, "polled")
    assert plans["g64"] == P(4096, 64, 1, 4, 4, 1, True, 4, "polled")
    assert plans["g65"] == P(4097, 65, 2, 4, 1, 1, True, 16, "polled")
    assert plans["g65_27pt"] == P(4128, 65, 2, 4, 1, 1, True, 16, "polled")
    assert plans["g256"] == P(16384, 256, 4, 4, 4, 1, True, 16, "polled")
    assert plans["g257"] == P(16385, 257, 5, 4, 1, 2, True, 32, "wave")
    assert {p.rounds > 1 for p in plans.values()} == {False, True}
    assert {1, 2, 4} <= {p.b_used for p in plans.values()} | {p.b_last for p in plans.values()}
    assert {p.top_passes for p in plans.values()} == {1, 2}
    assert {p.finalize for p in plans.values()} == {4, 16, 32}
    assert {p.top for p in plans.values()} == {"polled", "wave"}
    # the edges of the last slice and group: 37 rows in a group of 2 slices; one row alone; 32 slices of 512
    assert ds.nrows("g17") - 512 * 1025 == 37 and 1026 - 64 * 16 == 2
    assert ds.nrows("g65") - 512 * 4096 == 1 and ds.nrows("g257") - 512 * 16384 == 1
    assert ds.nrows("g65_27pt") == 512 * 4128 and 4128 - 64 * 64 == 32
    # what the existing suite stops at, and the arm left out
    assert ds.plan(106 ** 3).ng == 37 and ds.plan(66 * 512).ng == 2
    assert ds.plan(67108865) == P(131073, 2049, 33, 4, 1, 9, False, 32, "wave")
    # the groups' members are table shapes
    assert ds.counts("csr_g65_g17") == [2097153, 524837] and ds.counts("gen_g65_g65") == [2097153] * 2


def _second(name):
    return rank_dot(ds.members(name)) if name in ds.GROUPS else "np"


CASES = [(name, precond) for name in ds.CSR_SHAPES for precond in ("caller", "jacobi")]
CASES += [("g257", "caller")] + [(name, "caller") for name in ds.GROUPS]


@pytest.mark.parametrize("name,precond", CASES, ids=lambda v: str(v))
def test_reference_spread(name, precond):
    c = ds.case(name, precond)
    bar = 0.1 * (RTRANS_RTOL_MULTI if name in ds.GROUPS else RTRANS_RTOL_1GPU)
    worst = [0.0, 0.0]
    for lib in ds.run_libs(name):
        if precond == "jacobi" and lib not in cf.PRECONDITIONED:
            continue
        first = ds.references(c, lib, cache=False)
        second = ds.references(c, lib, dot=_second(name), cache=False)
        if lib == "pcg" and name == "g17":  # what poly at degree 0 is held to
            for a, b in zip(first, ds.references(c, "poly", 0, cache=False)):
                assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
        for k, (a, b) in zip(c["held"], zip(first, second)):
            assert a[1] == b[1] == c["max_iter"] - 1, (lib, k, a[1], b[1])
            ts = trace_spread(a[3], b[3])
            xs = float(np.max(np.abs(a[0] - b[0]))) / max(1.0, float(np.max(np.abs(a[0]))))
            worst = [max(worst[0], ts), max(worst[1], xs)]
            assert ts <= bar, (lib, k, ts)
            assert xs <= 1e-10, (lib, k, xs)
            if lib == "mixed":
                assert a[4][0].tobytes() == b[4][0].tobytes(), (k, a[4][0], b[4][0])
    print(f"\n{name} {precond}: spread rtrans {worst[0]:.1e}, x {worst[1]:.1e}")
    ds.release(name)


def _recording(name, into):
    """oracle.ddot that records the last slice's and the last group's share of every sum."""
    n = ds.nrows(name)
    p = ds.plan(n)
    s0 = 512 * (p.nslices - 1)
    g0 = 512 * 64 * (p.ng - 1)

    def dot(x, y):
        tot = oracle.ddot(x, y)
        into.append((abs(oracle.ddot(x[s0:], y[s0:]) / tot), abs(oracle.ddot(x[g0:], y[g0:]) / tot), tot))
        return tot
    return dot


@pytest.mark.parametrize("name", ds.CSR_SHAPES + ["g257"])
def test_the_last_slice_and_group_carry_a_visible_share_of_every_dot(name):
    c = ds.case(name)
    A = ds.matrix(name)
    B, X0 = ds.columns(name)
    m = cf.precond(c, A)[1]
    lmin, lmax = cf.bounds(c, A)
    need = 100.0 * RTRANS_RTOL_1GPU
    for lib in ("batch", "pcg", "srcg", "poly"):
        if lib not in ds.REFERENCE_LIBS[name]:
            continue
        for k in c["held"]:
            seen = []
            ref = cf.reference(lib, A, B[k], X0[k], m, ds.DEGREE, c["max_iter"], 0.0, _recording(name, seen), lmin, lmax)
            r0 = ref[3][0] ** 2
            assert ref[3][-1] ** 2 >= RTRANS_CUTOFF * r0  # the whole trace is checked
            assert len(seen) >= 3 * (c["max_iter"] - 1)
            low = (min(s[0] for s in seen), min(s[1] for s in seen))
            w = _shares.setdefault(name, [1.0, 1.0])
            w[0], w[1] = min(w[0], low[0]), min(w[1], low[1])
            assert low[0] >= need and low[1] >= need, (lib, k, low)
    ds.release(name)


def test_shares_are_reported():
    print()
    for name, w in _shares.items():
        print(f"{name}: smallest share of a dot in the last slice {w[0]:.1e}, in the last group {w[1]:.1e}")


def test_the_generated_r0_is_the_integer():
    n = ds.nrows("g17")
    assert ds.rr0("g17") == 625 * (n - 2) + 1352
    assert ds.rr0("g257") == 625 * (ds.nrows("g257") - 2) + 1352
    A = oracle.generate(1, 1, n)
    assert set(np.unique(A.b)) == {25.0, 26.0} and A.b[0] == A.b[-1] == 26.0
    ref = oracle.hpccg(A, max_iter=1)
    assert ref["trace"][0] == np.sqrt(np.float64(ds.rr0("g17")))
    assert oracle.ddot(A.b, A.b) == float(ds.rr0("g17"))
