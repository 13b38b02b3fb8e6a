"""Degenerate and non-finite columns for the multi-column solvers -- a helper
of tests/test_columns_edge_cpu.py and tests/test_gpu_columns_edge.py, not a
test.

The columns are those of test_gpu_edge.cases() (a zero initial residual, the
reference's 0/0 path under a negative tolerance, NaN in b or x0, +-inf in b or
x0) on any CSR of the column suites, and the outcomes the solvers must give for
them come from three references:

  * expect_plain: oracle.hpccg, the plain recurrence (HPCCG.cpp restated);
  * expect_pcg: test_gpu_pcg.restated with the column's x0, for Jacobi and for
    a caller's m;
  * expect_refined: the refinement of include/hpccg_hip_mixed.h restated, with
    its stop rule (a residual that is not finite or exactly zero ends the
    column at that residual step, whatever the tolerance).

tests/test_columns_edge_cpu.py pins what the GPU tests rely on: every case ends
at niters 0 with x untouched or at niters 2 with every x NaN, so the expected
values are exact and no tolerance is involved.
"""
import numpy as np

import oracle
from test_gpu_edge import cases, stencil_rows
from test_gpu_mixed import CSRS, STENCILS, band600, perturbed, random_spd
from test_gpu_pcg import csr_diagonal, restated, scale_of, scaled

MAX_ITER = 30  # (that of test_gpu_edge.cases)

EXACT = ["16c", "12x10x16_7pt", "band600", "dyadic_csr513"]
SHAPES = EXACT + ["plain_csr513"]
CPU_SHAPES = SHAPES + ["p2_" + s for s in SHAPES]
REFINED = ["plain_csr513", "pert_16c"]

# where the infinite entries go on the CSR shapes
CSR_ROWS = {
    "band600": {"row0": 0, "row511": 511, "row520": 520},  # slice 0's first and last row, the five-wide slice
    "csr513": {"row0": 0, "row512": 512},  # (row 512: the one row of the last slice)
}


def csr_of(name):
    """The oracle.CSR (b = A 1) of a shape of the column suites; "p2_": every
    entry a_ij s_i s_j with the power-of-two s of test_gpu_pcg."""
    if name.startswith("p2_"):
        A0 = csr_of(name[3:])
        return scaled(A0, scale_of("p2", A0.nrow))
    if name in STENCILS:
        nx, ny, nz, s7 = STENCILS[name]
        return oracle.generate(nx, ny, nz, use_7pt=s7)
    if name == "band600":
        return band600()
    if name.startswith("pert_"):
        nx, ny, nz, s7 = STENCILS[name[5:]]
        return perturbed(nx, ny, nz, s7, 31)
    form, key = name.split("_")
    n, per_row, band, seed = CSRS[key]
    return random_spd(np.random.default_rng(seed), n, per_row, band, form == "dyadic")


def inf_rows(name):
    """tag -> row of the infinite entries on a shape."""
    base = name[3:] if name.startswith("p2_") else name
    if base.startswith("pert_"):
        base = base[5:]
    if base in STENCILS:
        return stencil_rows(*STENCILS[base][:3])
    return CSR_ROWS["band600" if base == "band600" else base.split("_")[1]]


def shape_cases(name, A=None):
    """[(case name, b, x0, max_iter, tolerance)] of a shape."""
    return cases(csr_of(name) if A is None else A, inf_rows(name))


def group_rows(counts, nx=0, ny=0):
    """The rows next to the boundary between members 0 and 1 -- member 0's last
    plane and a face row of member 1's first (those of
    test_gpu_edge.test_degenerate_starts_group), or the two rows at the
    boundary of CSR slabs -- and one well inside member 1."""
    n0, n1 = counts[0], counts[1]
    if nx:
        return {"lo_side": n0 - nx * ny // 2, "hi_side": n0 + nx * ny // 2 + nx - 1, "inside": n0 + n1 // 2 + nx * (ny // 2) + nx // 2}
    return {"lo_side": n0 - 1, "hi_side": n0, "inside": n0 + n1 // 2}


# ---------------------------------------------------------------------------
# expected outcomes: (x, niters, normr, trace)
# ---------------------------------------------------------------------------
def expect_plain(A, b, x0, max_iter, tol):
    ref = oracle.hpccg(A, b=np.ascontiguousarray(b), x=np.ascontiguousarray(x0), max_iter=max_iter, tolerance=tol)
    return ref["x"], ref["niters"], ref["normr"], ref["trace"]


def expect_pcg(A, b, x0, max_iter, tol, minv=None):
    """minv None: Jacobi, 1 / a_ii."""
    if minv is None:
        minv = 1.0 / csr_diagonal(A)
    return restated(A, b, minv, max_iter, tol, x0=x0)


def fp32_image(A):
    return oracle.CSR(A.row_ptr, A.cols, A.vals.astype(np.float32).astype(np.float64), None, None, None)


def expect_refined(A, b, x0, max_iter, tol, max_sweeps=8, inner_rtol=2.0 ** -20, dot=oracle.ddot):
    """include/hpccg_hip_mixed.h, steps 1 to 4, restated: (x, niters, normr,
    inner trace, (sweep iters, sweep residuals)). dot: the order of every sum
    (the sequential one by default)."""
    A32 = fp32_image(A)
    ones = np.ones(A.nrow)
    x = np.array(x0, np.float64)
    left = max(max_iter, 1) - 1
    iters, resid, trace = [], [], []
    s = 0
    with np.errstate(all="ignore"):
        while True:
            r = b + (-1.0) * oracle.sparsemv(A, x)
            rho = np.sqrt(np.float64(dot(r, r)))
            resid.append(rho)
            if rho <= tol or not np.isfinite(rho) or rho == 0.0 or s == max_sweeps or left == 0:
                break
            d, it, _, tr = restated(A32, r, ones, left + 1, max(tol, inner_rtol * rho), dot=dot)
            x = x + d
            iters.append(it)
            trace.extend(tr)
            left -= it
            s += 1
    return x, int(sum(iters)), float(resid[-1]), np.array(trace), (np.array(iters, np.int32), np.array(resid))


def degenerate(x, niters, normr, trace, x0):
    """What every case comes to, asserted: niters 0 with normr 0.0 or NaN and x
    bitwise x0, or niters 2 (the reference's NaN path) with normr NaN and every
    x NaN; the trace has niters + 1 entries."""
    assert niters in (0, 2), niters
    assert normr == 0.0 or np.isnan(normr), normr
    if niters == 0:
        assert x.tobytes() == np.asarray(x0, np.float64).tobytes()
    else:
        assert np.isnan(normr) and np.isnan(x).all()
    assert len(trace) == niters + 1, (len(trace), niters)


# ---------------------------------------------------------------------------
# arrangements of bad columns among finite ones
# ---------------------------------------------------------------------------
def finite_columns(b, xexact, seed=5):
    """Four finite columns of test_gpu_mixed.columns(): the generated b, the
    scaled b with a nonzero x0, and two random ones (its column 2, x0 = xexact,
    is a degenerate start itself)."""
    from test_gpu_mixed import columns
    B, X0 = columns(b, xexact, 5, seed)
    keep = [0, 1, 3, 4]
    return B[keep], X0[keep]


def arrangements(case_names):
    """[(label, columns, call-wide tolerance)]: a column is an int (a finite
    column of finite_columns) or a case name. exact_negtol is the call-wide
    tolerance -1, so its neighbours run under -1 as well."""
    out = []

    def add(label, cols):
        out.append((label, cols, -1.0 if "exact_negtol" in cols else 0.0))

    for pos in range(4):  # nrhs = 4, nan_b at each position
        cols = [0, 1, 2]
        cols.insert(pos, "nan_b")
        add(f"4/nan_b@{pos}", cols)
    others = [c for c in case_names if c != "nan_b"]
    for i, name in enumerate(others):  # nrhs = 4, every other case, the position rotating
        cols = [0, 1, 2]
        cols.insert(i % 4, name)
        add(f"4/{name}@{i % 4}", cols)
    infs = [c for c in case_names if c.startswith("inf_b_")]
    add("2/bad@0", ["nan_x0", 1])
    add("2/bad@1", [0, infs[0]])
    add("5/bad@4", [0, 1, 2, 3, infs[-1]])  # alone in its launch
    add("5/bad@0", ["nan_b", 0, 1, 2, 3])
    add("3/two_bad", [[c for c in case_names if c.startswith("inf_x0_")][0], 2, infs[-1]])
    return out


def assemble(cols, FB, FX, by_name):
    """(B, X0) of an arrangement; by_name: case name -> (b, x0)."""
    B = np.stack([FB[c] if isinstance(c, int) else by_name[c][0] for c in cols])
    X0 = np.stack([FX[c] if isinstance(c, int) else by_name[c][1] for c in cols])
    return B, X0
