"""Every one-rank solver at the problem sizes where its dot completion changes
shape (tests/dot_shapes.py: the table, plan() and the columns). One test per
shape; each library is called with 1 column and then 3 columns on the same
Matrix, so the workspace grows.

  * g17, g65 on the CSR with a value of its own at every entry: batch, mixed,
    pcg, srcg, poly (degree 2 and 0) and poly32 are held to
    columns_fuzz.reference exactly as tests/test_gpu_columns_fuzz.py holds them
    (its check_columns and check_refined), under a caller's m and under Jacobi;
    what the headers promise bit for bit (a batch column is HPCCG of it; pcg
    with m = 1 is batch; poly at degree 0 is pcg; srcg with max_iter 2 is pcg;
    pcg under a constant power-of-two m returns batch's x bits); the SpMM of
    both images is bitwise oracle.sparsemv (the convert kernels' last slice);
    poly_bound and poly32_bound are NumPy's, as drawn and with m raised at one
    row of the last slice, the one the top block's last stride reads;
  * g64, g256, g65_27pt, generated on the device, no host matrix: the same
    identities, mixed = batch and poly32 = poly on the exact image, and every
    library's trace[0] with x0 = 0 and b = A 1 is the square root of the integer
    KAT-2 gives (dot_shapes.rr0), bit for bit;
  * g257: both, with batch, pcg and srcg under a caller's m held to their
    restatements on oracle.generate's CSR (column 0);
  * the single solve at every shape: fold 0, 1, -1 with use_graph 0 and 1 (one
    iteration per graph, so that the graph is replayed) give the same bits,
    get_option reports the effective option, and at g17, g65 and g257 it is the
    batch column held to oracle.hpccg above;
  * ddot at the table's row counts on small integers equals np.dot exactly.

test_census records plan(n) beside has_a and a_width of every shape and asserts
the device built the 3-wide uniform image on more than 4096 slices and the
27-wide one at g65_27pt (has_a with a_width 27: the x-triple plan on the interior
slices, which the SpMM takes from four columns on; that shape is also run with
four columns, bitwise against the single solves).

Sensitivity, measured once on scratch builds of all eleven libraries (wrong sums
only, never committed), the whole GPU suite under each:
  (a) col_dot_total's g0 loop stops after its first round: fails g65, g65_27pt,
      g256, g257, both groups of tests/test_gpu_dot_shapes_group.py, and of the
      suite before these modules tests/test_gpu_batch.py::test_wide_top_level alone;
  (b) top_sum_wave ignores i0 >= 256 (the header is shared, so the single solve
      loses its second pass too): fails g257 (trace[0] is 72407.73474567478
      where the integer's root is 72407.73941368422: one group of one row) and
      test_gpu_parity.py::test_full_size at 7-pt 256^3, 320^3 and 432^3;
      test_wide_top_level compares the batch with the single solve and passes,
      both being wrong alike;
  (c) col_finalize<true> takes r.z from the r.r total: fails every shape here and
      both groups, and 336 tests of the suite before (every one under an m that
      is not 1).
"""
import numpy as np
import pytest

import columns_fuzz as cf
import dot_shapes as ds
import test_gpu_batch as tb
import test_gpu_columns_fuzz as tcf
import test_gpu_mixed as tm
import test_gpu_pcg as tp
import test_gpu_poly as tpoly
import test_gpu_poly32 as tpoly32
import test_gpu_srcg as tsr
from test_gpu_mixed import assert_same

pytestmark = pytest.mark.gpu

_census = {}
POW2 = 2.0 ** -3


@pytest.fixture(scope="module", autouse=True)
def _workspaces_are_back(hp):
    base = tcf.live(hp)
    yield
    ds.release()
    assert tcf.live(hp) == base


def build(hp, name):
    if ds.TABLE[name][5]:
        A = ds.matrix(name)
        return hp.Matrix.from_csr(A.row_ptr, A.cols, A.vals)
    return hp.Matrix.generate(*ds.TABLE[name][0])


def run(hp, gpu, lib, M, B, X0, max_iter, m=None, degree=ds.DEGREE, lmin=None, lmax=None):
    """[(x, niters, normr, trace, ...)] per column; m: None (Jacobi), a number or an array."""
    if lib == "batch":
        return tb.batch_solve(hp, gpu, M, B, X0, max_iter)
    if lib == "mixed":
        return tm.mixed_solve(hp, gpu, M, B, X0, max_iter)
    if lib == "pcg":
        return tp.pcg_solve(hp, gpu, M, B, X0, max_iter, minv=m)
    if lib == "srcg":
        return tsr.srcg_solve(hp, gpu, M, B, X0, max_iter, minv=m)
    f = tpoly.poly_solve if lib == "poly" else tpoly32.poly32_solve
    return f(hp, gpu, M, B, X0, max_iter, degree=degree, lmin=lmin, lmax=lmax, minv=m)


def one_then_three(hp, gpu, lib, M, B, X0, max_iter, grows, **kw):
    """The library's call with column 0 and then with all three on the same Matrix."""
    held = getattr(M, lib + "_workspace_bytes")
    first = run(hp, gpu, lib, M, B[:1], X0[:1], max_iter, **kw)
    before = held()
    second = run(hp, gpu, lib, M, B, X0, max_iter, **kw)
    # (a batch of one column is the single solve itself and holds no vectors)
    assert held() > before if grows else held() == before > 0, (lib, before, held())
    assert_same(second[:1], first, sweeps=lib == "mixed")
    return first, second


def single_forms(hp, gpu, M, b, x0, max_iter):
    """The single solve of one column under fold 0, 1, -1 and use_graph 0, 1: the same bits."""
    chunk = int(M.get_option("graph_chunk"))
    base = None
    try:
        for fold in (0, 1, -1):
            for graph in (0, 1):
                M.set_option("fold", fold)
                M.set_option("use_graph", graph)
                M.set_option("graph_chunk", 1 if graph else chunk)
                assert M.get_option("fold") == (0 if fold == 0 else 1) and M.get_option("use_graph") == graph
                got = tm.single_solves(hp, gpu, M, b[None], x0[None], max_iter)
                assert got[0][1] == max_iter - 1
                if base is None:
                    base = got
                assert_same(got, base)
    finally:
        M.set_option("fold", -1)
        M.set_option("use_graph", 1)
        M.set_option("graph_chunk", chunk)
    return base


def identities(hp, gpu, M, B, X0, max_iter, last, m):
    """What the headers promise bit for bit, on three columns; last: the libraries' three-column results under m."""
    assert_same(last["batch"], tm.single_solves(hp, gpu, M, B, X0, max_iter))
    assert_same(run(hp, gpu, "pcg", M, B, X0, max_iter, m=1.0), last["batch"])
    scaled = run(hp, gpu, "pcg", M, B, X0, max_iter, m=POW2)
    for g, r in zip(scaled, last["batch"]):
        assert g[1] == r[1] and g[0].tobytes() == r[0].tobytes()
    assert_same(run(hp, gpu, "poly", M, B, X0, max_iter, m=m, degree=0), last["pcg"])
    assert_same(run(hp, gpu, "srcg", M, B, X0, 2, m=m), run(hp, gpu, "pcg", M, B, X0, 2, m=m))


def check_bounds(hp, gpu, name, A, M, m):
    """poly_bound and poly32_bound against NumPy's, as the bound tests of tests/test_gpu_poly.py compare them."""
    import torch
    n = A.nrow
    raised = m.copy()
    row = n - 1 - ((n - 1) % ds.SLICE) // 2  # a row of the last slice
    raised[row] *= 2.0 ** 20
    for what, mv in (("jacobi", None), ("drawn", m), ("raised", raised)):
        mh = 1.0 / tp.csr_diagonal(A) if mv is None else mv
        ref, w = tpoly.numpy_bound(A, mh)
        margin = (w + 3) * 2.0 ** -52  # one rounding per added term, the two products and the sqrt
        md = None if mv is None else torch.from_numpy(mv).to(gpu)
        got, got32 = hp.poly_bound(M, md), hp.poly32_bound(M, md)
        print(f"{name} {what}: bound {got!r} numpy {ref!r}")
        assert abs(got - ref) <= margin * ref, (what, got, ref)
        assert got32 == got, (what, got32, got)
    # the raised row holds the maximum, in the slice the top block (256 threads) reads on its last stride
    q = np.sqrt(raised)
    lo, hi = int(A.row_ptr[row]), int(A.row_ptr[row + 1])
    at_row = q[row] * float(np.sum(np.abs(A.vals[lo:hi]) * q[A.cols[lo:hi].astype(np.int64)]))
    assert at_row == ref and row // ds.SLICE == ds.plan(n).nslices - 1 >= 256


@pytest.mark.parametrize("name", ds.CSR_SHAPES)
def test_csr_shape(hp, gpu, name):
    A = ds.matrix(name)
    n = A.nrow
    B, X0 = ds.columns(name)
    assert not cf.exact32(A)
    M = build(hp, name)
    try:
        _census[name] = tcf.device_form(M, n)
        assert _census[name] == cf.form(A) == (1, 3, ds.plan(n).nslices)
        assert M.mixed_info()["exact"] == 0 and hp.poly32_info(M)["exact"] == 0
        for precond in ("caller", "jacobi"):
            c = ds.case(name, precond)
            max_iter = c["max_iter"]
            minv = cf.precond(c, A)[0]
            lmin, lmax = cf.passed_bounds(c, A)
            last = {}
            for lib in ds.ALL_LIBS if precond == "caller" else cf.PRECONDITIONED:
                ref = ds.references(c, lib)
                first, last[lib] = one_then_three(hp, gpu, lib, M, B, X0, max_iter, precond == "caller", m=minv,
                                                  lmin=lmin, lmax=lmax)
                for what, got, k in (("first call", first, 1), ("second call", last[lib], 3)):
                    if lib == "mixed":
                        tcf.check_refined(A, B, got, ref[:k], what)
                    else:
                        tcf.check_columns(lib, got, ref[:k], max_iter, what)
            poly0 = run(hp, gpu, "poly", M, B, X0, max_iter, m=minv, degree=0)
            tcf.check_columns("poly at degree 0", poly0, ds.references(c, "pcg"), max_iter, precond)
            assert_same(poly0, last["pcg"])
            assert_same(run(hp, gpu, "srcg", M, B, X0, 2, m=minv), run(hp, gpu, "pcg", M, B, X0, 2, m=minv))
            if precond == "caller":
                identities(hp, gpu, M, B, X0, max_iter, last, minv)
                # the single solve's forms: the batch column held to oracle.hpccg above
                assert_same(single_forms(hp, gpu, M, B[0], X0[0], max_iter), last["batch"][:1])
                tcf.check_spmm(hp, gpu, c, A, M, True)
                check_bounds(hp, gpu, name, A, M, minv)
    finally:
        M.close()
        ds.release(name)


def integer_residual(hp, gpu, name, M, n):
    """trace[0] of every library with x0 = 0 and b = A 1: sqrt of the integer, bit for bit (the second column: b / 8)."""
    import torch
    b = torch.zeros(n, dtype=torch.float64, device=gpu)
    hp.HPC_sparsemv(M, torch.ones(n, dtype=torch.float64, device=gpu), b)  # exact
    b = b.cpu().numpy()
    want = np.sqrt(np.float64(ds.rr0(name)))
    B1 = np.stack([b, b * 2.0 ** -3])
    Z = np.zeros_like(B1)
    for lib in ds.ALL_LIBS:
        got = run(hp, gpu, lib, M, B1, Z, 2)
        for k, scale in enumerate((1.0, 2.0 ** -3)):
            assert got[k][3][0] == want * scale, (lib, k, got[k][3][0], want * scale)
    single = tm.single_solves(hp, gpu, M, B1[:1], Z[:1], 2)
    assert single[0][3][0] == want


@pytest.mark.parametrize("name", [k for k in ds.NAMES if k not in ds.CSR_SHAPES])
def test_generated_shape(hp, gpu, name):
    c = ds.case(name)
    n = ds.nrows(name)
    max_iter = c["max_iter"]
    B, X0 = ds.columns(name)
    M = build(hp, name)
    try:
        _census[name] = tcf.device_form(M, n)
        assert _census[name][2] == ds.plan(n).nslices
        assert M.mixed_info()["exact"] == 1 and hp.poly32_info(M)["exact"] == 1
        last = {}
        for lib in ds.ALL_LIBS:  # (Jacobi, the bound left to the library)
            last[lib] = one_then_three(hp, gpu, lib, M, B, X0, max_iter, True)[1]
        identities(hp, gpu, M, B, X0, max_iter, last, None)
        assert_same([g[:4] for g in last["mixed"]], last["batch"])
        assert_same(last["poly32"], last["poly"])
        assert_same(single_forms(hp, gpu, M, B[0], X0[0], max_iter), last["batch"][:1])
        integer_residual(hp, gpu, name, M, n)
        if name == "g65_27pt":  # four columns: the SpMM's x-triple plan on the interior slices
            B4, X4 = np.concatenate([B, B[:1] * 0.5]), np.concatenate([X0, X0[2:]])
            assert_same(run(hp, gpu, "batch", M, B4, X4, max_iter), tm.single_solves(hp, gpu, M, B4, X4, max_iter))
        if c["held"]:  # g257: a caller's m against the restatements on the host CSR
            A = ds.matrix(name)
            minv = cf.precond(c, A)[0]
            tcf.check_columns("batch", last["batch"][:1], ds.references(c, "batch"), max_iter, "oracle.hpccg")
            for lib in ("pcg", "srcg"):
                first, second = one_then_three(hp, gpu, lib, M, B, X0, max_iter, False, m=minv)
                tcf.check_columns(lib, first, ds.references(c, lib), max_iter, "first call")
                tcf.check_columns(lib, second[:1], ds.references(c, lib), max_iter, "second call")
    finally:
        M.close()
        ds.release(name)


def test_ddot_at_the_tables_row_counts(hp, gpu):
    import torch
    for n in (524837, 2097152, 2097153, 8388608, 8388609):
        assert n in [ds.nrows(k) for k in ds.NAMES]
        a = np.arange(n, dtype=np.float64) % 7 - 3.0
        b = np.arange(n, dtype=np.float64) % 5 - 2.0
        r = hp.ddot(n, torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu))
        assert r == float(np.dot(a, b)), n  # small integers: exact in any order


def test_census(hp, gpu):
    """plan(n) beside (has_a, a_width, nslices) of every shape."""
    for name in ds.NAMES:
        if name not in _census:
            M = build(hp, name)
            try:
                _census[name] = tcf.device_form(M, ds.nrows(name))
            finally:
                M.close()
    print()
    for name in ds.NAMES:
        print(f"{name}: n {ds.nrows(name)} (has_a, a_width, nslices) {_census[name]} {ds.plan(ds.nrows(name))}")
    for name in ds.NAMES:
        want = (1, 27) if name == "g65_27pt" else (1, 3)
        assert _census[name][:2] == want and _census[name][2] == ds.plan(ds.nrows(name)).nslices >= 1026, name
    assert sum(1 for name in ds.NAMES if _census[name][:2] == (1, 3) and _census[name][2] > 4096) >= 3
