"""What the BiCGStab tests share (test_bicgstab_cpu.py, test_gpu_bicgstab.py):
the NumPy restatement of include/hpccg_hip_bicgstab.h, the non-symmetric test
matrices and the window of iterations on which the solver is held to the
restatement.

The restatement follows the header statement by statement over
oracle.sparsemv and a fixed-order (sequential) float64 dot; `dot` takes another
order, for the restatement's own error. hist[k] = rr_k; trace[k] is the normr
iteration k leaves, sqrt(rr_{k-1}) (trace[0] = sqrt(rr_0)), as in every solver
here; status: 0 the loop test, 1 breakdown, 2 an exactly zero residual.

The matrices (all with b = A 1):
  convect(nx, ny, nz, s7, eps)   oracle.generate's structure, off-diagonals
                  -1 + eps sign(j - i): 16c, 33c (71 slices, two dot groups),
                  12x10x16_7pt (a tail slice), 1x40x3, 1x1x1
  dominant16      values_cases.dominant(16, 16, 16, False, sym=False, ...)
  band600s, csr513s, csr3000s    test_gpu_mixed's band600 and dyadic random_spd
                  with column j scaled by 2^e_j, e_j random in [-3, 3]:
                  per-slice widths; the int32-column image

The window W of a matrix and an m: BiCGStab's residual is not monotone and the
recurrence amplifies rounding faster than CG's, so the r.r history is compared
on the longest prefix on which the restatement agrees with itself, under the
sequential dot and under numpy's blocked one, within RTRANS_RTOL_1GPU / 10 --
the tenth leaves the GPU tolerance room for the device's third order -- cut
where r.r falls under RTRANS_CUTOFF of its start. Measured (m = 1 / Jacobi):
16c 17 / 17, 33c 16 / 16, band600s 19-21, csr513s 15-18, csr3000s 19-23 (cut
at 13 under Jacobi), 12x10x16_7pt cut at 6, 1x40x3 cut at 5.
"""
import numpy as np

import oracle
import test_gpu_mixed as tm
import test_gpu_pcg as tp
import values_cases as vc
from conftest import RTRANS_CUTOFF, RTRANS_RTOL_1GPU

CONVECT = {
    "16c": (16, 16, 16, False, 0.25),
    "33c": (33, 33, 33, False, 0.25),
    "12x10x16_7pt": (12, 10, 16, True, 0.75),
    "1x40x3": (1, 40, 3, False, 0.5),
    "1x1x1": (1, 1, 1, False, 0.25),
}
SCALED = ["band600s", "csr513s", "csr3000s"]
TABLE = list(CONVECT) + ["dominant16"] + SCALED
MKINDS = ("one", "jacobi")
WINDOW_ITERS = 32  # the restatement's iterations a window is looked for in


def blocked_dot(x, y):
    return np.float64(np.dot(x, y))


def restated_bicg(A, b, m, max_iter, tol=0.0, x0=None, dot=oracle.ddot):
    """(x, niters, normr, trace, hist, status)"""
    with np.errstate(all="ignore"):
        x = np.zeros(A.nrow) if x0 is None else np.array(x0, np.float64)
        p = x + 0.0 * x
        Ap = oracle.sparsemv(A, p)
        r = b + (-1.0) * Ap
        rhat = r.copy()
        rho = np.float64(dot(r, r))
        hist = [rho]
        alpha = omega = beta = np.float64(0.0)
        v = None
        k = 0  # the iteration that has run
        if not (1 < max_iter and np.sqrt(hist[0]) > tol):
            status = 0
        elif hist[0] == 0.0:
            status = 2
        else:
            status = -1
        while status < 0:
            k += 1
            p = r + beta * (r if k == 1 else p + (-omega) * v)
            y = m * p
            v = oracle.sparsemv(A, y)
            rv = np.float64(dot(rhat, v))
            if rv == 0.0:
                k -= 1
                status = 1
                break
            alpha = rho / rv
            s = r + (-alpha) * v
            z = m * s
            t = oracle.sparsemv(A, z)
            ts = np.float64(dot(t, s))
            tt = np.float64(dot(t, t))
            omega = np.float64(0.0) if tt == 0.0 else ts / tt
            x = (x + alpha * y) + omega * z
            r = s + (-omega) * t
            hist.append(np.float64(dot(r, r)))
            rho_new = np.float64(dot(rhat, r))
            if not (k + 1 < max_iter and np.sqrt(hist[k - 1]) > tol):
                status = 0
            elif hist[k] == 0.0:
                status = 2
            elif rho_new == 0.0 or omega == 0.0:
                status = 1
            else:
                beta = (rho_new / rho) * (alpha / omega)
            rho = rho_new
        hist = np.array(hist)
        trace = np.sqrt(np.concatenate([hist[:1], hist[:k]]))
    return x, k, float(trace[k]), trace, hist, status


# ---------------------------------------------------------------------------
# the matrices
# ---------------------------------------------------------------------------
def convect(nx, ny, nz, s7, eps):
    G = oracle.generate(nx, ny, nz, use_7pt=s7)
    rows = tp.rows_of(G)
    c = G.cols.astype(np.int64)
    vals = np.where(rows == c, G.vals, -1.0 + eps * np.sign(c - rows))
    return tm.finish(G.row_ptr, G.cols, vals)


def column_scale(n, seed=78):
    return 2.0 ** np.random.default_rng(seed).integers(-3, 4, n)


def column_scaled(A, s):
    """Every entry a_ij s_j, b = A' 1."""
    return tm.finish(A.row_ptr, A.cols, A.vals * s[A.cols.astype(np.int64)])


def block_diagonal(blocks):
    """The block-diagonal CSR of (row_ptr, cols, vals) blocks, b = A 1."""
    rp, cols, vals, n0 = [np.zeros(1, np.int64)], [], [], 0
    for brp, bc, bv in blocks:
        rp.append(np.asarray(brp[1:], np.int64) + rp[-1][-1])
        cols.append(np.asarray(bc, np.int64) + n0)
        vals.append(np.asarray(bv, np.float64))
        n0 += len(brp) - 1
    return tm.finish(np.concatenate(rp), np.concatenate(cols), np.concatenate(vals))


def two_by_two():
    """[[1, 2], [0, 1]]: with b = (1, -1) and x0 = 0, rhat.v is 0 at k = 1."""
    return np.array([0, 2, 3], np.int64), np.array([0, 1, 1], np.int32), np.array([1.0, 2.0, 1.0])


_csrs = {}


def unscaled(name):
    """The matrix a SCALED entry is the column scaling of."""
    key = "base_" + name
    if key not in _csrs:
        _csrs[key] = tp.base_csr({"band600s": "band600", "csr513s": "dyadic_csr513", "csr3000s": "dyadic_csr3000"}[name])
    return _csrs[key]


def csr_of(name):
    if name not in _csrs:
        if name in CONVECT:
            _csrs[name] = convect(*CONVECT[name])
        elif name == "dominant16":
            _csrs[name] = vc.dominant(16, 16, 16, False, False, True, 41)
        elif name == "breakdown":
            G = csr_of("16c")
            _csrs[name] = block_diagonal([two_by_two(), (G.row_ptr, G.cols, G.vals)])
        else:
            A0 = unscaled(name)
            _csrs[name] = column_scaled(A0, column_scale(A0.nrow))
    return _csrs[name]


def scaled_pair(name):
    """(A, A S, s) for S = diag(2^e_j): a CONVECT entry with its column scaling,
    or a SCALED entry with the matrix it is the scaling of."""
    if name in SCALED:
        A0 = unscaled(name)
        return A0, csr_of(name), column_scale(A0.nrow)
    A0 = csr_of(name)
    s = column_scale(A0.nrow)
    if name + "@s" not in _csrs:
        _csrs[name + "@s"] = column_scaled(A0, s)
    return A0, _csrs[name + "@s"], s


def minv_of(A, kind):
    return np.ones(A.nrow) if kind == "one" else 1.0 / tp.csr_diagonal(A)


# ---------------------------------------------------------------------------
# the window
# ---------------------------------------------------------------------------
def agreeing_prefix(h1, h2, rtol):
    """(W, cut): the longest prefix of history h1 that h2 agrees with within
    rtol, ended (cut) where h1 falls under RTRANS_CUTOFF of its start."""
    for k in range(min(len(h1), len(h2))):
        if h1[k] < RTRANS_CUTOFF * h1[0]:
            return k, True
        if not abs(h2[k] - h1[k]) <= rtol * h1[k]:
            return k, False
    return min(len(h1), len(h2)), False


_windows = {}


def window(name, kind, b=None, x0=None, key=None):
    """(W, cut, sequential restatement, blocked restatement) of a table entry
    under m = kind, on (b, x0) (the generated b from zero by default; key names
    another pair in the cache)."""
    ck = (name, kind, key)
    if ck not in _windows:
        A = csr_of(name)
        m = minv_of(A, kind)
        b = A.b if b is None else b
        seq = restated_bicg(A, b, m, WINDOW_ITERS, x0=x0)
        blk = restated_bicg(A, b, m, WINDOW_ITERS, x0=x0, dot=blocked_dot)
        W, cut = agreeing_prefix(seq[4], blk[4], RTRANS_RTOL_1GPU / 10)
        _windows[ck] = (W, cut, seq, blk)
    return _windows[ck]
