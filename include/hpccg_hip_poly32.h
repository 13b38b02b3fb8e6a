/* hpccg_hip_poly32.h -- Chebyshev polynomial preconditioned CG whose
 * polynomial steps stream an fp32 image of the matrix (lib/libhpccg_hip_poly32.so,
 * linked against libhpccg_hip.so).
 *
 * This is the recurrence of hpccg_hip_poly.h, statement for statement -- the
 * host expressions of the Chebyshev scalars, step 0, step j, the prologue, the
 * iteration, the loop test, the trace, every dot's summation shape -- with two
 * differences.
 *
 * 1. The steps read the fp32 image. Let A~ be the matrix with every stored
 *    value rounded to float (element by element, round to nearest). In step j
 *      w_i = (A~ z)_i
 *    summed in slot order, each value widened to double in the register; every
 *    vector, product and sum is fp64 with no contraction. m (Jacobi's 1.0 / a_ii
 *    or the caller's), the Chebyshev scalars and the Gershgorin bound are fp64
 *    and come from the fp64 image, as in hpccg_hip_poly.h.
 *    Why this is safe: rounding an entry and its transpose gives the same
 *    value, so A~ is symmetric and P, a polynomial in diag(m) A~ times diag(m),
 *    is a fixed symmetric operator: CG on the fp64 system keeps its theory and
 *    converges to the fp64 answer; no refinement loop is needed (compare
 *    hpccg_hip_mixed.h, where the image is the system's operator). Within fp32
 *    range |a~_ij - a_ij| <= 2^-24 |a_ij|, so the symmetric Gershgorin bound of
 *    A~ is at most (1 + 2^-24) lmax; P is positive on (0, lmax + lmin), and the
 *    default lmin = lmax / 30 covers the excess many times over. A caller's own
 *    bounds are NOT verified, as in hpccg_hip_poly.h.
 *
 * 2. The outer SpMM (Ap = A p) streams the fp32 image only where the image is
 *    the matrix: where every stored value survives double -> float -> double
 *    ("exact": the conversion counts no inexact value; the generated stencils,
 *    anything scaled by powers of two). Otherwise it streams the fp64 image
 *    with the loops of hpccg_hip_poly.h's library. The system solved is
 *    therefore always the fp64 one, and normr is its residual's recurrence.
 *
 * Consequences:
 *   exact image         every column is bitwise hpccg_hip_poly_solve_device at
 *                       every degree: x, niters, normr and the trace.
 *   any image, degree 0 bitwise hpccg_hip_pcg_solve_device with the same m.
 *   inexact image,      the same recurrence with A~ inside P; it converges to
 *   degree >= 1         the fp64 tolerance on the fp64 residual.
 *   out of fp32 range   a stored value whose fp32 image is not finite, or that
 *                       is nonzero and below FLT_MIN in magnitude: every solve
 *                       and the info call are refused with HPCCG_HIP_EINVAL
 *                       ("outside fp32 range"); X is untouched.
 *   degenerate and      the recurrence is taken literally, as in
 *   non-finite columns  hpccg_hip_pcg.h; the other columns of the call are
 *                       bitwise unaffected, and nothing of a bad column stays in
 *                       the workspace.
 *
 * Memory. The library holds its own fp32 image, built on the device on first
 * use: exactly 4 bytes per stored slot of the image the matrix holds (864 MB
 * for the 27-point stencil at 200^3), beside the mixed library's image if both
 * libraries are used on one matrix. The info call reports the size; release
 * frees it with the workspace.
 *
 * Scope: one rank. Matrices of a communicator with more than one rank,
 * members of an in-process group and matrices with halo rows are refused with
 * HPCCG_HIP_EINVAL (message in hpccg_hip_last_error()).
 *
 * Layout, spectrum defaults, error codes: those of hpccg_hip_poly.h. Every
 * function returns 0 on success unless stated otherwise. Calls on one matrix
 * must not overlap in time. */
#ifndef HPCCG_HIP_POLY32_H
#define HPCCG_HIP_POLY32_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_poly32_abi_version(void);

/* The parameters of the fp64 polynomial solve on device pointers. B_dev,
 * X_dev: column-major, column c at B_dev + c * ldb. X holds the initial guesses
 * and receives the solutions. minv_dev: nrow device doubles, every one finite
 * and > 0 (checked on the device in every call), or NULL for Jacobi. degree: 0
 * to 16. lmin, lmax: the interval (0.0: the symmetric Gershgorin bound of the
 * fp64 image, and lmax / 30). A matrix outside fp32 range, a bad diagonal, a
 * bad m, a bad degree or bad bounds make the call fail with HPCCG_HIP_EINVAL; X
 * is untouched by a refused call. niters[nrhs], normr[nrhs]: per column.
 * max_iter < 0 is refused; 0 means 1, as in the single solve.
 * times (may be NULL) [7]: [0] the solve's wall time in seconds (device events
 * around it), [1..5] 0, [6] 0. */
int hpccg_hip_poly32_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                                  double* X_dev, long long ldx, const double* minv_dev, int degree,
                                  double lmin, double lmax, int max_iter, double tolerance, int* niters,
                                  double* normr, double* times);

/* The same with host pointers (minv included); times[6] is the time of the
 * copies to and from the device. */
int hpccg_hip_poly32_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                           long long ldx, const double* minv, int degree, double lmin, double lmax,
                           int max_iter, double tolerance, int* niters, double* normr, double* times);

/* *lmax = the symmetric Gershgorin bound of the fp64 image for m = minv_dev
 * (nrow device doubles, checked), or for Jacobi where minv_dev is NULL (0.0 for
 * a matrix without rows): the value the fp64 polynomial library computes. */
int hpccg_hip_poly32_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax);

/* The interval the last solve of this library on M used (degree 0: the
 * arguments as resolved without the device, 0.0 where none was given). */
int hpccg_hip_poly32_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax);

/* Residual trace (2-norm of r) of column col of the last solve of this library
 * on M (the layout of hpccg_hip_last_trace: niters + 1 entries). Returns the
 * number written, or a negative error code. */
int hpccg_hip_poly32_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* The fp32 image of M (built on first use). out[0]: 1 where the image is exact
 * (it is the matrix), else 0; out[1]: device bytes of the image; out[2]: stored
 * values that did not survive the round trip through float; out[3]: 0. */
int hpccg_hip_poly32_info(hpccg_hip_matrix* M, long long out[4]);

/* Free M's workspace of this library now, the fp32 image included (both are
 * rebuilt on the next call). hpccg_hip_matrix_destroy(M) does it at the latest. */
int hpccg_hip_poly32_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds, the image included (0: none). */
int hpccg_hip_poly32_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_poly32_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_POLY32_H */
