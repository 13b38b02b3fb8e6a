/* hpccg_hip_poly.h -- Chebyshev polynomial preconditioned CG over a device
 * matrix of hpccg_hip.h (lib/libhpccg_hip_poly.so, linked against
 * libhpccg_hip.so).
 *
 * nrhs independent systems A x_c = b_c are solved by the preconditioned
 * recurrence of hpccg_hip_pcg.h with z = P(r) in place of z = m r: P is the
 * Chebyshev iteration of `degree` steps for M^-1 A on the interval
 * [lmin, lmax], started from zero, with M^-1 = diag(m), m a positive vector of
 * nrow entries shared by the columns; by default Jacobi, m_i = 1.0 / a_ii.
 * degree = d >= 0 is the number of extra passes over the matrix per
 * application. All in fp64 with no contraction.
 *
 * Host, in double, exactly these expressions:
 *   theta = 0.5*(lmax+lmin);  delta = 0.5*(lmax-lmin);  sigma = theta/delta
 *   rho_0 = 1.0/sigma;  c0 = 1.0/theta
 *   j = 1..d:  rho_j = 1.0/(2.0*sigma - rho_{j-1});  a_j = rho_j*rho_{j-1}
 *              b_j = 2.0*rho_j/delta
 * Device, z = P(r), per row i:
 *   d == 0:   z_i = m_i*r_i                       (exactly hpccg_hip_pcg.h's z)
 *   step 0:   t = m_i*r_i;  dd_i = c0*t;  z_i = dd_i
 *   step j:   w_i = (A z)_i                       (the SpMM's row sum, slot order)
 *             t = m_i*(r_i - w_i);  dd_i = a_j*dd_i + b_j*t;  z_i = z_i + dd_i
 * Around it, per column:
 *   prologue: p = x + 0.0*x;  Ap = A p;  r = b + (-1.0)*Ap;  z = P(r)
 *             rz_0 = sum r_i * z_i;   rr_0 = sum r_i * r_i
 *   k >= 1:   p = z + beta*y                 (y = z, beta = 0.0 for k == 1, else
 *                                             y = p, beta = rz_{k-1} / rz_{k-2})
 *             Ap = A p;  alpha = rz_{k-1} / (p.Ap)
 *             x = x + alpha*p;  r = r + (-alpha)*Ap;  z = P(r)
 *             rz_k = sum r_i * z_i;  rr_k = sum r_i * r_i
 * The loop test, the residual trace, niters and the returned normr are the
 * single solve's (HPCCG.cpp:312-402), taken on rr, as in hpccg_hip_pcg.h;
 * every dot has the single solve's summation shape.
 *
 * P is a fixed polynomial in M^-1 A times M^-1, positive on (0, lmax + lmin):
 * the preconditioner is symmetric positive definite whenever lmax bounds the
 * spectrum of M^-1 A. Degree 0 is bitwise hpccg_hip_pcg_solve_device with the
 * same m (with m = 1.0 everywhere: hpccg_hip_solve_device of each column).
 *
 * The spectrum. lmax == 0.0 means the symmetric Gershgorin bound, computed on
 * the device: with q_i = sqrt(m_i),
 *   lmax = max_i q_i * sum_j |a_ij|*q_j     (summed in slot order)
 * which bounds the spectrum of M^-1/2 A M^-1/2 and so that of M^-1 A. For
 * Jacobi it is computed once and kept with 1 / a_ii; for a caller's m it is
 * computed in every call that passes lmax == 0.0. lmin == 0.0 means
 * lmax / 30, the conventional eigenvalue ratio of Chebyshev smoothers. A
 * caller's own bounds are NOT verified: an lmax below the spectrum's top makes
 * P indefinite and the recurrence meaningless, without an error. Negative or
 * non-finite bounds and lmin >= lmax are refused. With degree 0 the bounds are
 * checked but not used, and none is computed.
 *
 * Scope: one rank. Matrices of a communicator with more than one rank,
 * members of an in-process group and matrices with halo rows are refused with
 * HPCCG_HIP_EINVAL (message in hpccg_hip_last_error()).
 *
 * Degenerate and non-finite columns: the recurrence is taken literally, as in
 * hpccg_hip_pcg.h; the other columns of the call are bitwise unaffected, and
 * nothing of a bad column stays in the workspace.
 *
 * Layout: B and X are column-major, column c at B + c * ldb (doubles), with
 * ldb, ldx >= nrow; the columns are copied into an aligned, padded workspace
 * that belongs to the matrix. The workspace (with the cached 1 / a_ii and its
 * bound) grows on demand and is freed by hpccg_hip_poly_release() or, at the
 * latest, by hpccg_hip_matrix_destroy(M).
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one matrix must not overlap in time. */
#ifndef HPCCG_HIP_POLY_H
#define HPCCG_HIP_POLY_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_poly_abi_version(void);

/* B_dev, X_dev: device pointers. X holds the initial guesses and receives the
 * solutions. minv_dev: nrow device doubles, every one finite and > 0 (checked
 * on the device in every call), or NULL for Jacobi. degree: 0 to 16. lmin,
 * lmax: the interval (0.0: the defaults above). A bad diagonal, a bad m, a bad
 * degree or bad bounds make the call fail with HPCCG_HIP_EINVAL; X is untouched
 * by a refused call. niters[nrhs], normr[nrhs]: per column. max_iter < 0 is
 * refused; 0 means 1, as in the single solve.
 * times (may be NULL) [7]: [0] the solve's wall time in seconds (device events
 * around it), [1..5] 0, [6] 0. */
int hpccg_hip_poly_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                                double* X_dev, long long ldx, const double* minv_dev, int degree,
                                double lmin, double lmax, int max_iter, double tolerance, int* niters,
                                double* normr, double* times);

/* The same with host pointers (minv included); times[6] is the time of the
 * copies to and from the device. */
int hpccg_hip_poly_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                         long long ldx, const double* minv, int degree, double lmin, double lmax,
                         int max_iter, double tolerance, int* niters, double* normr, double* times);

/* *lmax = the symmetric Gershgorin bound above for m = minv_dev (nrow device
 * doubles, checked), or for Jacobi where minv_dev is NULL (0.0 for a matrix
 * without rows). */
int hpccg_hip_poly_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax);

/* The interval the last solve on M used (degree 0: the arguments as resolved
 * without the device, 0.0 where none was given). */
int hpccg_hip_poly_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax);

/* Residual trace (2-norm of r) of column col of the last polynomial solve on M
 * (the layout of hpccg_hip_last_trace: niters + 1 entries). Returns the number
 * written, or a negative error code. */
int hpccg_hip_poly_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* Free M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_poly_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_poly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_poly_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_POLY_H */
