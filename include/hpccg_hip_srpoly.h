/* hpccg_hip_srpoly.h -- single-reduction CG with the Chebyshev polynomial
 * preconditioner over a device matrix of hpccg_hip.h
 * (lib/libhpccg_hip_srpoly.so, linked against libhpccg_hip.so).
 *
 * nrhs independent systems A x_c = b_c are solved by the single-reduction
 * (Chronopoulos-Gear) recurrence of hpccg_hip_srcg.h with u = P(r) in place of
 * u = m r: P is hpccg_hip_poly.h's Chebyshev iteration of `degree` steps for
 * M^-1 A on [lmin, lmax], started from zero, with M^-1 = diag(m), by default
 * Jacobi, m_i = 1.0 / a_ii; its coefficients, its defaults for the interval and
 * its device expressions are that header's. All in fp64 with no contraction.
 *
 * Per column:
 *   prologue: t = x + 0.0*x;  r = b + (-1.0)*(A t);  u = P(r);  w = A u
 *             gamma_0 = sum r_i*u_i;  delta_0 = sum u_i*w_i;  rr_0 = sum r_i*r_i
 *             beta = 0.0;  alpha = gamma_0 / delta_0
 *   k >= 1:   p = u + beta*y                 (y = u for k == 1, else y = p)
 *             s = w + beta*y'                (y' = w for k == 1, else y' = s)
 *             x = x + alpha*p;  r = r + (-alpha)*s;  u = P(r);  w = A u
 *             gamma_k = sum r_i*u_i;  delta_k = sum u_i*w_i;  rr_k = sum r_i*r_i
 *             beta = gamma_k / gamma_{k-1}
 *             alpha = gamma_k / (delta_k - (beta*gamma_k) / alpha_old)
 * An iteration completes its three dots at one point, where hpccg_hip_poly.h's
 * completes two dots at two; it costs two more vectors (s, and w beside Ap).
 * The loop test, the residual trace, niters and the returned normr are the
 * single solve's (HPCCG.cpp:312-402), taken on rr; every dot has the single
 * solve's summation shape.
 *
 * Degree 0 is bitwise hpccg_hip_srcg_solve_device with the same m. With any
 * degree, x, niters, normr and the trace are bitwise
 * hpccg_hip_poly_solve_device's with the same m and interval up to
 * max_iter = 2, and the trace up to max_iter = 3; later iterations agree to
 * rounding (s = A p holds by recurrence, not by a product).
 *
 * The spectrum, a caller's bounds, the scope (one rank), degenerate and
 * non-finite columns, the layout of B and X and the workspace: as in
 * hpccg_hip_poly.h. The workspace is freed by hpccg_hip_srpoly_release() or, at
 * the latest, by hpccg_hip_matrix_destroy(M).
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one matrix must not overlap in time. */
#ifndef HPCCG_HIP_SRPOLY_H
#define HPCCG_HIP_SRPOLY_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_srpoly_abi_version(void);

/* The arguments, the refusals and `times` of hpccg_hip_poly_solve_device. */
int hpccg_hip_srpoly_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                                  double* X_dev, long long ldx, const double* minv_dev, int degree,
                                  double lmin, double lmax, int max_iter, double tolerance, int* niters,
                                  double* normr, double* times);

/* The same with host pointers (minv included); times[6] is the time of the
 * copies to and from the device. */
int hpccg_hip_srpoly_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                           long long ldx, const double* minv, int degree, double lmin, double lmax,
                           int max_iter, double tolerance, int* niters, double* normr, double* times);

/* *lmax = hpccg_hip_poly_bound's value: the symmetric Gershgorin bound for
 * m = minv_dev (nrow device doubles, checked), or for Jacobi where minv_dev is
 * NULL (0.0 for a matrix without rows). */
int hpccg_hip_srpoly_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax);

/* The interval the last solve on M used (degree 0: the arguments as resolved
 * without the device, 0.0 where none was given). */
int hpccg_hip_srpoly_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax);

/* Residual trace (2-norm of r) of column col of the last single-reduction
 * polynomial solve on M (the layout of hpccg_hip_last_trace: niters + 1
 * entries). Returns the number written, or a negative error code. */
int hpccg_hip_srpoly_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* Free M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_srpoly_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_srpoly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_srpoly_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_SRPOLY_H */
