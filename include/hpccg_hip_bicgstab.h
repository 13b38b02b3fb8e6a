/* hpccg_hip_bicgstab.h -- right-preconditioned BiCGStab over a device matrix
 * of hpccg_hip.h (lib/bicgstab/libhpccg_hip_bicgstab.so, linked against
 * libhpccg_hip.so one directory up).
 *
 * Every other solver of this project is a form of CG and needs a symmetric
 * positive definite matrix: on a non-symmetric one it returns 0 and a wrong x.
 * This one solves nrhs independent systems A x_c = b_c for any square matrix
 * the recurrence does not break down on, with M^-1 = diag(m), m a positive
 * vector of nrow entries shared by the columns; by default Jacobi,
 * m_i = 1.0 / a_ii. Per column, all in fp64 with no contraction, every product
 * and sum rounded where it is written:
 *
 *   prologue: p = x + 0.0*x;  Ap = A p;  r = b + (-1.0)*Ap;  rhat = r
 *             rr_0 = sum r_i * r_i;  rho_1 = rr_0
 *   k >= 1:   beta  = 0.0 (k == 1) | (rho_k / rho_{k-1}) * (alpha / omega)
 *             p     = r + beta*(p + (-omega)*v)     (k == 1 reads r for the bracket)
 *             y_i   = m_i * p_i;  v = A y;  rv = sum rhat_i * v_i
 *             alpha = rho_k / rv
 *             s     = r + (-alpha)*v;  z_i = m_i * s_i;  t = A z
 *             ts = sum t_i * s_i;  tt = sum t_i * t_i
 *             omega = ts / tt                       (tt == 0.0: omega = 0.0)
 *             x     = (x + alpha*y) + omega*z
 *             r     = s + (-omega)*t
 *             rr_k = sum r_i * r_i;  rho_{k+1} = sum rhat_i * r_i
 *
 * The loop test, the residual trace, niters and the returned normr keep the
 * conventions of hpccg_hip_pcg.h (the single solve's, HPCCG.cpp:312-402, taken
 * on rr): iteration k + 1 runs while k + 1 < max_iter and normr > tolerance,
 * normr being sqrt(rr_{k-1}) (sqrt(rr_0) for k + 1 = 1, 2), the lagged test of
 * the reference; the trace holds niters + 1 entries, entry k the normr that
 * iteration k leaves, sqrt(rr_{k-1}) (entry 0: sqrt(rr_0)); the returned normr
 * is entry niters. Entry 0 is bitwise hpccg_hip_pcg's on the same b and x0.
 * Every dot has the single solve's summation shape, and every value slot of
 * the matrix is read twice per iteration for up to four columns.
 *
 * Two identities hold bit for bit, because a power of two commutes with every
 * rounding above (short of overflow and underflow): a uniform m = 2^e gives
 * the x and the history of m = 1.0; and Jacobi on A S, S = diag(2^e_j), gives
 * x' with s_j * x'_j the x of Jacobi on A, and the same history.
 *
 * How a column ends (hpccg_hip_bicgstab_last_status), in this order:
 *   HPCCG_HIP_BICGSTAB_CONVERGED (0)  the loop test: the tolerance or max_iter
 *   HPCCG_HIP_BICGSTAB_EXACT (2)      rr_k == 0.0 after iteration k (or in the
 *             prologue): the system is solved exactly; niters = k
 *   HPCCG_HIP_BICGSTAB_BREAKDOWN (1)  a denominator of the next step is zero:
 *             rho_{k+1} == 0.0 or omega == 0.0 after iteration k (niters = k, x
 *             and r as iteration k left them), or rv == 0.0 inside iteration k
 *             (niters = k - 1, x as iteration k - 1 left it). No division by
 *             zero is carried out, so no NaN comes of a breakdown.
 * Non-finite values get no special case: every comparison above is false for
 * a NaN, and the lagged loop test ends the column as in the CG libraries (a
 * NaN in b or x0: niters 0, x untouched; an infinite b entry: niters 2, x NaN;
 * status 0). The other columns of the call are bitwise unaffected, and nothing
 * of such a column stays in the workspace.
 *
 * Scope: one rank. Matrices of a communicator with more than one rank,
 * members of an in-process group and matrices with halo rows are refused with
 * HPCCG_HIP_EINVAL (message in hpccg_hip_last_error(), prefixed "bicgstab:").
 * No fp32 image, no left preconditioning, no BiCGStab(l), no restarts.
 *
 * Layout: B and X are column-major, column c at B + c * ldb (doubles), with
 * ldb, ldx >= nrow; the columns are copied into an aligned, padded workspace
 * that belongs to the matrix (eight vectors per column). The workspace (with
 * the cached 1 / a_ii) grows on demand and is freed by
 * hpccg_hip_bicgstab_release() or, at the latest, by hpccg_hip_matrix_destroy(M).
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one matrix must not overlap in time. */
#ifndef HPCCG_HIP_BICGSTAB_H
#define HPCCG_HIP_BICGSTAB_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HPCCG_HIP_BICGSTAB_CONVERGED 0
#define HPCCG_HIP_BICGSTAB_BREAKDOWN 1
#define HPCCG_HIP_BICGSTAB_EXACT 2

/* 1 */
int hpccg_hip_bicgstab_abi_version(void);

/* B_dev, X_dev: device pointers. X holds the initial guesses and receives the
 * solutions. minv_dev: nrow device doubles, every one finite and > 0 (checked
 * on the device in every call), or NULL for Jacobi: 1.0 / a_ii, taken from the
 * matrix image on first use and kept with the workspace. A row whose diagonal
 * is missing, not finite or <= 0 makes a Jacobi call fail with
 * HPCCG_HIP_EINVAL (the message names the first such row); X is untouched by a
 * refused call. niters[nrhs], normr[nrhs]: per column. max_iter < 0 is
 * refused; 0 means 1 (the prologue alone), as in the single solve.
 * times (may be NULL) [7]: [0] the solve's wall time in seconds (device events
 * around it), [1..5] 0, [6] 0. */
int hpccg_hip_bicgstab_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                                    double* X_dev, long long ldx, const double* minv_dev, int max_iter,
                                    double tolerance, int* niters, double* normr, double* times);

/* The same with host pointers (minv included); times[6] is the time of the
 * copies to and from the device. */
int hpccg_hip_bicgstab_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                             long long ldx, const double* minv, int max_iter, double tolerance, int* niters,
                             double* normr, double* times);

/* Residual trace (2-norm of r) of column col of the last BiCGStab solve on M
 * (the layout of hpccg_hip_last_trace: niters + 1 entries). Returns the number
 * written, or a negative error code. */
int hpccg_hip_bicgstab_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* *status: how column col of the last BiCGStab solve on M ended, one of
 * HPCCG_HIP_BICGSTAB_*. HPCCG_HIP_EINVAL where that solve had no such column
 * (an empty matrix keeps none). */
int hpccg_hip_bicgstab_last_status(const hpccg_hip_matrix* M, int col, int* status);

/* Free M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_bicgstab_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_bicgstab_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_bicgstab_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_BICGSTAB_H */
