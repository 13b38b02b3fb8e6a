/* hpccg_hip_srcg.h -- single-reduction (Chronopoulos-Gear) preconditioned CG
 * over a device matrix of hpccg_hip.h (lib/libhpccg_hip_srcg.so, linked against
 * libhpccg_hip.so).
 *
 * nrhs independent systems A x_c = b_c are solved by preconditioned CG with
 * M^-1 = diag(m), m a positive vector of nrow entries shared by the columns; by
 * default Jacobi, m_i = 1.0 / a_ii (hpccg_hip_pcg.h's m). It is the method of
 * hpccg_hip_pcg.h in the form that needs one reduction point per iteration
 * instead of two: one more vector, s = A p, is kept by recurrence, and r.u,
 * u.w and r.r of an iteration are completed together. An iteration is three
 * kernel launches (vector step, SpMM, finalize) where hpccg_hip_pcg.h's is
 * five. Per column, all in fp64 with no contraction:
 *
 *   prologue: t = x + 0.0*x;  At = A t;  r = b + (-1.0)*At;  u = m*r;  w = A u
 *             gamma_0 = sum r_i * u_i;  delta_0 = u.w;  rr_0 = sum r_i * r_i
 *             beta_1 = 0.0;  alpha_1 = gamma_0 / delta_0
 *   k >= 1:   p = u + beta_k*p            (k == 1: u read for p)
 *             s = w + beta_k*s            (k == 1: w read for s)
 *             x = x + alpha_k*p;  r = r + (-alpha_k)*s;  u = m*r
 *             gamma_k = sum r_i * u_i;  rr_k = sum r_i * r_i
 *             w = A u;  delta_k = u.w
 *             beta_{k+1}  = gamma_k / gamma_{k-1}
 *             alpha_{k+1} = gamma_k / (delta_k - (beta_{k+1}*gamma_k) / alpha_k)
 *
 * The loop test, the residual trace, niters and the returned normr are the
 * single solve's (HPCCG.cpp:312-402), taken on rr, the recurrence's r.r, as in
 * every solver here: `tolerance` bounds the 2-norm of the residual recurrence.
 * Every dot has the single solve's summation shape, and every value slot of
 * the matrix is read once per SpMM for up to four columns, as in
 * hpccg_hip_batch.h.
 *
 * What follows from the expressions above:
 *   - The first iteration is hpccg_hip_pcg.h's bit for bit: with max_iter 0, 1
 *     or 2 and the same m, x, niters, normr and the trace are those of
 *     hpccg_hip_pcg_solve_device. With max_iter 3 the trace is still equal; x
 *     in general is not (p.Ap is replaced by delta - beta*gamma/alpha, equal in
 *     exact arithmetic only). Later iterations follow the classic recurrence to
 *     rounding: on the test matrices the r.r history agrees to 2e-10 relative
 *     and the iteration counts under a tolerance are equal.
 *   - A uniform m that is a power of two gives the bits of m = 1.0 (gamma
 *     scales by m, delta by m^2, alpha by 1/m, p by m, all exactly).
 *   - Jacobi commutes exactly with a symmetric power-of-two scaling: on
 *     a_ij s_i s_j with b_i s_i, s_i x_i is bitwise the x of A with b.
 *   - A solve runs one SpMM more than hpccg_hip_pcg.h's for the same niters:
 *     the prologue has two (A t and A u), and the last iteration's w is never
 *     used.
 *
 * Scope: one rank. Matrices of a communicator with more than one rank,
 * members of an in-process group and matrices with halo rows are refused with
 * HPCCG_HIP_EINVAL (message in hpccg_hip_last_error()).
 *
 * Degenerate and non-finite columns: the recurrence above is taken literally,
 * for any m, and niters and normr (NaN or not) are hpccg_hip_pcg.h's. A zero
 * initial residual, a NaN in b or x0, or an infinite x0 entry runs no
 * iteration: niters 0, normr 0.0 (NaN for the non-finite ones), x untouched. A
 * negative tolerance from a zero residual, or an infinite b entry, takes the
 * 0/0 path: niters 2, normr NaN, every x NaN. The other columns of the call
 * are bitwise unaffected by a degenerate one, and nothing of a bad column
 * stays in the workspace.
 *
 * Layout: B and X are column-major, column c at B + c * ldb (doubles), with
 * ldb, ldx >= nrow; the columns are copied into an aligned, padded workspace
 * that belongs to the matrix. The workspace (with the cached 1 / a_ii) grows on
 * demand and is freed by hpccg_hip_srcg_release() or, at the latest, by
 * hpccg_hip_matrix_destroy(M).
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one matrix must not overlap in time. */
#ifndef HPCCG_HIP_SRCG_H
#define HPCCG_HIP_SRCG_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_srcg_abi_version(void);

/* B_dev, X_dev: device pointers. X holds the initial guesses and receives the
 * solutions. minv_dev: nrow device doubles, every one finite and > 0 (checked
 * on the device in every call), or NULL for Jacobi: 1.0 / a_ii, taken from the
 * matrix image on first use and kept with the workspace. A row whose diagonal
 * is missing, not finite or <= 0 makes a Jacobi call fail with
 * HPCCG_HIP_EINVAL (the message names the first such row); X is untouched by a
 * refused call. niters[nrhs], normr[nrhs]: per column. max_iter < 0 is
 * refused; 0 means 1, as in the single solve.
 * times (may be NULL) [7]: [0] the solve's wall time in seconds (device events
 * around it), [1..5] 0, [6] 0. */
int hpccg_hip_srcg_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                                double* X_dev, long long ldx, const double* minv_dev, int max_iter,
                                double tolerance, int* niters, double* normr, double* times);

/* The same with host pointers (minv included); times[6] is the time of the
 * copies to and from the device. */
int hpccg_hip_srcg_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                         long long ldx, const double* minv, int max_iter, double tolerance, int* niters,
                         double* normr, double* times);

/* Residual trace (2-norm of r) of column col of the last single-reduction
 * solve on M (the layout of hpccg_hip_last_trace: niters + 1 entries). Returns
 * the number written, or a negative error code. */
int hpccg_hip_srcg_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* Free M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_srcg_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_srcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_srcg_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_SRCG_H */
