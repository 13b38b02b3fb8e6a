/* hpccg_hip_pcg.h -- diagonally preconditioned CG over a device matrix of
 * hpccg_hip.h (lib/libhpccg_hip_pcg.so, linked against libhpccg_hip.so).
 *
 * nrhs independent systems A x_c = b_c are solved by the preconditioned
 * recurrence with M^-1 = diag(m), m a positive vector of nrow entries shared by
 * the columns; by default Jacobi, m_i = 1.0 / a_ii. Per column, all in fp64
 * with no contraction:
 *
 *   prologue: p = x + 0.0*x;  Ap = A p;  r = b + (-1.0)*Ap
 *             rz_0 = sum r_i * (m_i * r_i);   rr_0 = sum r_i * r_i
 *   k >= 1:   z_i = m_i * r_i                (never stored)
 *             p = z + beta*y                 (y = z, beta = 0.0 for k == 1, else
 *                                             y = p, beta = rz_{k-1} / rz_{k-2})
 *             Ap = A p;  alpha = rz_{k-1} / (p.Ap)
 *             x = x + alpha*p;  r = r + (-alpha)*Ap
 *             rz_k = sum r_i * (m_i * r_i);  rr_k = sum r_i * r_i
 *
 * The loop test, the residual trace, niters and the returned normr are the
 * single solve's (HPCCG.cpp:312-402), taken on rr: `tolerance` bounds the
 * 2-norm of the true residual recurrence, as in hpccg_hip_solve_device. Every
 * dot has the single solve's summation shape, and every value slot of the
 * matrix is read once per iteration for up to four columns, as in
 * hpccg_hip_batch.h. With m = 1.0 everywhere column c is bitwise
 * hpccg_hip_solve_device of that column.
 *
 * Scope: one rank. Matrices of a communicator with more than one rank,
 * members of an in-process group and matrices with halo rows are refused with
 * HPCCG_HIP_EINVAL (message in hpccg_hip_last_error()).
 *
 * Degenerate and non-finite columns (tests/test_gpu_columns_edge.py): the
 * recurrence above is taken literally, for any m. A zero initial residual, a
 * NaN in b or x0, or an infinite x0 entry (p = x + 0.0*x is NaN there) runs no
 * iteration: niters 0, normr 0.0 (NaN for the non-finite ones), x untouched. A
 * negative tolerance from a zero residual, or an infinite b entry, takes the
 * 0/0 path: niters 2, normr NaN, every x NaN. With m = 1.0 that is
 * hpccg_hip_solve_device's outcome. The other columns of the call are bitwise
 * unaffected, and nothing of a bad column stays in the workspace.
 *
 * Layout: B and X are column-major, column c at B + c * ldb (doubles), with
 * ldb, ldx >= nrow; the columns are copied into an aligned, padded workspace
 * that belongs to the matrix. The workspace (with the cached 1 / a_ii) grows on
 * demand and is freed by hpccg_hip_pcg_release() or, at the latest, by
 * hpccg_hip_matrix_destroy(M).
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one matrix must not overlap in time. */
#ifndef HPCCG_HIP_PCG_H
#define HPCCG_HIP_PCG_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_pcg_abi_version(void);

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
int hpccg_hip_pcg_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                               double* X_dev, long long ldx, const double* minv_dev, int max_iter,
                               double tolerance, int* niters, double* normr, double* times);

/* The same with host pointers (minv included); times[6] is the time of the
 * copies to and from the device. */
int hpccg_hip_pcg_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                        long long ldx, const double* minv, int max_iter, double tolerance, int* niters,
                        double* normr, double* times);

/* d_dev[i] = a_ii for the nrow rows (a device pointer), 0.0 where row i stores
 * no diagonal entry. */
int hpccg_hip_pcg_diagonal(hpccg_hip_matrix* M, double* d_dev);

/* Residual trace (2-norm of r) of column col of the last preconditioned solve
 * on M (the layout of hpccg_hip_last_trace: niters + 1 entries). Returns the
 * number written, or a negative error code. */
int hpccg_hip_pcg_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* Free M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_pcg_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_pcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_pcg_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_PCG_H */
