/* hpccg_hip_batch.h -- batched multi-right-hand-side CG over a device matrix of
 * hpccg_hip.h (lib/libhpccg_hip_batch.so, linked against libhpccg_hip.so).
 *
 * nrhs independent systems A x_c = b_c share one pass over the matrix per
 * iteration: every value slot of the SELL-512-A (or SELL-512) image is read
 * once and multiplied into all columns. Each column is its own CG recurrence
 * (HPCCG.cpp:312-402) with its own alpha, beta, iteration count and stop;
 * a column whose loop has ended is frozen while the others go on.
 *
 * Parity promise: for finite B and X0, column c's x, niters, normr and residual
 * trace are bitwise those of hpccg_hip_solve_device(M, B(:,c), X(:,c), ...)
 * on that column alone.
 *
 * Degenerate and non-finite columns (tests/test_gpu_columns_edge.py): a column
 * has the single solve's outcome. A zero initial residual, a NaN in b or x0, or
 * an infinite x0 entry runs no iteration: niters 0, normr 0.0 (NaN for the
 * non-finite ones), x untouched. A negative tolerance from a zero residual, or
 * an infinite b entry, takes the reference's 0/0 path: niters 2, normr NaN,
 * every x NaN. The other columns of the call are bitwise unaffected, wherever
 * the bad one stands, and the call ends when they do. Nothing of it stays in
 * the workspace: the next call and hpccg_hip_batch_sparsemv give their usual
 * bits from the same vectors.
 *
 * Scope: one rank. Matrices of a communicator with more than one rank,
 * members of an in-process group and matrices with halo rows are refused with
 * HPCCG_HIP_EINVAL (message in hpccg_hip_last_error()).
 *
 * Layout: B and X are column-major, column c at B + c * ldb (doubles), with
 * ldb, ldx >= nrow; any leading dimension is accepted (the columns are copied
 * into an aligned, padded workspace that belongs to the matrix). The workspace
 * grows on demand and is freed by hpccg_hip_batch_release() or, at the latest,
 * by hpccg_hip_matrix_destroy(M): no order to remember.
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one matrix must not overlap in time. */
#ifndef HPCCG_HIP_BATCH_H
#define HPCCG_HIP_BATCH_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_batch_abi_version(void);

/* B_dev, X_dev: device pointers. X holds the initial guesses and receives the
 * solutions. niters[nrhs], normr[nrhs]: per column, as hpccg_hip_solve_device
 * returns them (a column whose loop never runs reports what the single solve
 * reports for it). max_iter < 0 is refused; 0 means 1, as in the single solve.
 * times (may be NULL) [7]: [0] the batch's wall time in seconds (device events
 * around it), [1..5] 0 (the batch keeps no per-class timers), [6] 0. */
int hpccg_hip_batch_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                                 double* X_dev, long long ldx, int max_iter, double tolerance,
                                 int* niters, double* normr, double* times);

/* The same with host pointers; times[6] is the time of the copies to and from
 * the device. */
int hpccg_hip_batch_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                          long long ldx, int max_iter, double tolerance, int* niters, double* normr,
                          double* times);

/* Residual trace of column col of the last batch solve on M (the layout of
 * hpccg_hip_last_trace: niters + 1 entries). Returns the number written, or a
 * negative error code. */
int hpccg_hip_batch_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* Y(:,c) = A X(:,c) for every column (device pointers, ldx, ldy >= nrow); each
 * column is bitwise hpccg_hip_sparsemv of that column. */
int hpccg_hip_batch_sparsemv(hpccg_hip_matrix* M, int nrhs, const double* X_dev, long long ldx,
                             double* Y_dev, long long ldy);

/* Free M's batch workspace now (it is rebuilt on the next call). */
int hpccg_hip_batch_release(hpccg_hip_matrix* M);

/* Device bytes M's batch workspace holds (0: none). */
int hpccg_hip_batch_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a batch workspace at the moment. */
int hpccg_hip_batch_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_BATCH_H */
