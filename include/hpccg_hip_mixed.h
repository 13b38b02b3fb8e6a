/* hpccg_hip_mixed.h -- mixed-precision CG over a device matrix of hpccg_hip.h
 * (lib/libhpccg_hip_mixed.so, linked against libhpccg_hip.so).
 *
 * The matrix values are held a second time in fp32 (4 B per value slot; the
 * fp64 image stays); every vector and every operation is fp64: a value is
 * widened to double in the register before it is multiplied. The solver is
 * bound by the value stream, and this halves it.
 *
 * exact (hpccg_hip_mixed_info): every stored value survives the round trip
 * double -> float -> double. Then the fp32 image is the matrix, and column c's
 * x, niters, normr and residual trace are, for finite B and X0, bitwise those
 * of hpccg_hip_solve_device(M, B(:,c), X(:,c), max_iter, tolerance, ...);
 * max_sweeps and inner_rtol are ignored. The generated stencils are exact.
 *
 * Otherwise the solve is an iterative refinement against the fp64 matrix A,
 * with the fp32 image A~ as the inner operator. Per column, with
 * left = max(max_iter, 1) - 1 inner iterations to spend and s = 0:
 *   1. r_s = b - A x_s in fp64, rho_s = sqrt(r_s . r_s)
 *   2. stop if rho_s <= tolerance, or rho_s is not finite (NaN, inf), or
 *      rho_s == 0.0 (whatever the tolerance, a negative one too), or
 *      s == max_sweeps, or left == 0. There is no further sweep: normr is that
 *      rho_s and x is x_s as it stands -- at s = 0 the caller's x0 bit for bit,
 *      the signs of its zeros included
 *   3. the CG recurrence (HPCCG.cpp:312-402) on A~ d = r_s from d = 0, stopped
 *      at max(tolerance, inner_rtol * rho_s) or after left iterations (it_s)
 *   4. x_{s+1} = x_s + d, left -= it_s, s += 1
 * niters is the sum of the it_s. normr is the last rho: the fp64 residual norm
 * ||b - A x|| of the returned x against the fp64 matrix, NOT a value of the
 * recurrence (which is what hpccg_hip_solve_device returns).
 *
 * Assumption: A~ is symmetric positive definite like A. A matrix whose
 * smallest eigenvalue lies below the fp32 rounding perturbation (about
 * 6e-8 * ||A||) may lose that; a breakdown of the inner recurrence is not
 * detected specially, and the returned normr tells the truth about x.
 *
 * Every column is independent: column c of a multi-column call is bitwise the
 * single-column call on it. A column that has stopped is frozen while the
 * others go on.
 *
 * Degenerate and non-finite columns (tests/test_gpu_columns_edge.py). An exact
 * matrix: the column has hpccg_hip_solve_device's outcome -- a zero initial
 * residual, a NaN in b or x0 or an infinite x0 entry: niters 0, normr 0.0 (NaN
 * for the non-finite ones), x untouched; a negative tolerance from a zero
 * residual or an infinite b entry: the reference's 0/0 path, niters 2, normr
 * NaN, every x NaN. The refinement does NOT take the reference's NaN path: by
 * step 2 each of these columns ends at its first residual step with niters 0,
 * no sweep (resid has its one entry), normr rho_0 (0.0, NaN or inf) and x0
 * returned bit for bit -- where the fp64 single solve returns niters 2 and a
 * NaN x for an infinite b entry or a negative tolerance, the refinement
 * returns niters 0 and x0. Either way the other columns of the call are
 * bitwise unaffected, and nothing of a bad column stays in the workspace: the
 * next call and hpccg_hip_mixed_sparsemv give their usual bits.
 *
 * Values outside fp32 range: a stored value whose fp32 image is not finite, or
 * that is nonzero with |v| < FLT_MIN, makes every mixed call on that matrix
 * return HPCCG_HIP_EINVAL ("outside fp32 range"); X is left untouched.
 *
 * Scope: one rank. Matrices of a communicator with more than one rank, members
 * of an in-process group and matrices with halo rows are refused with
 * HPCCG_HIP_EINVAL (message in hpccg_hip_last_error()).
 *
 * Layout: B and X are column-major, column c at B + c * ldb (doubles), with
 * ldb, ldx >= nrow; the columns are copied into a padded workspace that belongs
 * to the matrix, and nothing is stored between the caller's columns. The
 * workspace (the fp32 image included) is freed by hpccg_hip_mixed_release() or,
 * at the latest, by hpccg_hip_matrix_destroy(M).
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one matrix must not overlap in time. */
#ifndef HPCCG_HIP_MIXED_H
#define HPCCG_HIP_MIXED_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_mixed_abi_version(void);

/* B_dev, X_dev: device pointers. X holds the initial guesses and receives the
 * solutions. niters[nrhs], normr[nrhs]: per column (see above). max_iter < 0 is
 * refused; 0 means 1. max_sweeps >= 1. inner_rtol in [0, 1); a negative value
 * selects the default, 2^-20. times (may be NULL) [7]: [0] the solve's wall
 * time in seconds (device events around it), [1..5] 0, [6] 0. n == 0 returns
 * at once. */
int hpccg_hip_mixed_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb,
                                 double* X_dev, long long ldx, int max_iter, double tolerance,
                                 int max_sweeps, double inner_rtol, int* niters, double* normr,
                                 double* times);

/* The same with host pointers; times[6] is the time of the copies to and from
 * the device. */
int hpccg_hip_mixed_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X,
                          long long ldx, int max_iter, double tolerance, int max_sweeps,
                          double inner_rtol, int* niters, double* normr, double* times);

/* Y(:,c) = A~ X(:,c) for every column, A~ being the fp32 image (device
 * pointers, ldx, ldy >= nrow): the fp64 row sums of the widened values in the
 * matrix's slot order. */
int hpccg_hip_mixed_sparsemv(hpccg_hip_matrix* M, int nrhs, const double* X_dev, long long ldx,
                             double* Y_dev, long long ldy);

/* out: [0] exact (1 / 0), [1] device bytes of the fp32 image, [2] device bytes
 * of the rest of the mixed workspace, [3] stored values that did not survive
 * the round trip. Builds the image if there is none yet. */
int hpccg_hip_mixed_info(hpccg_hip_matrix* M, long long out[4]);

/* The inner recurrence's normr of column col of the last mixed solve on M:
 * every sweep contributes its it_s + 1 entries in order (one sweep: the layout
 * of hpccg_hip_last_trace). Returns the number written, or a negative error
 * code. */
int hpccg_hip_mixed_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap);

/* The sweeps of column col of the last mixed solve on M: iters[s] = it_s and
 * resid[s] = rho_s, the fp64 residual norm before sweep s; resid has one more
 * entry, the final residual (normr). An exact matrix: one sweep, resid[0] and
 * resid[1] are the recurrence's first and last normr. Writes at most cap
 * entries of each; returns the number of sweeps, or a negative error code. */
int hpccg_hip_mixed_last_sweeps(const hpccg_hip_matrix* M, int col, int* iters, double* resid, int cap);

/* Free M's mixed workspace and fp32 image now (rebuilt on the next call). */
int hpccg_hip_mixed_release(hpccg_hip_matrix* M);

/* Device bytes M's mixed workspace holds, the fp32 image included (0: none). */
int hpccg_hip_mixed_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a mixed workspace at the moment. */
int hpccg_hip_mixed_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_MIXED_H */
