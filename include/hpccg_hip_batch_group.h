/* hpccg_hip_batch_group.h -- the batched multi-right-hand-side CG of
 * hpccg_hip_batch.h over an in-process rank group of hpccg_hip.h
 * (hpccg_hip_group_generate, hpccg_hip_group_create_csr): member r is rank r of
 * a z-slab job on its own device. Implemented in lib/libhpccg_hip_batch.so.
 *
 * Every member runs the batch kernels on its rows of every column; per
 * iteration the ghost planes of every column's p are copied between
 * neighbouring members, and the two dots of every column are the members'
 * local totals added in rank order (the group solve's sum). All members see
 * the same per-column alpha, beta and stop, so a column whose loop has ended
 * is frozen on every member while the others go on.
 *
 * Parity promise: for finite B and X0, column c -- every member's x, niters,
 * normr and the residual trace -- is bitwise hpccg_hip_group_solve of that
 * column alone on the same members. A degenerate or non-finite column (see
 * hpccg_hip_batch.h) has hpccg_hip_group_solve's outcome on every member --
 * niters 0 with x untouched, or niters 2 with every x NaN -- also where the bad
 * entry lies on a plane a neighbour reads; the other columns are bitwise
 * unaffected (a frozen column's ghost planes are copied, never used), and
 * nothing of it stays in the members' workspaces
 * (tests/test_gpu_columns_edge.py).
 *
 * Scope: the whole group in rank order (Ms[r] is member r, nranks the group's
 * size), members of the z-slab halo plan with a SELL-512-A or SELL-512 image.
 * Refused before any device work, the caller's X untouched and its current
 * device kept: members of the gather plan (HPCCG_HIP_EPLAN); a wrong nranks,
 * members of different groups, a member not at its own rank, nrhs <= 0,
 * max_iter < 0, a leading dimension below a member's nrow, NULL arguments
 * (HPCCG_HIP_EINVAL). nranks == 1 is the single-rank batch of hpccg_hip_batch.h;
 * nrhs == 1 is hpccg_hip_group_solve. The functions of hpccg_hip_batch.h keep
 * refusing the members of a group of more than one rank.
 *
 * The workspace is one batch workspace per member, owned by the member matrix:
 * hpccg_hip_batch_workspace_bytes, hpccg_hip_batch_release and
 * hpccg_hip_batch_live_workspaces account for it, and it goes with the matrix
 * at the latest. The members' own solve vectors are never touched: a
 * hpccg_hip_group_solve before or after gives its usual bits.
 *
 * Members on different devices use peer copies and peer stores of the column
 * state; that path has not been run (it needs more than one GPU).
 *
 * Error codes are those of hpccg_hip.h; calls on one group must not overlap. */
#ifndef HPCCG_HIP_BATCH_GROUP_H
#define HPCCG_HIP_BATCH_GROUP_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_group_batch_abi_version(void);

/* B_dev[r], X_dev[r]: member r's local rows on its device, column-major,
 * column c at B_dev[r] + c * ldb[r]; ldb[r], ldx[r] >= member r's nrow.
 * X in/out. niters[nrhs], normr[nrhs] per column. times (may be NULL) [7]:
 * [0] wall seconds from device events on member 0's stream, the rest 0. */
int hpccg_hip_group_batch_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs,
                                       const double* const* B_dev, const long long* ldb,
                                       double* const* X_dev, const long long* ldx, int max_iter,
                                       double tolerance, int* niters, double* normr, double* times);

/* Y(:,c) = A X(:,c) of the global matrix, rows split over the members like X
 * (the halo of X is exchanged inside). Each row sum adds its products in the
 * matrix's slot order with no contraction. */
int hpccg_hip_group_batch_sparsemv(hpccg_hip_matrix* const* Ms, int nranks, int nrhs,
                                   const double* const* X_dev, const long long* ldx,
                                   double* const* Y_dev, const long long* ldy);

/* Residual trace of column col of the last group batch solve (one set of
 * all-reduced scalars: the same for every member). Returns the number of
 * entries written, or a negative error code. */
int hpccg_hip_group_batch_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out,
                                     int cap);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_BATCH_GROUP_H */
