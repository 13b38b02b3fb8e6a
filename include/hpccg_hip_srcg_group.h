/* hpccg_hip_srcg_group.h -- the single-reduction (Chronopoulos-Gear)
 * preconditioned CG of hpccg_hip_srcg.h over an in-process rank group of
 * hpccg_hip.h (hpccg_hip_group_generate, hpccg_hip_group_create_csr): member r
 * is rank r of a z-slab job on its own device. Implemented in
 * lib/libhpccg_hip_srcg_group.so (linked against libhpccg_hip.so), a library of
 * its own beside the ten others.
 *
 * Per column the recurrence is exactly the one written in hpccg_hip_srcg.h,
 * with M^-1 = diag(m) and by default Jacobi, m_i = 1.0 / a_ii. Every member
 * runs it on its rows of every column; per iteration the ghost planes of every
 * column's u = m r move between neighbouring members (one kernel launch per
 * member), and the three dots of every column -- r.r, r.u and u.w -- are the
 * members' local totals added in rank order from 0.0, all three in ONE sum over
 * the members (hpccg_hip_pcg_group.h needs two per iteration: p.Ap, then r.z
 * with r.r). All members see the same per-column alpha, beta and stop, so a
 * column whose loop has ended is frozen on every member while the others go on.
 * The tolerance, niters, normr and the residual trace stay on the 2-norm of r.
 *
 * What follows from the expressions of hpccg_hip_srcg.h:
 *   - The first iteration is hpccg_hip_pcg_group.h's bit for bit: with max_iter
 *     0, 1 or 2 and the same m, every member's x, niters, normr and the trace
 *     are those of hpccg_hip_group_pcg_solve_device on the same members; with
 *     max_iter 3 the trace is still equal.
 *   - A group of one (or a plain one-rank matrix) is bitwise
 *     hpccg_hip_srcg_solve_device.
 *   - A uniform power-of-two m gives the bits of m = 1.0; Jacobi commutes
 *     exactly with a symmetric power-of-two scaling.
 *   - Column c of a call is bitwise the call with that column alone.
 *
 * Jacobi needs no communication: a member's image holds a_ii of each of its
 * rows (hpccg_hip_group_pcg_diagonal reads them). A row whose diagonal is
 * missing, not finite or <= 0 on any member makes a Jacobi call fail with
 * HPCCG_HIP_EINVAL (the message names the member and its first such row,
 * counted from the member's first row); a caller's m is checked on every member
 * in every call in the same way. Such a call is refused before any column is
 * staged: every X is left untouched.
 *
 * A degenerate or non-finite column ends with hpccg_hip_pcg_group.h's niters
 * and normr on every member; the other columns are bitwise unaffected, and
 * nothing of it stays in the members' workspaces.
 *
 * Scope: the whole group in rank order (Ms[r] is member r, nranks the group's
 * size), members of the z-slab halo plan with a SELL-512-A or SELL-512 image;
 * one device has been tested. Refused before any device work, the caller's X
 * untouched and its current device kept: members of the gather plan
 * (HPCCG_HIP_EPLAN); a wrong nranks, members of different groups, a member not
 * at its own rank, a member without rows, nrhs <= 0, max_iter < 0, a leading
 * dimension below a member's nrow, NULL arguments (HPCCG_HIP_EINVAL).
 * nranks == 1 runs the same code on a halo-free matrix, and nrhs == 1 the
 * one-column kernels: nothing is forwarded to another library. The functions of
 * hpccg_hip_srcg.h keep refusing the members of a group.
 *
 * The workspace is one per member, owned by the member matrix: the columns (u
 * with the member's ghost planes, p, s), the member's cached 1 / a_ii with its
 * verdict, and room for a caller's m. It grows on demand and is freed by
 * hpccg_hip_group_srcg_release() or, at the latest, with the matrix. The
 * members' own solve vectors and their workspaces of the other libraries are
 * never touched: those solves give their usual bits before and after.
 *
 * Members on different devices: the halo kernel and the column-state stores go
 * through peer pointers, and a caller's m is copied on the member's stream.
 * That path has not been run (it needs more than one GPU).
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one group must not overlap in time. */
#ifndef HPCCG_HIP_SRCG_GROUP_H
#define HPCCG_HIP_SRCG_GROUP_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_group_srcg_abi_version(void);

/* B_dev[r], X_dev[r]: member r's local rows on its device, column-major,
 * column c at B_dev[r] + c * ldb[r]; ldb[r], ldx[r] >= member r's nrow. X
 * in/out. minv_dev: NULL for Jacobi on every member; else minv_dev[r] is member
 * r's nrow device doubles, every one finite and > 0 (every minv_dev[r] must be
 * non-NULL). niters[nrhs], normr[nrhs] per column. max_iter < 0 is refused; 0
 * means 1. times (may be NULL) [7]: [0] wall seconds from device events on
 * member 0's stream, the rest 0. */
int hpccg_hip_group_srcg_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs,
                                      const double* const* B_dev, const long long* ldb,
                                      double* const* X_dev, const long long* ldx,
                                      const double* const* minv_dev, int max_iter, double tolerance,
                                      int* niters, double* normr, double* times);

/* Residual trace (2-norm of r) of column col of the last group solve of this
 * library (one set of all-reduced scalars: the same for every member). Returns
 * the number of entries written, or a negative error code. */
int hpccg_hip_group_srcg_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out,
                                    int cap);

/* Free member M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_group_srcg_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_group_srcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_group_srcg_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_SRCG_GROUP_H */
