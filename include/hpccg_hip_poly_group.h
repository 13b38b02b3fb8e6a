/* hpccg_hip_poly_group.h -- the Chebyshev polynomial preconditioned CG of
 * hpccg_hip_poly.h over an in-process rank group of hpccg_hip.h
 * (hpccg_hip_group_generate, hpccg_hip_group_create_csr): member r is rank r of
 * a z-slab job on its own device. Implemented in
 * lib/libhpccg_hip_poly_group.so (linked against libhpccg_hip.so), a library of
 * its own beside the six others.
 *
 * Per column the recurrence, the host scalars and the device expressions are
 * exactly those written in hpccg_hip_poly.h, with M^-1 = diag(m) and by default
 * Jacobi, m_i = 1.0 / a_ii, on the global matrix. Every member runs them on its
 * rows of every column. Per iteration of a solve of degree d:
 *   update (+ step 0: dd = c0*m*r, z = dd)      -> halo of z, if d >= 1
 *   step j = 1 .. d: w = A z on the member's rows (the neighbours' boundary
 *            rows of z read from the member's ghost planes);
 *            dd = a_j*dd + b_j*m*(r - w);  z' = z + dd
 *                                               -> halo of z' unless j == d
 *   r.r and r.z: the members' local totals added in rank order from 0.0
 *   p = z_d + beta*p  -> halo of p;  Ap = A p;  p.Ap summed likewise
 * that is d halos of z and one of p, each one kernel launch per member for all
 * columns, and two group sums. A step needs no dot. z lives in two buffers per
 * member that the steps alternate between (step j reads buffer (j - 1) & 1 and
 * stores buffer j & 1). All members see the same per-column alpha, beta and
 * stop, so a column whose loop has ended is frozen on every member while the
 * others go on. The tolerance, niters, normr and the residual trace stay on the
 * 2-norm of r.
 *
 * Bitwise statements, for finite B and X0:
 *   - degree 0 is hpccg_hip_group_pcg_solve_device with the same m on the same
 *     members: every member's x, niters, normr and every trace;
 *   - a group of one (or a plain one-rank matrix, nranks == 1) is
 *     hpccg_hip_poly_solve_device of the same arguments, and its bound and
 *     spectrum are that library's;
 *   - column c of a call is its single-column call on every member;
 *   - exact scaling: on S A S with S b, S a diagonal of powers of two, s_i x'_i
 *     is bitwise the x on A on every member, with explicit bounds and with the
 *     default bound (the bound is the same number on both).
 * Against the one-rank solve of the global matrix the group differs in the
 * summation order of the dots only (the members' totals in rank order).
 *
 * The spectrum. lmax == 0.0 means the symmetric Gershgorin bound of the global
 * matrix, lmax = max_i q_i * sum_j |a_ij|*q_j with q = sqrt(m): every member
 * takes q of its rows, the ghost planes of q move once, every member runs the
 * bound pass over its own image, and the group's bound is the maximum over the
 * members -- order-free and exact; a NaN stays a NaN and is refused. For
 * Jacobi each member's part is computed once and cached in that member's
 * workspace of this library beside its 1 / a_ii (it goes with the workspace);
 * for a caller's m it is computed in every call that passes lmax == 0.0.
 * lmin == 0.0 means lmax / 30. A caller's bounds are NOT verified. Negative or
 * non-finite bounds and lmin >= lmax (as given, or against the computed lmax)
 * are refused. With degree 0 the bounds are checked but not used, and none is
 * computed.
 *
 * A row whose diagonal is missing, not finite or <= 0 on any member makes a
 * Jacobi call fail with HPCCG_HIP_EINVAL (the message names the member and its
 * first such row, counted from the member's first row); a caller's m is checked
 * on every member in every call in the same way. Every refusal happens before
 * any column is staged: every X is left untouched.
 *
 * A degenerate or non-finite column has the outcome written in hpccg_hip_pcg.h
 * on every member, also where the bad entry lies on a plane a neighbour reads;
 * the other columns are bitwise unaffected, and nothing of it stays in the
 * members' workspaces.
 *
 * Scope: the whole group in rank order (Ms[r] is member r, nranks the group's
 * size), members of the z-slab halo plan with a SELL-512-A or SELL-512 image.
 * Refused before any device work, the caller's X untouched and its current
 * device kept: members of the gather plan (HPCCG_HIP_EPLAN); a wrong nranks,
 * members of different groups, a member not at its own rank, a member without
 * rows, nrhs <= 0, max_iter < 0, a degree outside 0 .. 16, bad bounds, a
 * leading dimension below a member's nrow, NULL arguments (HPCCG_HIP_EINVAL).
 * nranks == 1 runs the same code on a halo-free matrix: nothing is forwarded to
 * another library. The functions of hpccg_hip_poly.h keep refusing the members
 * of a group.
 *
 * The workspace is one per member, owned by the member matrix: the columns (p
 * and the two z buffers with the member's ghost planes), the member's cached
 * 1 / a_ii with its verdict and its part of Jacobi's bound, room for a caller's
 * m and the bound's vectors. It grows on demand and is freed by
 * hpccg_hip_group_poly_release() or, at the latest, with the matrix. The
 * members' own solve vectors and their workspaces of the other libraries are
 * never touched: those solves give their usual bits before and after.
 *
 * Members on different devices: the halo kernel and the column-state stores go
 * through peer pointers, and a caller's m is copied on the member's stream.
 * That path is untested: it has never been run (it needs more than one GPU).
 * All members on one device is what has been tested.
 *
 * The environment variable HPCCG_GROUP_POLY_HALO_COPIES (any value) moves every
 * ghost plane by one copy per column and side instead of the halo kernel: a
 * fallback and a baseline with the same bits.
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one group must not overlap in time. */
#ifndef HPCCG_HIP_POLY_GROUP_H
#define HPCCG_HIP_POLY_GROUP_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_group_poly_abi_version(void);

/* B_dev, ldb, X_dev, ldx, minv_dev, max_iter, tolerance, niters, normr, times:
 * as hpccg_hip_group_pcg_solve_device (hpccg_hip_pcg_group.h). degree: 0 to 16.
 * lmin, lmax: the interval (0.0: the defaults above). */
int hpccg_hip_group_poly_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs,
                                      const double* const* B_dev, const long long* ldb,
                                      double* const* X_dev, const long long* ldx,
                                      const double* const* minv_dev, int degree, double lmin,
                                      double lmax, int max_iter, double tolerance, int* niters,
                                      double* normr, double* times);

/* *lmax = the group's symmetric Gershgorin bound above: minv_dev NULL for
 * Jacobi, else minv_dev[r] is member r's nrow device doubles (checked). */
int hpccg_hip_group_poly_bound(hpccg_hip_matrix* const* Ms, int nranks,
                               const double* const* minv_dev, double* lmax);

/* The interval the last solve of this library on the group used (degree 0: the
 * arguments as resolved without the device, 0.0 where none was given). */
int hpccg_hip_group_poly_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin,
                                       double* lmax);

/* Residual trace (2-norm of r) of column col of the last group solve of this
 * library (one set of all-reduced scalars: the same for every member). Returns
 * the number of entries written, or a negative error code. */
int hpccg_hip_group_poly_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out,
                                    int cap);

/* Free member M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_group_poly_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_group_poly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_group_poly_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_POLY_GROUP_H */
