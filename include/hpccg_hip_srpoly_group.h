/* hpccg_hip_srpoly_group.h -- the single-reduction CG with the Chebyshev
 * polynomial preconditioner of hpccg_hip_srpoly.h over an in-process rank group
 * of hpccg_hip.h (hpccg_hip_group_generate, hpccg_hip_group_create_csr): member
 * r is rank r of a z-slab job on its own device. Implemented in
 * lib/libhpccg_hip_srpoly_group.so (linked against libhpccg_hip.so), a library
 * of its own beside the others.
 *
 * Per column the recurrence, the host scalars and the device expressions are
 * exactly those written in hpccg_hip_srpoly.h, with M^-1 = diag(m) and by
 * default Jacobi on the global matrix. Every member runs them on its rows of
 * every column. Per iteration of a solve of degree d:
 *   step: p, s, x, r (+ step 0: dd = c0*m*r, z = dd)   -> halo of z, if d >= 1
 *   step j = 1 .. d: w = A z on the member's rows;
 *            dd = a_j*dd + b_j*m*(r - w);  z' = z + dd   -> halo of z'
 *   w = A u with u = z_d on the member's rows
 *   r.r, r.u and u.w: the members' local totals added in rank order from 0.0,
 *            at one point
 * that is d + 1 halos, as hpccg_hip_poly_group.h has (d of z and one of p), each
 * one kernel launch per member for all columns, and one group sum where that
 * library has two. All members see the same per-column alpha, beta and stop.
 *
 * Bitwise statements, for finite B and X0:
 *   - degree 0 is hpccg_hip_group_srcg_solve_device with the same m on the same
 *     members: every member's x, niters, normr and every trace;
 *   - up to max_iter = 2 a call is hpccg_hip_group_poly_solve_device of the same
 *     arguments, and the trace up to max_iter = 3;
 *   - a group of one (or a plain one-rank matrix, nranks == 1) is
 *     hpccg_hip_srpoly_solve_device of the same arguments, and its bound and
 *     spectrum are that library's;
 *   - column c of a call is its single-column call on every member.
 *
 * The spectrum, the refusals (a bad diagonal or m on any member, bad bounds, a
 * bad degree: HPCCG_HIP_EINVAL before any column is staged, every X left
 * untouched; members of the gather plan: HPCCG_HIP_EPLAN), degenerate columns,
 * the scope, the workspace (one per member: hpccg_hip_poly_group.h's and the
 * columns p and s; freed by hpccg_hip_group_srpoly_release() or with the
 * matrix) and members on different devices (untested): as written in
 * hpccg_hip_poly_group.h. The functions of hpccg_hip_srpoly.h keep refusing the
 * members of a group.
 *
 * The environment variable HPCCG_GROUP_SRPOLY_HALO_COPIES (any value) moves
 * every ghost plane by one copy per column and side instead of the halo kernel:
 * a fallback and a baseline with the same bits.
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one group must not overlap in time. */
#ifndef HPCCG_HIP_SRPOLY_GROUP_H
#define HPCCG_HIP_SRPOLY_GROUP_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_group_srpoly_abi_version(void);

/* The arguments of hpccg_hip_group_poly_solve_device (hpccg_hip_poly_group.h). */
int hpccg_hip_group_srpoly_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs,
                                        const double* const* B_dev, const long long* ldb,
                                        double* const* X_dev, const long long* ldx,
                                        const double* const* minv_dev, int degree, double lmin,
                                        double lmax, int max_iter, double tolerance, int* niters,
                                        double* normr, double* times);

/* *lmax = the group's symmetric Gershgorin bound (hpccg_hip_group_poly_bound's
 * value): minv_dev NULL for Jacobi, else minv_dev[r] is member r's nrow device
 * doubles (checked). */
int hpccg_hip_group_srpoly_bound(hpccg_hip_matrix* const* Ms, int nranks,
                                 const double* const* minv_dev, double* lmax);

/* The interval the last solve of this library on the group used (degree 0: the
 * arguments as resolved without the device, 0.0 where none was given). */
int hpccg_hip_group_srpoly_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin,
                                         double* lmax);

/* Residual trace (2-norm of r) of column col of the last group solve of this
 * library (one set of all-reduced scalars: the same for every member). Returns
 * the number of entries written, or a negative error code. */
int hpccg_hip_group_srpoly_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out,
                                      int cap);

/* Free member M's workspace of this library now (it is rebuilt on the next call). */
int hpccg_hip_group_srpoly_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds (0: none). */
int hpccg_hip_group_srpoly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_group_srpoly_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_SRPOLY_GROUP_H */
