/* hpccg_hip_poly32_group.h -- the Chebyshev polynomial preconditioned CG of
 * hpccg_hip_poly_group.h over an in-process rank group, with the polynomial
 * steps of every member streamed from an fp32 image of that member's rows, as
 * hpccg_hip_poly32.h does on one rank. Implemented in
 * lib/libhpccg_hip_poly32_group.so (linked against libhpccg_hip.so), a library
 * of its own beside the eight others.
 *
 * This is the recurrence of hpccg_hip_poly_group.h, statement for statement --
 * per member the update with step 0, the steps with the halos of z between
 * them, the group sums of r.r, r.z and p.Ap in rank order, the p update with
 * its halo, the outer SpMM -- with the two differences of hpccg_hip_poly32.h,
 * taken per member.
 *
 * 1. The steps read the member's fp32 image. Let A~ be the matrix with every
 *    stored value rounded to float. In step j member r forms w_i = (A~ z)_i on
 *    its rows, summed in slot order, each value widened to double in the
 *    register; every vector, product and sum is fp64 with no contraction. The
 *    z buffers and the ghost planes that move between the members carry fp64
 *    vectors exactly as in hpccg_hip_poly_group.h. m (Jacobi's 1.0 / a_ii or
 *    the caller's), the Chebyshev scalars and the Gershgorin bound (the
 *    maximum over the members) are fp64 and come from the fp64 image. Why an
 *    inexact image is safe is written in hpccg_hip_poly32.h: A~ is symmetric
 *    (an entry and its transpose round alike, also across two members), so the
 *    preconditioner stays one fixed symmetric positive definite operator.
 *
 * 2. The outer SpMM (Ap = A p) of member r streams its fp32 image only where
 *    that image is exact, i.e. every stored value of the member's rows survives
 *    double -> float -> double; otherwise it streams the member's fp64 image
 *    with the loops and plan choices of hpccg_hip_poly_group.h's library. The
 *    members of one group may differ in this: the bits are the same either way
 *    where the image is exact. The system solved is always the fp64 one.
 *
 * The image. Each member holds one fp32 image in its workspace of this
 * library: exactly 4 bytes per stored slot of the image the member holds. It is
 * built on the member's device on first use (a solve, the bound or the info
 * call), before the member's preconditioner and at every degree, and freed by
 * hpccg_hip_group_poly32_release() or, at the latest, with the matrix. A member
 * with a stored value whose fp32 image is not finite, or that is nonzero and
 * below FLT_MIN in magnitude, refuses the whole call with HPCCG_HIP_EINVAL
 * ("group poly32: member r: the matrix is outside fp32 range ..."), before any
 * column is staged: every X is left untouched.
 *
 * Bitwise statements, for finite B and X0:
 *   1. where every member's image is exact, every column is
 *      hpccg_hip_group_poly_solve_device bit for bit at every degree: each
 *      member's x, niters, normr and every trace;
 *   2. degree 0 is hpccg_hip_group_pcg_solve_device with the same m, bit for
 *      bit, on any matrix;
 *   3. a group of one (or a plain one-rank matrix, nranks == 1) is
 *      hpccg_hip_poly32_solve_device bit for bit, on exact and inexact images at
 *      every degree, and its bound and spectrum are that library's;
 *   4. column c of a call is its single-column call on every member;
 *   5. the halo kernel and the halo by copies give the same bits;
 *   6. the non-temporal and the plain forms of the value loads (the matrix
 *      option "nt" forced to 1 and to 0) give the same bits.
 * On inexact images at degree >= 1 the iterates are not those of
 * hpccg_hip_group_poly_solve_device: the same recurrence with A~ inside the
 * polynomial, converging to the fp64 tolerance on the fp64 residual. Against
 * hpccg_hip_poly32_solve_device of the global matrix the group differs in the
 * summation order of the dots only.
 *
 * Spectrum, diagonal and m checks, degenerate and non-finite columns: as
 * written in hpccg_hip_poly_group.h, with this library's name in the messages.
 *
 * Scope: that of hpccg_hip_poly_group.h. The whole group in rank order (Ms[r]
 * is member r, nranks the group's size), members of the z-slab halo plan with a
 * SELL-512-A or SELL-512 image. Refused before any device work, the caller's X
 * untouched and its current device kept: members of the gather plan
 * (HPCCG_HIP_EPLAN); a wrong nranks, members of different groups, a member not
 * at its own rank, a member without rows, nrhs <= 0, max_iter < 0, a degree
 * outside 0 .. 16, bad bounds, a leading dimension below a member's nrow, NULL
 * arguments (HPCCG_HIP_EINVAL). nranks == 1 runs the same code on a halo-free
 * matrix: nothing is forwarded to another library. The functions of
 * hpccg_hip_poly32.h keep refusing the members of a group, and those of
 * hpccg_hip_poly_group.h keep streaming fp64 values.
 *
 * The workspace is one per member, owned by the member matrix: what
 * hpccg_hip_poly_group.h's holds, and the member's fp32 image. The members' own
 * solve vectors and their workspaces of the other libraries are never touched:
 * those solves give their usual bits before and after.
 *
 * Members on different devices: the halo kernel and the column-state stores go
 * through peer pointers, and a caller's m is copied on the member's stream.
 * That path is untested: it has never been run (it needs more than one GPU).
 * All members on one device is what has been tested.
 *
 * The environment variable HPCCG_GROUP_POLY32_HALO_COPIES (any value) moves
 * every ghost plane by one copy per column and side instead of the halo
 * kernel: a fallback and a baseline with the same bits.
 *
 * Error codes are those of hpccg_hip.h; every function returns 0 on success
 * unless stated otherwise. Calls on one group must not overlap in time. */
#ifndef HPCCG_HIP_POLY32_GROUP_H
#define HPCCG_HIP_POLY32_GROUP_H

#include "hpccg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 */
int hpccg_hip_group_poly32_abi_version(void);

/* The arguments of hpccg_hip_group_poly_solve_device (hpccg_hip_poly_group.h). */
int hpccg_hip_group_poly32_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs,
                                        const double* const* B_dev, const long long* ldb,
                                        double* const* X_dev, const long long* ldx,
                                        const double* const* minv_dev, int degree, double lmin,
                                        double lmax, int max_iter, double tolerance, int* niters,
                                        double* normr, double* times);

/* *lmax = the group's symmetric Gershgorin bound of the fp64 image: minv_dev
 * NULL for Jacobi, else minv_dev[r] is member r's nrow device doubles
 * (checked). The value hpccg_hip_group_poly_bound computes. */
int hpccg_hip_group_poly32_bound(hpccg_hip_matrix* const* Ms, int nranks,
                                 const double* const* minv_dev, double* lmax);

/* The interval the last solve of this library on the group used (degree 0: the
 * arguments as resolved without the device, 0.0 where none was given). */
int hpccg_hip_group_poly32_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin,
                                         double* lmax);

/* Residual trace (2-norm of r) of column col of the last group solve of this
 * library (one set of all-reduced scalars: the same for every member). Returns
 * the number of entries written, or a negative error code. */
int hpccg_hip_group_poly32_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col,
                                      double* out, int cap);

/* The members' fp32 images (built on first use). out holds 4 * nranks entries;
 * for member r, out[4r]: 1 where its image is exact (it is the member's rows of
 * the matrix), else 0; out[4r + 1]: device bytes of its image; out[4r + 2]: its
 * stored values that did not survive the round trip through float;
 * out[4r + 3]: 0. */
int hpccg_hip_group_poly32_info(hpccg_hip_matrix* const* Ms, int nranks, long long* out);

/* Free member M's workspace of this library now, its fp32 image included (both
 * are rebuilt on the next call). */
int hpccg_hip_group_poly32_release(hpccg_hip_matrix* M);

/* Device bytes M's workspace of this library holds, the image included (0: none). */
int hpccg_hip_group_poly32_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes);

/* Matrices that hold a workspace of this library at the moment. */
int hpccg_hip_group_poly32_live_workspaces(int* count);

#ifdef __cplusplus
}
#endif

#endif /* HPCCG_HIP_POLY32_GROUP_H */
