// hpccg_poly_group_host.h -- the host code of the Chebyshev polynomial
// preconditioned CG over an in-process rank group, shared by the polynomial
// group units (hpccg_poly_group.hip, hpccg_poly32_group.hip): the members'
// preconditioner and bound, the group's update phase with the halos of z
// (group_poly_update: the ordering argument is written there), the solve and
// the bodies of the units' extern "C" functions that take the group (release,
// workspace_bytes and live_workspaces are hpccg_onerank_host.h's). It stands on
// hpccg_group.h (the group engine), hpccg_poly_host.h (the polynomial's
// workspace, arguments, launchers and interval) and, through it,
// hpccg_onerank_host.h (the launch dispatch, the init, SpMM and finalize
// launchers).
// A unit hands over one traits struct U: what those two headers' launchers
// need (Args, Workspace, row0, init, p, update, finalize, spmm_a, spmm_sell,
// and step, step_sell where it runs the fp64 steps) and further
//   who                   the name in front of its messages ("group poly")
//   halo_env              the environment variable of the halo by copies
//   sum, halo             its group sum and halo kernels
//   diag, check, q, bound, bound_top   the preconditioner's and the bound's kernels
//   launch_spmm(w, a, prologue), launch_step(w, a)   a member's SpMM and one
//                         step over the chunks of columns
//   image(w, r)           what the unit builds per member before the
//                         preconditioner (the fp32 unit: the member's image,
//                         whose verdict comes first; else nothing)
// Its Workspace is a PolyWorkspace and a GroupMember with total_bytes().
// The __global__ entry points and the extern "C" definitions stay in the units.
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include <cstdlib>
#include <vector>

#include "hpccg_group.h"
#include "hpccg_poly_host.h"

namespace hpccg {

namespace {

template <class U>
using PolyGroupOf = Group<typename U::Workspace, typename U::Args>;

// a group of one is checked and run like any other: nothing forwards it
constexpr bool kOneForwarded = false;

// The member's cache (hpccg_jacobi.h), its two events and the bound's vectors.
template <class U>
int ensure_rest(typename U::Workspace* w)
{
    HIP_TRY(hipSetDevice(w->v.device));
    TRY(w->create_events());
    TRY(ensure_cache(w));
    w->p0 = guarded_p_column(w->v).p0;
    return ensure_bound_vectors(w, guarded_p_column(w->v).pcs);
}

template <class U>
int ensure_member_jacobi(typename U::Workspace* w, int r)
{
    int row = -1;
    TRY(build_jacobi(w, U::diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "%s: Jacobi needs a finite diagonal > 0 in every row; on member %d row %d (local) is the "
                    "first whose diagonal is missing, not finite or <= 0",
                    U::who, r, row);
    return 0;
}

template <class U>
int stage_member_minv(typename U::Workspace* w, int r, const double* minv)
{
    int row = -1;
    TRY(load_minv(w, minv, hipMemcpyDeviceToDevice, U::check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "%s: member %d's minv[%d] is not finite and > 0 (the first such entry)", U::who, r,
                    row);
    return 0;
}

template <class U>
void launch_halo(hipStream_t s, dim3 grid, const HaloArgs& h)
{
    hipLaunchKernelGGL(U::halo, grid, dim3(kHaloThreads), 0, s, h);
}

// The members' records, what the unit builds per member, events, caches and
// preconditioner vectors: m[r] is member r's padded device m (its muser, or its
// cached 1 / a_ii).
template <class U>
int group_preconditioner(hpccg_hip_matrix* const* Ms, PolyGroupOf<U>* G, const double* const* minv,
                         std::vector<const double*>* m)
{
    G->w.assign(G->P, nullptr);
    m->assign(G->P, nullptr);
    for (int r = 0; r < G->P; r++) {
        TRY(g_ws<typename U::Workspace>.record(Ms[r], G->v[r], &G->w[r]));
        TRY(U::image(G->w[r], r));
        TRY(ensure_rest<U>(G->w[r]));
        if (minv)
            TRY(stage_member_minv<U>(G->w[r], r, minv[r]));
        else
            TRY(ensure_member_jacobi<U>(G->w[r], r));
        (*m)[r] = minv ? G->w[r]->muser : G->w[r]->jac;
    }
    return 0;
}

// The symmetric Gershgorin bound of the global matrix with the members' m:
// every member takes q = sqrt(m) of its rows into its guarded q column, the
// ghost planes of q move once, every member runs the bound pass over its own
// image (its rows' sums reach the neighbours' q through the ghost planes), and
// the group's bound is the maximum of the members': order-free and exact. A NaN
// stays one and is refused here. part[r] (may be null): member r's maximum.
template <class U>
int compute_group_bound(const PolyGroupOf<U>& G, const std::vector<const double*>& m, bool copies, double* part,
                        double* lmax)
{
    using W = typename U::Workspace;
    for (int r = 0; r < G.P; r++) {
        const MatrixView& v = G.v[r];
        const W* w = G.w[r];
        TRY(use(G, r));
        hipLaunchKernelGGL(U::q, dim3((v.n + 255) / 256), dim3(256), 0, v.stream, m[r], v.n, w->qbuf + w->p0);
    }
    HIP_TRY(hipGetLastError());
    // (q is written once per call and read by the bound pass only, which every
    // member's stream has finished before this function returns)
    TRY(group_halo_of(G, 1, copies ? nullptr : launch_halo<U>, [&](int r) {
        return HaloBuf{G.w[r]->qbuf + G.w[r]->p0, guarded_p_column(G.v[r]).pcs};
    }));
    for (int r = 0; r < G.P; r++) {
        const MatrixView& v = G.v[r];
        const W* w = G.w[r];
        TRY(use(G, r));
        hipLaunchKernelGGL(U::bound, dim3(v.nslices), dim3(kBlock), 0, v.stream, diag_args(v),
                           (const double*)(w->qbuf + w->p0), w->smax);
        hipLaunchKernelGGL(U::bound_top, dim3(1), dim3(kBlock), 0, v.stream, (const double*)w->smax, v.nslices,
                           w->lmax_dev);
    }
    HIP_TRY(hipGetLastError());
    double top = 0.0;
    std::vector<double> h(G.P, 0.0);
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipMemcpyAsync(&h[r], G.w[r]->lmax_dev, sizeof(double), hipMemcpyDeviceToHost, G.v[r].stream));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    for (int r = 0; r < G.P; r++) {
        if (part) part[r] = h[r];
        if (h[r] > top || h[r] != h[r]) top = h[r];  // (max_nan)
        if (top != top) break;
    }
    if (!(top > 0.0 && std::isfinite(top)))
        return fail(HPCCG_HIP_EINVAL, "%s: the Gershgorin bound of the matrix is %g (finite and > 0 needed)", U::who,
                    top);
    *lmax = top;
    return 0;
}

// Jacobi's bound: every member's part is cached in its workspace beside its
// 1 / a_ii (matrices and groups are immutable); the maximum is retaken per call.
template <class U>
int jacobi_group_bound(const PolyGroupOf<U>& G, const std::vector<const double*>& m, bool copies, double* lmax)
{
    bool built = true;
    for (int r = 0; r < G.P; r++) built = built && G.w[r]->jac_lmax_built;
    if (!built) {
        std::vector<double> part(G.P, 0.0);
        double top = 0.0;
        TRY(compute_group_bound<U>(G, m, copies, part.data(), &top));
        for (int r = 0; r < G.P; r++) {
            G.w[r]->jac_lmax = part[r];
            G.w[r]->jac_lmax_built = true;
        }
    }
    double top = 0.0;
    for (int r = 0; r < G.P; r++) top = std::max(top, G.w[r]->jac_lmax);  // (finite: checked when built)
    *lmax = top;
    return 0;
}

// ---------------------------------------------------------------------------
// The group's update phase (hpccg_group.h's hook): every member's update with
// step 0, then for j = 1 .. d the halo of z buffer (j - 1) & 1 and every
// member's step j, which reads that buffer with its ghost planes and stores the
// member's own rows of buffer j & 1. Call the halo that follows step j halo j
// (j = 0 .. d - 1; it moves buffer j & 1): d halos of z per iteration.
//
// Two buffers suffice, and no member's rows of a buffer are overwritten before
// every neighbour has pulled them:
//   - Member r's halo j reads its neighbours' rows of buffer j & 1 once their
//     step j has stored them: it waits on the events the neighbours record
//     after their step j (group_halo_of records, then waits).
//   - The next store into those rows is the neighbour's step j + 2 (the same
//     parity). On the neighbour's stream step j + 2 follows its halo j + 1;
//     that halo waits on r's event recorded after r's step j + 1; and on r's
//     stream step j + 1 follows r's halo j. So r has pulled the rows of step j
//     before the neighbour's step j + 2 can start. The events a neighbour's
//     halo j waits on likewise follow that neighbour's halo j - 1.
//   - Member r's own ghost planes of a buffer are stored by r's halos and read
//     by r's steps only, all on r's stream.
//   - The next iteration's step 0 stores buffer 0 on every member. The last
//     pull of buffer 0 is the halo with the largest even j <= d - 1 of this
//     iteration; every member's finalize of r.r follows its halos on its own
//     stream, the group sum of r.r waits for every member's finalize, and the
//     next update follows that sum (and the sum of p.Ap) on every stream. For
//     an even d, z_d lives in buffer 0 and the p update reads the member's own
//     rows of it: that kernel precedes the next update on the same stream.
// Frozen columns' planes move too; a frozen column's z is no longer stored.
// Which image a step streams its matrix values from (U::launch_step) does not
// enter the argument: z and its planes are fp64 vectors in either unit.
// ---------------------------------------------------------------------------
template <class U>
int group_poly_update(const PolyGroupOf<U>& G, int nrhs, bool prologue, HaloLaunch halo)
{
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_update0<U>(G.w[r], G.a[r], prologue);
    }
    const int d = G.w[0]->degree;
    for (int j = 1; j <= d; j++) {
        const int in = (j - 1) & 1;
        TRY(group_halo_of(G, nrhs, halo, [&](int r) { return HaloBuf{z_of<U>(G.w[r], in), G.a[r].pcs}; }));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            U::launch_step(G.w[r], step_args<U>(G.w[r], G.a[r], j));
        }
    }
    return 0;
}

template <class U>
void launch_group_sum(const typename U::Workspace* w, const typename U::Args& a, const GroupTotals& gt, int which)
{
    hipLaunchKernelGGL(U::sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt, which);
}

// copies: the halos by copies (the fallback and the baseline), else by the unit's halo kernel.
template <class U>
int group_solve(hpccg_hip_matrix* const* Ms, const PolyGroupOf<U>& G0, int nrhs, const double* const* B,
                const long long* ldb, double* const* X, const long long* ldx, const double* const* minv, int degree,
                double lmin, double lmax, int max_iter, double tol, bool copies, int* niters, double* normr,
                double* times)
{
    using W = typename U::Workspace;
    using A = typename U::Args;
    PolyGroupOf<U> G = G0;
    if (times) std::fill(times, times + 7, 0.0);
    if (max_iter < 1) max_iter = 1;
    G.a.resize(G.P);
    // the preconditioner and the interval first, on every member: a refused
    // call leaves every X as it is
    std::vector<const double*> m;
    TRY(group_preconditioner<U>(Ms, &G, minv, &m));
    double cheb0 = 0.0, aj[kPolyMaxDegree + 1] = {}, bj[kPolyMaxDegree + 1] = {};
    TRY(resolve_interval(U::who, degree, &lmin, &lmax, &cheb0, aj, bj, [&](double* top) {
        return minv ? compute_group_bound<U>(G, m, copies, nullptr, top) : jacobi_group_bound<U>(G, m, copies, top);
    }));
    for (int r = 0; r < G.P; r++) {
        W* w = G.w[r];
        TRY(ensure_vectors(w, nrhs, max_iter, guarded_p_column(w->v).pcs, 3));
        w->degree = degree;
        w->cheb0 = cheb0;
        std::copy(aj, aj + kPolyMaxDegree + 1, w->aj);
        std::copy(bj, bj + kPolyMaxDegree + 1, w->bj);
        G.a[r] = make_args<U>(w, nrhs, m[r]);
    }
    G.w[0]->last_lmin = lmin;
    G.w[0]->last_lmax = lmax;
    G.w[0]->solved = true;
    TRY(group_stage_in(G, nrhs, B, ldb, X, ldx));
    const GroupLaunch<W, A> launch = {launch_init<U>,
                                      launch_p<U>,
                                      U::launch_spmm,
                                      launch_update0<U>,
                                      launch_finalize<U>,
                                      launch_group_sum<U>,
                                      copies ? nullptr : launch_halo<U>,
                                      group_poly_update<U>};
    double wall = 0.0;
    TRY(group_run_cg(G, nrhs, max_iter, tol, launch, niters, normr, &wall));
    TRY(group_stage_out(G, nrhs, X, ldx));
    if (times) times[0] = wall;
    return 0;
}

template <class U>
bool halo_by_copies()
{
    // diagnostics: the halos by copies, the A/B of the unit's halo kernel (the group benchmark tools)
    return std::getenv(U::halo_env) != nullptr;
}

// ---------------------------------------------------------------------------
// The bodies of a unit's extern "C" functions
// ---------------------------------------------------------------------------
template <class U>
int group_poly_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                            const long long* ldb, double* const* X_dev, const long long* ldx,
                            const double* const* minv_dev, int degree, double lmin, double lmax, int max_iter,
                            double tolerance, int* niters, double* normr, double* times)
{
    const char* who = U::who;
    TRY(check_group_args(who, Ms, nranks));
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "%s: nrhs %d (at least 1)", who, nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "%s: max_iter %d is negative", who, max_iter);
    if (!B_dev || !ldb || !X_dev || !ldx || !niters || !normr)
        return fail(HPCCG_HIP_EINVAL, "%s: NULL argument (B_dev, ldb, X_dev, ldx, niters or normr)", who);
    for (int r = 0; r < nranks; r++) {
        if (!Ms[r]) return fail(HPCCG_HIP_EINVAL, "%s: Ms[%d] is NULL", who, r);  // (before any is looked at)
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "%s: B_dev[%d] or X_dev[%d] is NULL", who, r, r);
        if (minv_dev && !minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "%s: minv_dev[%d] is NULL", who, r);
    }
    if (degree < 0 || degree > kPolyMaxDegree)
        return fail(HPCCG_HIP_EINVAL, "%s: degree %d (0 to %d)", who, degree, kPolyMaxDegree);
    TRY(check_bounds(who, lmin, lmax));
    PolyGroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    TRY(check_group_lds(who, G, ldb, ldx, "ldb, ldx"));
    const bool copies = halo_by_copies<U>();
    return keep_device([&] {
        return group_solve<U>(Ms, G, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance,
                              copies, niters, normr, times);
    });
}

template <class U>
int group_poly_bound(hpccg_hip_matrix* const* Ms, int nranks, const double* const* minv_dev, double* lmax)
{
    const char* who = U::who;
    TRY(check_group_args(who, Ms, nranks));
    if (!lmax) return fail(HPCCG_HIP_EINVAL, "%s: lmax is NULL", who);
    for (int r = 0; minv_dev && r < nranks; r++)
        if (!minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "%s: minv_dev[%d] is NULL", who, r);
    PolyGroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    const bool copies = halo_by_copies<U>();
    return keep_device([&]() -> int {
        std::vector<const double*> m;
        TRY(group_preconditioner<U>(Ms, &G, minv_dev, &m));
        return minv_dev ? compute_group_bound<U>(G, m, copies, nullptr, lmax)
                        : jacobi_group_bound<U>(G, m, copies, lmax);
    });
}

template <class U>
int group_poly_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin, double* lmax)
{
    const char* who = U::who;
    TRY(check_group_args(who, Ms, nranks));
    if (!lmin || !lmax) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument (lmin or lmax)", who);
    PolyGroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    // one interval for the group: kept with member 0's record
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(Ms[0]);
    if (!w || !w->solved)
        return fail(HPCCG_HIP_EINVAL, "%s: no spectrum (no polynomial group solve ran on the members)", who);
    *lmin = w->last_lmin;
    *lmax = w->last_lmax;
    return 0;
}

template <class U>
int group_poly_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    const char* who = U::who;
    TRY(check_group_args(who, Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "%s: out is NULL", who);
    PolyGroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    // one set of all-reduced scalars: kept with member 0's record
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(Ms[0]);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "%s: no trace of column %d (the last group solve had %d)", who, col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

}  // namespace

}  // namespace hpccg
