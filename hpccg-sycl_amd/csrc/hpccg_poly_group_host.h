// hpccg_poly_group_host.h -- the host code of the Chebyshev polynomial
// preconditioned CG over an in-process rank group, shared by the polynomial
// group units (hpccg_poly_group.hip, hpccg_poly32_group.hip and, with its own
// recurrence in solve_device's slots, hpccg_srpoly_group.hip): what is
// polynomial in them -- the members' bound, the group's update phase with the
// halos of z (group_poly_update: the ordering argument is written there), the
// interval of a solve and the bodies of solve_device, bound and last_spectrum.
// It stands on hpccg_group_host.h (the members' preconditioner, the argument
// checks and the staging of a group solve, last_trace; through it
// hpccg_group.h, the group engine, and hpccg_onerank_host.h, the launch
// dispatch and the bookkeeping bodies) and hpccg_poly_host.h (the polynomial's
// workspace, arguments, launchers and interval).
// A unit hands over one traits struct U: what those headers ask for (Args,
// Workspace, who, halo_env, sum, halo, diag, check; row0, init, p, update,
// finalize, spmm_a, spmm_sell, and step, step_sell where it runs the fp64
// steps) and further
//   q, bound, bound_top   the bound's kernels
//   launch_spmm(w, a, prologue), launch_step(w, a)   a member's SpMM and one
//                         step over the chunks of columns
//   image(w, r)           what the unit builds per member before the
//                         preconditioner (the fp32 unit: the member's image,
//                         whose verdict comes first; else nothing)
// Its Workspace is a PolyWorkspace and a GroupMember with total_bytes().
// The __global__ entry points and the extern "C" definitions stay in the units.
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include "hpccg_group_host.h"
#include "hpccg_poly_host.h"

namespace hpccg {

namespace {

// hpccg_group_host.h's preparation of the members with what a polynomial unit
// adds: its image before the preconditioner, and beside the member's cache
// the bound's vectors.
template <class U>
int group_preconditioner(hpccg_hip_matrix* const* Ms, GroupOf<U>* G, const double* const* minv,
                         std::vector<const double*>* m)
{
    return group_members<U>(Ms, G, minv, m, U::image, [](typename U::Workspace* w) {
        w->p0 = guarded_p_column(w->v).p0;
        return ensure_bound_vectors(w, guarded_p_column(w->v).pcs);
    });
}

// The symmetric Gershgorin bound of the global matrix with the members' m:
// every member takes q = sqrt(m) of its rows into its guarded q column, the
// ghost planes of q move once, every member runs the bound pass over its own
// image (its rows' sums reach the neighbours' q through the ghost planes), and
// the group's bound is the maximum of the members': order-free and exact. A NaN
// stays one and is refused here. part[r] (may be null): member r's maximum.
template <class U>
int compute_group_bound(const GroupOf<U>& G, const std::vector<const double*>& m, HaloLaunch halo, double* part,
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
    TRY(group_halo_of(G, 1, halo, [&](int r) {
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
int jacobi_group_bound(const GroupOf<U>& G, const std::vector<const double*>& m, HaloLaunch halo, double* lmax)
{
    bool built = true;
    for (int r = 0; r < G.P; r++) built = built && G.w[r]->jac_lmax_built;
    if (!built) {
        std::vector<double> part(G.P, 0.0);
        double top = 0.0;
        TRY(compute_group_bound<U>(G, m, halo, part.data(), &top));
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
int group_poly_update(const GroupOf<U>& G, int nrhs, bool prologue, HaloLaunch halo)
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

// ---------------------------------------------------------------------------
// The bodies of a unit's extern "C" functions
// ---------------------------------------------------------------------------
// The polynomial CG's launch loop: hpccg_group.h's, with the update phase above.
template <class U>
int group_poly_run(const GroupOf<U>& G, int nrhs, int max_iter, double tol, HaloLaunch halo, int* niters,
                   double* normr, double* wall)
{
    const GroupLaunch<typename U::Workspace, typename U::Args> launch = {
        launch_init<U>,     launch_p<U>,         U::launch_spmm, launch_update0<U>,
        launch_finalize<U>, launch_group_sum<U>, halo,           group_poly_update<U>};
    return group_run_cg(G, nrhs, max_iter, tol, launch, niters, normr, wall);
}

// hpccg_group_host.h's solve_device with the degree and the bounds checked
// after the arrays, and the interval resolved once every member's m is in hand.
// Where a unit differs (the single-reduction unit, hpccg_srcg_group_host.h):
// more(w, cap) (may be null) allocates what its workspace adds to the
// polynomial's vectors, member_args are a member's kernel arguments, run is its
// launch loop.
template <class U>
int group_poly_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                            const long long* ldb, double* const* X_dev, const long long* ldx,
                            const double* const* minv_dev, int degree, double lmin, double lmax, int max_iter,
                            double tolerance, int* niters, double* normr, double* times,
                            int (*more)(typename U::Workspace*, int cap) = nullptr,
                            typename U::Args (*member_args)(const typename U::Workspace*, int, const double*) =
                                make_args<U>,
                            int (*run)(const GroupOf<U>&, int nrhs, int max_iter, double tol, HaloLaunch halo,
                                       int* niters, double* normr, double* wall) = group_poly_run<U>)
{
    using W = typename U::Workspace;
    const char* who = U::who;
    return group_solve_device<U>(
        Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, niters, normr, times, true,
        [&] { return check_polynomial(who, degree, lmin, lmax); },
        [&](GroupOf<U>& G, int kmax) -> int {
            const HaloLaunch halo = halo_launcher<U>();
            // the preconditioner and the interval first, on every member: a
            // refused call leaves every X as it is
            std::vector<const double*> m;
            TRY(group_preconditioner<U>(Ms, &G, minv_dev, &m));
            double cheb0 = 0.0, aj[kPolyMaxDegree + 1] = {}, bj[kPolyMaxDegree + 1] = {};
            TRY(resolve_interval(who, degree, &lmin, &lmax, &cheb0, aj, bj, [&](double* top) {
                return minv_dev ? compute_group_bound<U>(G, m, halo, nullptr, top)
                                : jacobi_group_bound<U>(G, m, halo, top);
            }));
            for (int r = 0; r < G.P; r++) {
                W* w = G.w[r];
                TRY(ensure_vectors(w, nrhs, kmax, guarded_p_column(w->v).pcs, 3,
                                   [&](int cap) { return more ? more(w, cap) : 0; }));
                w->degree = degree;
                w->cheb0 = cheb0;
                std::copy(aj, aj + kPolyMaxDegree + 1, w->aj);
                std::copy(bj, bj + kPolyMaxDegree + 1, w->bj);
                G.a[r] = member_args(w, nrhs, m[r]);
            }
            G.w[0]->last_lmin = lmin;
            G.w[0]->last_lmax = lmax;
            G.w[0]->solved = true;
            return group_run_staged(G, nrhs, B_dev, ldb, X_dev, ldx, times, [&](double* wall) {
                return run(G, nrhs, kmax, tolerance, halo, niters, normr, wall);
            });
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
    GroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    const HaloLaunch halo = halo_launcher<U>();
    return keep_device([&]() -> int {
        std::vector<const double*> m;
        TRY(group_preconditioner<U>(Ms, &G, minv_dev, &m));
        return minv_dev ? compute_group_bound<U>(G, m, halo, nullptr, lmax) : jacobi_group_bound<U>(G, m, halo, lmax);
    });
}

template <class U>
int group_poly_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin, double* lmax)
{
    const char* who = U::who;
    TRY(check_group_args(who, Ms, nranks));
    if (!lmin || !lmax) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument (lmin or lmax)", who);
    GroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    // one interval for the group: kept with member 0's record
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(Ms[0]);
    if (!w || !w->solved)
        return fail(HPCCG_HIP_EINVAL, "%s: no spectrum (no polynomial group solve ran on the members)", who);
    *lmin = w->last_lmin;
    *lmax = w->last_lmax;
    return 0;
}

}  // namespace

}  // namespace hpccg
