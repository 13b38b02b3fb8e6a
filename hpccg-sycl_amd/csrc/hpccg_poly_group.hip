// hpccg_poly_group.hip -- Chebyshev polynomial preconditioned CG over an
// in-process rank group (include/hpccg_hip_poly_group.h,
// lib/libhpccg_hip_poly_group.so): kernels and host code of the seventh library.
//
// Member r is rank r of a z-slab job. Every member runs the recurrence of
// hpccg_poly.hip (hpccg_poly_bodies.h's device code, the kPre bodies of
// hpccg_columns.h, the SpMM loops of hpccg_spmm.h, that library's launch bounds
// and plan choices) on its own rows, on its own stream, in a workspace of its
// own. Per iteration:
//   update   k_poly_group_update<kR, kCheb>: with step 0 (dd = c0 m r, z = dd)
//            into z buffer 0                       -> halo of buffer 0 (d >= 1)
//   step j   k_poly_group_step<kW, kR, kWaves> | k_poly_group_step_sell<kR>,
//            j = 1 .. d: w = A z on the member's rows, the ghost planes of
//            buffer (j - 1) & 1 read; dd, z' = z + dd into buffer j & 1
//                                                  -> halo of z' unless j == d
//   finalize k_poly_group_finalize with store_total (r.r and r.z), then
//   sum      k_poly_group_sum on member 0's stream: the totals in rank order,
//            the state stored to every member
//   p update k_poly_group_p<kR, kPre>: p = z_d + beta p   -> halo of p
//   SpMM     k_poly_group_spmm_a<kW, kR, kWaves> | k_poly_group_spmm_sell<kR>,
//            finalize p.Ap, sum
//   halo     k_poly_group_halo: one launch per member moves the ghost planes of
//            all columns of one buffer (d z-halos and the p-halo per
//            iteration); the copy form is kept as the fallback and the baseline
//   bound    k_poly_group_q, k_poly_group_bound, k_poly_group_bound_top: per
//            member over its own image, after one halo of q; the group's lmax
//            is the maximum over the members, taken on the host
//   diagonal k_poly_group_diag | k_poly_group_check (hpccg_jacobi.h's bodies)
// Degree 0 applies no polynomial: the launches are the group pcg's.
//
// The group engine is hpccg_group.h, shared with hpccg_batch.hip and
// hpccg_pcg_group.hip; the polynomial's workspace, arguments, launchers and
// interval are hpccg_poly_host.h, shared with hpccg_poly.hip and
// hpccg_poly32.hip. This unit adds the members' preconditioner and bound and
// the update phase with the halos of z (group_poly_update: the ordering
// argument is written there). Ordering between
// the members is by stream events only. No kernel here waits on another block.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "../../include/hpccg_hip_poly_group.h"
#include "hpccg_group.h"
#include "hpccg_poly_host.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// (PolyArgs' p and z buffers: a guard zone around each column, ghost_lo rows
// below row 0, ghost_hi rows from row n; xsell: -ghost_lo; tot: the member's
// local dot totals, [3][cap])

__global__ void k_poly_group_init(PolyArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// kPre: p = m r + beta p (degree 0). Else a.r is the stored z_d: p = z + beta p.
template <int kR, bool kPre>
__global__ __launch_bounds__(kBlock) void k_poly_group_p(PolyArgs a, bool prologue)
{
    col_p<kR, kPre>(a, prologue);
}

// The poly library's plan choices (hpccg_poly.hip).
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_poly_group_spmm_a(
    PolyArgs a, bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_poly_group_spmm_sell(PolyArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

template <int kR, bool kCheb>
__global__ __launch_bounds__(kBlock) void k_poly_group_update(PolyArgs a, bool prologue)
{
    if constexpr (kCheb)
        poly_update0<kR>(a, prologue);
    else
        col_update<kR, true>(a, prologue);
}

template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_poly_group_step(PolyArgs a)
{
    spmm_a_body<kW, kR, PolyArgs, PolyStep>(a, false);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_poly_group_step_sell(PolyArgs a)
{
    spmm_sell_body<kR, PolyArgs, PolyStep>(a, false);
}

// store_total: the totals are this member's parts of the dots (the r.r launch:
// of r.r and of r.z) and the state is left to k_poly_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_poly_group_finalize(PolyArgs a, int which, int store_total)
{
    col_finalize<true>(a, which, store_total);
}

__global__ void k_poly_group_sum(PolyArgs a, GroupTotals g, int which)
{
    col_group_sum<true>(a, g, which);
}

// The halo of every column of one guarded buffer in one launch per member (hpccg_group.h).
__global__ __launch_bounds__(kHaloThreads) void k_poly_group_halo(HaloArgs h)
{
    halo_body(h);
}

__global__ __launch_bounds__(kBlock) void k_poly_group_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_poly_group_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// The bound's kernels (hpccg_poly_bodies.h), on a member's rows: q's ghost
// planes hold the neighbours' q.
__global__ void k_poly_group_q(const double* __restrict__ m, int n, double* __restrict__ q)
{
    poly_q_body(m, n, q);
}

__global__ __launch_bounds__(kBlock) void k_poly_group_bound(DiagArgs a, const double* __restrict__ q,
                                                             double* __restrict__ smax)
{
    poly_bound_body(a, q, smax);
}

__global__ __launch_bounds__(kBlock) void k_poly_group_bound_top(const double* __restrict__ smax, int nslices,
                                                                 double* __restrict__ out)
{
    poly_bound_top_body(smax, nslices, out);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// One member's workspace (hpccg_poly_host.h's, with the member's events and
// p0): the columns with dd and the two z buffers, the cached 1 / a_ii with its
// verdict and the member's part of Jacobi's bound, a slot for a caller's m, the
// bound's vectors. The call's degree and scalars are kept on every member; the
// spectrum and the traces of the last solve with member 0.
struct Workspace : PolyWorkspace, GroupMember {
    void free_own_rest()
    {
        PolyWorkspace::free_own_rest();
        destroy_events();
    }
};

using PolyGroup = Group<Workspace, PolyArgs>;
constexpr const char* kGroupWho = "group poly";
// a group of one is checked and run like any other: nothing forwards it
constexpr bool kOneForwarded = false;

// What hpccg_poly_host.h's launchers run: this unit's kernels, on a member's rows.
struct GroupPoly {
    using Args = PolyArgs;
    using Workspace = hpccg::Workspace;
    static long long row0(const Workspace* w) { return w->p0; }

    static constexpr auto init = k_poly_group_init;
    template <int kR, bool kPre>
    static constexpr auto p = k_poly_group_p<kR, kPre>;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_poly_group_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_poly_group_spmm_sell<kR>;
    template <int kR, bool kCheb>
    static constexpr auto update = k_poly_group_update<kR, kCheb>;
    template <int kW, int kR, int kWaves>
    static constexpr auto step = k_poly_group_step<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto step_sell = k_poly_group_step_sell<kR>;
    static constexpr auto finalize = k_poly_group_finalize;
};

// The member's cache (hpccg_jacobi.h), its two events and the bound's vectors.
int ensure_rest(Workspace* w)
{
    HIP_TRY(hipSetDevice(w->v.device));
    TRY(w->create_events());
    TRY(ensure_cache(w));
    w->p0 = guarded_p_column(w->v).p0;
    return ensure_bound_vectors(w, guarded_p_column(w->v).pcs);
}

int ensure_member_jacobi(Workspace* w, int r)
{
    int row = -1;
    TRY(build_jacobi(w, k_poly_group_diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "group poly: Jacobi needs a finite diagonal > 0 in every row; on member %d row %d (local) is the "
                    "first whose diagonal is missing, not finite or <= 0",
                    r, row);
    return 0;
}

int stage_member_minv(Workspace* w, int r, const double* minv)
{
    int row = -1;
    TRY(load_minv(w, minv, hipMemcpyDeviceToDevice, k_poly_group_check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "group poly: member %d's minv[%d] is not finite and > 0 (the first such entry)", r,
                    row);
    return 0;
}

void launch_halo(hipStream_t s, dim3 grid, const HaloArgs& h)
{
    hipLaunchKernelGGL(k_poly_group_halo, grid, dim3(kHaloThreads), 0, s, h);
}

// The members' records, events, caches and preconditioner vectors: m[r] is
// member r's padded device m (its muser, or its cached 1 / a_ii).
int group_preconditioner(hpccg_hip_matrix* const* Ms, PolyGroup* G, const double* const* minv,
                         std::vector<const double*>* m)
{
    G->w.assign(G->P, nullptr);
    m->assign(G->P, nullptr);
    for (int r = 0; r < G->P; r++) {
        TRY(g_ws<Workspace>.record(Ms[r], G->v[r], &G->w[r]));
        TRY(ensure_rest(G->w[r]));
        if (minv)
            TRY(stage_member_minv(G->w[r], r, minv[r]));
        else
            TRY(ensure_member_jacobi(G->w[r], r));
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
int compute_group_bound(const PolyGroup& G, const std::vector<const double*>& m, bool copies, double* part,
                        double* lmax)
{
    for (int r = 0; r < G.P; r++) {
        const MatrixView& v = G.v[r];
        const Workspace* w = G.w[r];
        TRY(use(G, r));
        hipLaunchKernelGGL(k_poly_group_q, dim3((v.n + 255) / 256), dim3(256), 0, v.stream, m[r], v.n,
                           w->qbuf + w->p0);
    }
    HIP_TRY(hipGetLastError());
    // (q is written once per call and read by the bound pass only, which every
    // member's stream has finished before this function returns)
    TRY(group_halo_of(G, 1, copies ? nullptr : launch_halo, [&](int r) {
        return HaloBuf{G.w[r]->qbuf + G.w[r]->p0, guarded_p_column(G.v[r]).pcs};
    }));
    for (int r = 0; r < G.P; r++) {
        const MatrixView& v = G.v[r];
        const Workspace* w = G.w[r];
        TRY(use(G, r));
        hipLaunchKernelGGL(k_poly_group_bound, dim3(v.nslices), dim3(kBlock), 0, v.stream, diag_args(v),
                           (const double*)(w->qbuf + w->p0), w->smax);
        hipLaunchKernelGGL(k_poly_group_bound_top, dim3(1), dim3(kBlock), 0, v.stream, (const double*)w->smax,
                           v.nslices, w->lmax_dev);
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
        return fail(HPCCG_HIP_EINVAL, "group poly: the Gershgorin bound of the matrix is %g (finite and > 0 needed)",
                    top);
    *lmax = top;
    return 0;
}

// Jacobi's bound: every member's part is cached in its workspace beside its
// 1 / a_ii (matrices and groups are immutable); the maximum is retaken per call.
int jacobi_group_bound(const PolyGroup& G, const std::vector<const double*>& m, bool copies, double* lmax)
{
    bool built = true;
    for (int r = 0; r < G.P; r++) built = built && G.w[r]->jac_lmax_built;
    if (!built) {
        std::vector<double> part(G.P, 0.0);
        double top = 0.0;
        TRY(compute_group_bound(G, m, copies, part.data(), &top));
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
// ---------------------------------------------------------------------------
int group_poly_update(const PolyGroup& G, int nrhs, bool prologue, HaloLaunch halo)
{
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_update0<GroupPoly>(G.w[r], G.a[r], prologue);
    }
    const int d = G.w[0]->degree;
    for (int j = 1; j <= d; j++) {
        const int in = (j - 1) & 1;
        TRY(group_halo_of(G, nrhs, halo, [&](int r) { return HaloBuf{z_of<GroupPoly>(G.w[r], in), G.a[r].pcs}; }));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_step64<GroupPoly>(G.w[r], step_args<GroupPoly>(G.w[r], G.a[r], j));
        }
    }
    return 0;
}

void launch_group_sum(const Workspace* w, const PolyArgs& a, const GroupTotals& gt, int which)
{
    hipLaunchKernelGGL(k_poly_group_sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt, which);
}

// copies: the halos by copies (the fallback and the baseline), else by k_poly_group_halo.
int group_solve(hpccg_hip_matrix* const* Ms, const PolyGroup& G0, int nrhs, const double* const* B, const long long* ldb,
                double* const* X, const long long* ldx, const double* const* minv, int degree, double lmin, double lmax,
                int max_iter, double tol, bool copies, int* niters, double* normr, double* times)
{
    PolyGroup G = G0;
    if (times) std::fill(times, times + 7, 0.0);
    if (max_iter < 1) max_iter = 1;
    G.a.resize(G.P);
    // the preconditioner and the interval first, on every member: a refused
    // call leaves every X as it is
    std::vector<const double*> m;
    TRY(group_preconditioner(Ms, &G, minv, &m));
    double cheb0 = 0.0, aj[kPolyMaxDegree + 1] = {}, bj[kPolyMaxDegree + 1] = {};
    TRY(resolve_interval(kGroupWho, degree, &lmin, &lmax, &cheb0, aj, bj, [&](double* top) {
        return minv ? compute_group_bound(G, m, copies, nullptr, top) : jacobi_group_bound(G, m, copies, top);
    }));
    for (int r = 0; r < G.P; r++) {
        Workspace* w = G.w[r];
        TRY(ensure_vectors(w, nrhs, max_iter, guarded_p_column(w->v).pcs, 3));
        w->degree = degree;
        w->cheb0 = cheb0;
        std::copy(aj, aj + kPolyMaxDegree + 1, w->aj);
        std::copy(bj, bj + kPolyMaxDegree + 1, w->bj);
        G.a[r] = make_args<GroupPoly>(w, nrhs, m[r]);
    }
    G.w[0]->last_lmin = lmin;
    G.w[0]->last_lmax = lmax;
    G.w[0]->solved = true;
    TRY(group_stage_in(G, nrhs, B, ldb, X, ldx));
    const GroupLaunch<Workspace, PolyArgs> launch = {launch_init<GroupPoly>,
                                                     launch_p<GroupPoly>,
                                                     launch_spmm64<GroupPoly>,
                                                     launch_update0<GroupPoly>,
                                                     launch_finalize<GroupPoly>,
                                                     launch_group_sum,
                                                     copies ? nullptr : launch_halo,
                                                     group_poly_update};
    double wall = 0.0;
    TRY(group_run_cg(G, nrhs, max_iter, tol, launch, niters, normr, &wall));
    TRY(group_stage_out(G, nrhs, X, ldx));
    if (times) times[0] = wall;
    return 0;
}

bool halo_by_copies()
{
    // diagnostics: the halos by copies, the A/B of k_poly_group_halo (tools/group_poly_bench.py)
    return std::getenv("HPCCG_GROUP_POLY_HALO_COPIES") != nullptr;
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_group_poly_abi_version(void) { return 1; }

int hpccg_hip_group_poly_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                      const long long* ldb, double* const* X_dev, const long long* ldx,
                                      const double* const* minv_dev, int degree, double lmin, double lmax, int max_iter,
                                      double tolerance, int* niters, double* normr, double* times)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "group poly: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "group poly: max_iter %d is negative", max_iter);
    if (!B_dev || !ldb || !X_dev || !ldx || !niters || !normr)
        return fail(HPCCG_HIP_EINVAL, "group poly: NULL argument (B_dev, ldb, X_dev, ldx, niters or normr)");
    for (int r = 0; r < nranks; r++) {
        if (!Ms[r]) return fail(HPCCG_HIP_EINVAL, "group poly: Ms[%d] is NULL", r);  // (before any is looked at)
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "group poly: B_dev[%d] or X_dev[%d] is NULL", r, r);
        if (minv_dev && !minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "group poly: minv_dev[%d] is NULL", r);
    }
    if (degree < 0 || degree > kPolyMaxDegree)
        return fail(HPCCG_HIP_EINVAL, "group poly: degree %d (0 to %d)", degree, kPolyMaxDegree);
    TRY(check_bounds(kGroupWho, lmin, lmax));
    PolyGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    TRY(check_group_lds(kGroupWho, G, ldb, ldx, "ldb, ldx"));
    const bool copies = halo_by_copies();
    return keep_device([&] {
        return group_solve(Ms, G, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance,
                           copies, niters, normr, times);
    });
}

int hpccg_hip_group_poly_bound(hpccg_hip_matrix* const* Ms, int nranks, const double* const* minv_dev, double* lmax)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (!lmax) return fail(HPCCG_HIP_EINVAL, "group poly: lmax is NULL");
    for (int r = 0; minv_dev && r < nranks; r++)
        if (!minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "group poly: minv_dev[%d] is NULL", r);
    PolyGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    const bool copies = halo_by_copies();
    return keep_device([&]() -> int {
        std::vector<const double*> m;
        TRY(group_preconditioner(Ms, &G, minv_dev, &m));
        return minv_dev ? compute_group_bound(G, m, copies, nullptr, lmax) : jacobi_group_bound(G, m, copies, lmax);
    });
}

int hpccg_hip_group_poly_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin, double* lmax)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (!lmin || !lmax) return fail(HPCCG_HIP_EINVAL, "group poly: NULL argument (lmin or lmax)");
    PolyGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    // one interval for the group: kept with member 0's record
    const Workspace* w = g_ws<Workspace>.find(Ms[0]);
    if (!w || !w->solved)
        return fail(HPCCG_HIP_EINVAL, "group poly: no spectrum (no polynomial group solve ran on the members)");
    *lmin = w->last_lmin;
    *lmax = w->last_lmax;
    return 0;
}

int hpccg_hip_group_poly_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "group poly: out is NULL");
    PolyGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    // one set of all-reduced scalars: kept with member 0's record
    const Workspace* w = g_ws<Workspace>.find(Ms[0]);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "group poly: no trace of column %d (the last group solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

int hpccg_hip_group_poly_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "group poly: NULL argument");
    g_ws<Workspace>.drop(M);
    return 0;
}

int hpccg_hip_group_poly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "group poly: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    *bytes = w ? w->bytes + w->rest_bytes : 0;
    return 0;
}

int hpccg_hip_group_poly_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "group poly: NULL argument");
    *count = g_ws<Workspace>.live();
    return 0;
}

}  // extern "C"
