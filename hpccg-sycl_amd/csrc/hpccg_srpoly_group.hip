// hpccg_srpoly_group.hip -- single-reduction CG with the Chebyshev polynomial
// preconditioner over an in-process rank group
// (include/hpccg_hip_srpoly_group.h, lib/libhpccg_hip_srpoly_group.so): kernels
// and host code of the thirteenth library.
//
// Member r is rank r of a z-slab job. Every member runs the recurrence of
// hpccg_srpoly.hip (the fused step of hpccg_srpoly_bodies.h, the steps' ends of
// hpccg_poly_bodies.h, the finalize of hpccg_srcg_bodies.h, the SpMM loops of
// hpccg_spmm.h, that library's launch bounds and plan choices) on its own rows,
// on its own stream, in a workspace of its own. Per iteration:
//   step     k_srpoly_group_step<kR, true>: p, s, x, r, then step 0 (dd = c0 m r,
//            z = dd) into z buffer 0 and the r.r slice partial | <kR, false>,
//            degree 0: hpccg_srcg_bodies.h's step, u = m r
//   step j   k_srpoly_group_cheb<kW, kR, kWaves> | k_srpoly_group_cheb_sell<kR>,
//            j = 1 .. d, each after the halo of buffer (j - 1) & 1; the last
//            forms the r.u slice partial
//   SpMM     k_srpoly_group_spmm_a<kW, kR, kWaves> | k_srpoly_group_spmm_sell<kR>
//            after the halo of u = z_d (buffer d & 1): w = A u, the u.w partial
//   finalize k_srpoly_group_finalize with store_total: the member's local totals
//            of r.r, r.u and u.w
//   sum      k_srpoly_group_sum on member 0's stream: each of the three totals
//            added in rank order from 0.0, one srcg_advance, the state stored to
//            every member
//   halo     k_srpoly_group_halo: one launch per member moves the ghost planes
//            of all columns of one buffer (d + 1 per iteration, as the group
//            poly has); the copy form is kept as the fallback and the baseline
//   prologue k_srpoly_group_t<kR>: t = x + 0 x into p's buffer, then its halo
//   bound    k_srpoly_group_q, k_srpoly_group_bound, k_srpoly_group_bound_top
//   diagonal k_srpoly_group_diag | k_srpoly_group_check
// That is one sum over the members per iteration where the group poly has two.
// The group engine is hpccg_group.h; the members' preconditioner, the argument
// checks and the staging are hpccg_group_host.h; the members' bound and the
// polynomial's workspace, arguments, step launchers and interval are
// hpccg_poly_group_host.h and hpccg_poly_host.h; this unit adds p and s, the
// sum kernel, the launch loop (group_iteration: the ordering argument is written
// there) and the body of solve_device. Ordering between the members is by
// stream events only. No kernel here waits on another block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_srpoly_group.h"
#include "hpccg_poly_group_host.h"
#include "hpccg_srpoly_bodies.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// (SrpolyArgs' p and z buffers: a guard zone around each column, ghost_lo rows
// below row 0, ghost_hi rows from row n; xsell: -ghost_lo; tot: the member's
// local dot totals, [3][cap])

__global__ void k_srpoly_group_init(SrpolyArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// The prologue's t = x + 0.0*x, into p's buffer (col_p's prologue form; launched with no other).
template <int kR>
__global__ __launch_bounds__(kBlock) void k_srpoly_group_t(SrpolyArgs a, bool prologue)
{
    col_p<kR, true>(a, prologue);
}

// kCheb: hpccg_srpoly_bodies.h's step with step 0 in r's pass; else (degree 0) hpccg_srcg_bodies.h's.
template <int kR, bool kCheb>
__global__ __launch_bounds__(kBlock) void k_srpoly_group_step(SrpolyArgs a, bool prologue)
{
    if constexpr (kCheb)
        srpoly_step<kR>(a, prologue);
    else
        srcg_step<kR>(srcg_view(a), prologue);
}

// The poly library's plan choices (hpccg_poly.hip).
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_srpoly_group_spmm_a(
    SrpolyArgs a, bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srpoly_group_spmm_sell(SrpolyArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_srpoly_group_cheb(SrpolyArgs a)
{
    spmm_a_body<kW, kR, PolyArgs, PolyStep>(a, false);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srpoly_group_cheb_sell(SrpolyArgs a)
{
    spmm_sell_body<kR, PolyArgs, PolyStep>(a, false);
}

// store_total: the three totals are this member's parts of the dots and the
// state is left to k_srpoly_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_srpoly_group_finalize(SrpolyArgs a, int store_total)
{
    srcg_finalize(a, store_total);
}

// The group's three dots and the column's state on every member: one thread
// per column on member 0's stream, after every member's local finalize. Each
// dot is the members' local totals added in rank order from 0.0; the column
// advances once, as in the one-rank finalize, and its state is stored into
// every member's state array, so all members freeze a column together. hist
// and the "columns ended" word are member 0's (a: its args).
__global__ void k_srpoly_group_sum(SrpolyArgs a, GroupTotals g)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nrhs) return;
    ColState s = a.st[c];
    if (!s.run) return;  // frozen on every member
    double rr = 0.0, gamma = 0.0, delta = 0.0;
    for (int r = 0; r < g.nranks; r++) rr += g.tot[r][(size_t)kDotRR * g.cap[r] + c];
    for (int r = 0; r < g.nranks; r++) gamma += g.tot[r][(size_t)kDotRZ * g.cap[r] + c];
    for (int r = 0; r < g.nranks; r++) delta += g.tot[r][(size_t)kDotPAP * g.cap[r] + c];
    srcg_advance(a, &s, c, rr, gamma, delta);
    for (int r = 0; r < g.nranks; r++) g.st[r][c] = s;
}

// The halo of every column of one guarded buffer in one launch per member (hpccg_group.h).
__global__ __launch_bounds__(kHaloThreads) void k_srpoly_group_halo(HaloArgs h)
{
    halo_body(h);
}

__global__ __launch_bounds__(kBlock) void k_srpoly_group_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_srpoly_group_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// The bound's kernels (hpccg_poly_bodies.h), on a member's rows: q's ghost
// planes hold the neighbours' q.
__global__ void k_srpoly_group_q(const double* __restrict__ m, int n, double* __restrict__ q)
{
    poly_q_body(m, n, q);
}

__global__ __launch_bounds__(kBlock) void k_srpoly_group_bound(DiagArgs a, const double* __restrict__ q,
                                                               double* __restrict__ smax)
{
    poly_bound_body(a, q, smax);
}

__global__ __launch_bounds__(kBlock) void k_srpoly_group_bound_top(const double* __restrict__ smax, int nslices,
                                                                   double* __restrict__ out)
{
    poly_bound_top_body(smax, nslices, out);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// One member's workspace: hpccg_poly_host.h's (the columns with dd and the two
// z buffers, the cached 1 / a_ii with its verdict and the member's part of
// Jacobi's bound, a slot for a caller's m, the bound's vectors) with the
// member's events and p0, and the recurrence's plain columns p and s.
struct Workspace : PolyWorkspace, GroupMember {
    double *pd = nullptr, *sd = nullptr;  // p and s = A p (never zeroed again: k == 1 reads u and w)

    void free_own_vectors()
    {
        PolyWorkspace::free_own_vectors();
        for (double* q : {pd, sd})
            if (q) (void)hipFree(q);
        pd = sd = nullptr;
    }
    void free_own_rest()
    {
        PolyWorkspace::free_own_rest();
        destroy_events();
    }
};

// What the shared host code runs: this unit's kernels, on a member's rows.
struct GroupSrpoly {
    using Args = SrpolyArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "group srpoly";
    // diagnostics: the halos by copies, the A/B of k_srpoly_group_halo (tools/group_srpoly_bench.py)
    static constexpr const char* halo_env = "HPCCG_GROUP_SRPOLY_HALO_COPIES";
    static long long row0(const Workspace* w) { return w->p0; }
    static int image(Workspace*, int) { return 0; }  // (the fp64 image the matrix holds)

    static constexpr auto init = k_srpoly_group_init;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_srpoly_group_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_srpoly_group_spmm_sell<kR>;
    template <int kW, int kR, int kWaves>
    static constexpr auto step = k_srpoly_group_cheb<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto step_sell = k_srpoly_group_cheb_sell<kR>;
    static constexpr auto halo = k_srpoly_group_halo;
    static constexpr auto diag = k_srpoly_group_diag;
    static constexpr auto check = k_srpoly_group_check;
    static constexpr auto q = k_srpoly_group_q;
    static constexpr auto bound = k_srpoly_group_bound;
    static constexpr auto bound_top = k_srpoly_group_bound_top;
};
using Grp = GroupOf<GroupSrpoly>;

// u: z buffer d & 1 (degree 0: u = m r lives in p's buffer, which also holds the prologue's t)
HaloBuf u_buf(const Grp& G, int r)
{
    const int d = G.w[r]->degree;
    return d > 0 ? HaloBuf{z_of<GroupSrpoly>(G.w[r], d & 1), G.a[r].pcs} : HaloBuf{G.a[r].p, G.a[r].pcs};
}

SrpolyArgs make_member_args(const Workspace* w, int nrhs, const double* m)
{
    SrpolyArgs a = make_args<GroupSrpoly>(w, nrhs, m);
    a.u = z_of<GroupSrpoly>(w, w->degree & 1);
    a.zout = z_of<GroupSrpoly>(w, 0);  // the step's: step 0's z
    a.pd = w->pd;
    a.sd = w->sd;
    return a;
}

void launch_t(const Workspace* w, const SrpolyArgs& a)
{
    // (prologue: col_p's form)
    launch_chunks(w, a, true, [](auto r) { return k_srpoly_group_t<decltype(r)::value>; });
}

void launch_step(const Workspace* w, const SrpolyArgs& a, bool prologue)
{
    const int d = w->degree;
    launch_chunks(w, a, prologue, [d](auto r) {
        return d > 0 ? k_srpoly_group_step<decltype(r)::value, true> : k_srpoly_group_step<decltype(r)::value, false>;
    });
}

// w = A u and the u.w slice partial: the SpMM with u in p's place.
void launch_spmm_u(const Workspace* w, SrpolyArgs a)
{
    if (w->degree > 0) a.p = const_cast<double*>(a.u);
    launch_spmm64<GroupSrpoly>(w, a, false);
}

// (store_total: always 1 here, a member's part; the state is the group sum's)
void launch_finalize(const Workspace* w, const SrpolyArgs& a)
{
    hipLaunchKernelGGL(k_srpoly_group_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, 1);
}

// (which: group_sum's; the one launch sums all three dots)
void launch_sum(const Workspace* w, const SrpolyArgs& a, const GroupTotals& gt, int)
{
    hipLaunchKernelGGL(k_srpoly_group_sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt);
}

// Every member's stream waits for what its neighbours' streams hold so far.
// Degree 0's prologue needs it once: a member's step overwrites the t rows (u
// shares p's buffer there) its neighbours' halos read, with no group sum
// between the two. With d >= 1 nothing stores p's buffer after t.
int neighbour_fence(const Grp& G)
{
    if (G.P == 1) return 0;
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        if (r > 0) HIP_TRY(hipStreamWaitEvent(G.v[r].stream, G.w[r - 1]->evr, 0));
        if (r < G.P - 1) HIP_TRY(hipStreamWaitEvent(G.v[r].stream, G.w[r + 1]->evr, 0));
    }
    return 0;
}

// ---------------------------------------------------------------------------
// One iteration: every member's fused step (step 0 into buffer 0), then for
// j = 1 .. d the halo of z buffer (j - 1) & 1 and every member's step j, which
// stores the member's own rows of buffer j & 1; then the halo of u = z_d
// (buffer d & 1; degree 0: of p's buffer), every member's SpMM and finalize,
// and the group's one sum. Call the halo that follows step j halo j
// (j = 0 .. d; it moves buffer j & 1): d + 1 halos per iteration.
//
// Two buffers suffice, and no member's rows of a buffer are overwritten before
// every neighbour has pulled them:
//   - Halos 0 .. d - 1 and steps 1 .. d are hpccg_poly_group_host.h's
//     (group_poly_update): member r's halo j waits on the events its neighbours
//     record after their step j; the next store into those rows within the
//     iteration is the neighbour's step j + 2, which follows its halo j + 1,
//     which waits on r's event recorded after r's step j + 1, which follows r's
//     halo j on r's stream.
//   - Halo d moves u after step d. Nothing of this iteration stores buffer
//     d & 1 after step d: the SpMM and the finalize read only.
//   - The next iteration's fused step stores buffer 0 on every member, and its
//     step 1 buffer 1. Both follow the group's sum on every stream; the sum
//     waits for every member's finalize; every member's finalize follows all
//     its halos, halo d included, on its own stream. So every pull of either
//     buffer is over before the next iteration stores into it.
//   - The fused step reads the member's own rows of u = z_d before it stores
//     buffer 0 (for an even d the same rows, by the same thread); it follows
//     the member's SpMM, the last reader of u's ghost planes, on its stream.
//   - A member's ghost planes are stored by its halos and read by its steps and
//     its SpMM only, all on its stream.
// Frozen columns' planes move too; a frozen column's z is no longer stored.
// ---------------------------------------------------------------------------
int group_iteration(const Grp& G, int nrhs, bool prologue, HaloLaunch halo, const GroupTotals& gt,
                    const GroupLaunch<Workspace, SrpolyArgs>& L)
{
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_step(G.w[r], G.a[r], prologue);
    }
    const int d = G.w[0]->degree;
    for (int j = 1; j <= d; j++) {
        const int in = (j - 1) & 1;
        TRY(group_halo_of(G, nrhs, halo, [&](int r) { return HaloBuf{z_of<GroupSrpoly>(G.w[r], in), G.a[r].pcs}; }));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_step64<GroupSrpoly>(G.w[r], step_args<GroupSrpoly>(G.w[r], G.a[r], j));
        }
    }
    TRY(group_halo_of(G, nrhs, halo, [&](int r) { return u_buf(G, r); }));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm_u(G.w[r], G.a[r]);
        launch_finalize(G.w[r], G.a[r]);
    }
    return group_sum(G, gt, kDotRR, L);
}

// The recurrence over the group on the columns staged in the members' b and x:
// hpccg_srpoly.hip's launch sequence on every member's stream. Every
// kCheckEvery iterations the host reads member 0's "columns ended" word, as
// group_run_cg does.
int group_run_srpoly(const Grp& G, int nrhs, int max_iter, double tol, HaloLaunch halo, int* niters, double* normr,
                     double* wall)
{
    const GroupTotals gt = group_totals(G);
    GroupLaunch<Workspace, SrpolyArgs> L{};  // (group_sum takes the sum's launcher from it)
    L.sum = launch_sum;
    TRY(use(G, 0));
    HIP_TRY(hipEventRecord(G.w[0]->ev0, G.v[0].stream));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_init<GroupSrpoly>(G.w[r], G.a[r], max_iter, tol);
        launch_t(G.w[r], G.a[r]);
    }
    TRY(group_halo(G, nrhs, halo));
    if (G.w[0]->degree == 0) TRY(neighbour_fence(G));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm64<GroupSrpoly>(G.w[r], G.a[r], true);
    }
    TRY(group_iteration(G, nrhs, true, halo, gt, L));
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < max_iter; k++) {
        TRY(group_iteration(G, nrhs, false, halo, gt, L));
        if (k % kCheckEvery == 0 && k + 1 < max_iter) {
            bool ended = false;
            TRY(group_ended(G, nrhs, &ended));
            if (ended) break;
        }
    }
    return group_finish(G, nrhs, niters, normr, wall);
}

// hpccg_poly_group_host.h's solve_device (the degree and the bounds checked
// after the arrays, the interval resolved once every member's m is in hand)
// with this unit's vectors and launch loop.
int solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev, const long long* ldb,
                 double* const* X_dev, const long long* ldx, const double* const* minv_dev, int degree, double lmin,
                 double lmax, int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    using U = GroupSrpoly;
    const char* who = U::who;
    return group_solve_device<U>(
        Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, niters, normr, times, true,
        [&]() -> int {
            if (degree < 0 || degree > kPolyMaxDegree)
                return fail(HPCCG_HIP_EINVAL, "%s: degree %d (0 to %d)", who, degree, kPolyMaxDegree);
            return check_bounds(who, lmin, lmax);
        },
        [&](Grp& G, int kmax) -> int {
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
                Workspace* w = G.w[r];
                const size_t npad = (size_t)w->v.npad;
                TRY(ensure_vectors(w, nrhs, kmax, guarded_p_column(w->v).pcs, 3, [&](int cap) {
                    TRY(alloc_zero(w, &w->pd, npad * cap));
                    return alloc_zero(w, &w->sd, npad * cap);
                }));
                w->degree = degree;
                w->cheb0 = cheb0;
                std::copy(aj, aj + kPolyMaxDegree + 1, w->aj);
                std::copy(bj, bj + kPolyMaxDegree + 1, w->bj);
                G.a[r] = make_member_args(w, nrhs, m[r]);
            }
            G.w[0]->last_lmin = lmin;
            G.w[0]->last_lmax = lmax;
            G.w[0]->solved = true;
            return group_run_staged(G, nrhs, B_dev, ldb, X_dev, ldx, times, [&](double* wall) {
                return group_run_srpoly(G, nrhs, kmax, tolerance, halo, niters, normr, wall);
            });
        });
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_group_srpoly_abi_version(void) { return 1; }

int hpccg_hip_group_srpoly_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                        const long long* ldb, double* const* X_dev, const long long* ldx,
                                        const double* const* minv_dev, int degree, double lmin, double lmax,
                                        int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_device(Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance,
                        niters, normr, times);
}

int hpccg_hip_group_srpoly_bound(hpccg_hip_matrix* const* Ms, int nranks, const double* const* minv_dev, double* lmax)
{
    return group_poly_bound<GroupSrpoly>(Ms, nranks, minv_dev, lmax);
}

int hpccg_hip_group_srpoly_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin, double* lmax)
{
    return group_poly_last_spectrum<GroupSrpoly>(Ms, nranks, lmin, lmax);
}

int hpccg_hip_group_srpoly_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    return group_last_trace<GroupSrpoly>(Ms, nranks, col, out, cap);
}

int hpccg_hip_group_srpoly_release(hpccg_hip_matrix* M) { return unit_release<GroupSrpoly>(M); }

int hpccg_hip_group_srpoly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<GroupSrpoly>(M, bytes);
}

int hpccg_hip_group_srpoly_live_workspaces(int* count) { return unit_live_workspaces<GroupSrpoly>(count); }

}  // extern "C"
