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
// hpccg_poly_group_host.h and hpccg_poly_host.h, whose solve_device this unit
// runs with p and s and its own recurrence; p and s, the launchers, the sum
// kernel's body, the fence between neighbours and the launch loop
// (group_iteration: the ordering argument is written there) are
// hpccg_srcg_group_host.h (over hpccg_srcg_host.h), shared with
// hpccg_srcg_group.hip. This unit keeps its kernel arguments, the steps
// 1 .. d with their halos and the SpMM of u. Ordering between the members is by
// stream events only. No kernel here waits on another block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_srpoly_group.h"
#include "hpccg_poly_group_host.h"
#include "hpccg_srcg_group_host.h"
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

// The group's three dots and the column's state on every member (hpccg_srcg_group_host.h).
__global__ void k_srpoly_group_sum(SrpolyArgs a, GroupTotals g)
{
    srcg_group_sum(a, g);
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
struct Workspace : PolyWorkspace, GroupMember, SrcgColumns {
    void free_own_vectors()
    {
        PolyWorkspace::free_own_vectors();
        free_ps();
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
    template <int kR>
    static constexpr auto t = k_srpoly_group_t<kR>;
    // (degree 0: hpccg_srcg_bodies.h's step)
    template <int kR>
    static auto fused_step(const Workspace* w)
    {
        return w->degree > 0 ? k_srpoly_group_step<kR, true> : k_srpoly_group_step<kR, false>;
    }
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_srpoly_group_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_srpoly_group_spmm_sell<kR>;
    template <int kW, int kR, int kWaves>
    static constexpr auto step = k_srpoly_group_cheb<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto step_sell = k_srpoly_group_cheb_sell<kR>;
    static constexpr auto finalize = k_srpoly_group_finalize;
    static constexpr auto sum = k_srpoly_group_sum;
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

// w = A u and the u.w slice partial: the SpMM with u in p's place.
void launch_spmm_u(const Workspace* w, SrpolyArgs a, bool prologue)
{
    if (w->degree > 0) a.p = const_cast<double*>(a.u);
    launch_spmm64<GroupSrpoly>(w, a, prologue);
}

// Steps 1 .. d over the group, each after the halo of the buffer it reads (halos 0 .. d - 1 of group_iteration).
int group_steps(const Grp& G, int nrhs, HaloLaunch halo)
{
    const int d = G.w[0]->degree;
    for (int j = 1; j <= d; j++) {
        const int in = (j - 1) & 1;
        TRY(group_halo_of(G, nrhs, halo, [&](int r) { return HaloBuf{z_of<GroupSrpoly>(G.w[r], in), G.a[r].pcs}; }));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_step64<GroupSrpoly>(G.w[r], step_args<GroupSrpoly>(G.w[r], G.a[r], j));
        }
    }
    return 0;
}

// The launch loop with u = z_d: the prologue fences at degree 0 only, where u shares p's buffer with t.
int group_run(const Grp& G, int nrhs, int max_iter, double tol, HaloLaunch halo, int* niters, double* normr,
              double* wall)
{
    const SrcgGroupLaunch<Workspace, SrpolyArgs> S{launch_spmm_u, u_buf, G.w[0]->degree == 0, group_steps};
    return group_run_srcg<GroupSrpoly>(G, nrhs, max_iter, tol, halo, S, niters, normr, wall);
}

int more_vectors(Workspace* w, int cap) { return alloc_ps(w, (size_t)w->v.npad * cap); }

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
    return group_poly_solve_device<GroupSrpoly>(Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax,
                                                max_iter, tolerance, niters, normr, times, more_vectors,
                                                make_member_args, group_run);
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
