// hpccg_srcg_group.hip -- single-reduction preconditioned CG over an in-process
// rank group (include/hpccg_hip_srcg_group.h, lib/libhpccg_hip_srcg_group.so):
// kernels and host code of the eleventh library.
//
// Member r is rank r of a z-slab job. Every member runs the Chronopoulos-Gear
// recurrence of hpccg_srcg.hip (the step and the finalize of
// hpccg_srcg_bodies.h, the SpMM bodies of hpccg_spmm.h, that library's launch
// bounds and plan choices) on its own rows, on its own stream, in a workspace
// of its own. An iteration carries one sum over the members where the group
// pcg's carries two:
//   step      k_srcg_group_step<kR>: p, s, x, r, u = m r and the r.u and r.r
//             slice partials (prologue: r = b - A t, u = m r), then the halo of
//             every column's u
//   SpMM      k_srcg_group_spmm_a<kW, kR, kWaves> | k_srcg_group_spmm_sell<kR>:
//             w = A u and the u.w slice partial
//   finalize  k_srcg_group_finalize with store_total: the member's local totals
//             of r.r, r.u and u.w
//   sum       k_srcg_group_sum on member 0's stream: each of the three totals
//             added in rank order from 0.0, one srcg_advance, the state stored
//             to every member
//   halo      k_srcg_group_halo: one launch per member moves the ghost planes
//             of all columns; the copy form is kept as the fallback and the
//             baseline
//   prologue  k_srcg_group_t<kR>: t = x + 0 x into u's buffer, then the halo of t
//   diagonal  k_srcg_group_diag | k_srcg_group_check: hpccg_jacobi.h's bodies,
//             per member, with no communication
// The group and its checks, the guarded u column, the bodies of the halo
// kernel, the halo, the ordering of the sum and the staging of B and X are
// hpccg_group.h; the dispatch of a launch on a chunk's columns and SpMM form
// and the bookkeeping exports are hpccg_onerank_host.h; the member's workspace
// and preconditioner, the argument checks and the solve are hpccg_group_host.h,
// shared with hpccg_pcg_group.hip; p and s, the launchers, the sum kernel's
// body, the fence between neighbours and the launch loop are
// hpccg_srcg_group_host.h (over hpccg_srcg_host.h), shared with
// hpccg_srpoly_group.hip. Ordering between the members is by stream events. No
// kernel here waits on another block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_srcg_group.h"
#include "hpccg_srcg_group_host.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// (SrcgArgs' p: u, a guard zone around each column, ghost_lo rows below row 0,
// ghost_hi rows from row n; xsell: -ghost_lo; minv: the member's m; tot: the
// member's local dot totals, [3][cap])

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_srcg_group_init(SrcgArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// The prologue's t = x + 0.0*x, into u's buffer (col_p's prologue form; launched with no other).
template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_group_t(SrcgArgs a, bool prologue)
{
    col_p<kR, true>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_group_step(SrcgArgs a, bool prologue)
{
    srcg_step<kR>(a, prologue);
}

// The pcg library's plan choices (hpccg_pcg.hip): kWaves 5 for the 27-wide
// four-column form over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_srcg_group_spmm_a(
    SrcgArgs a, bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_group_spmm_sell(SrcgArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

// store_total: the three totals are this member's parts of the dots and the
// state is left to k_srcg_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_srcg_group_finalize(SrcgArgs a, int store_total)
{
    srcg_finalize(a, store_total);
}

// The group's three dots and the column's state on every member (hpccg_srcg_group_host.h).
__global__ void k_srcg_group_sum(SrcgArgs a, GroupTotals g)
{
    srcg_group_sum(a, g);
}

// The halo of every column's u (in the prologue: t) in one launch per member (hpccg_group.h).
__global__ __launch_bounds__(kHaloThreads) void k_srcg_group_halo(HaloArgs h)
{
    halo_body(h);
}

// The diagonal of a member's rows and the check of a caller's m: hpccg_jacobi.h's
// bodies (the view of a member with ghost rows is read like any other).
__global__ __launch_bounds__(kBlock) void k_srcg_group_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_srcg_group_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// One member's workspace: the columns (u's guarded, with the member's ghost
// planes), p and s, the cached 1 / a_ii with its verdict and a slot for a
// caller's m. The member's other workspaces are other records.
struct Workspace : GroupWorkspace, SrcgColumns {
    void free_own_vectors()
    {
        GroupWorkspace::free_own_vectors();
        free_ps();
    }
};

// hpccg_srcg_group_host.h's, hpccg_group_host.h's and hpccg_onerank_host.h's host code over this unit's kernels
struct SrcgGroupUnit {
    using Args = SrcgArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "group srcg";
    // diagnostics: the halo by copies, the A/B of k_srcg_group_halo (tools/group_srcg_bench.py)
    static constexpr const char* halo_env = "HPCCG_GROUP_SRCG_HALO_COPIES";
    static int own_vectors(Workspace* w, size_t count) { return alloc_ps(w, count); }
    static SrcgArgs make_args(const Workspace* w, int nrhs, const double* m)
    {
        SrcgArgs a{};
        fill_member_args(&a, w, nrhs, m);
        a.pd = w->pd;
        a.sd = w->sd;
        return a;
    }

    static constexpr auto init = k_srcg_group_init;
    template <int kR>
    static constexpr auto t = k_srcg_group_t<kR>;
    template <int kR>
    static auto fused_step(const Workspace*)
    {
        return k_srcg_group_step<kR>;
    }
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_srcg_group_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_srcg_group_spmm_sell<kR>;
    static constexpr auto finalize = k_srcg_group_finalize;
    static constexpr auto sum = k_srcg_group_sum;
    static constexpr auto halo = k_srcg_group_halo;
    static constexpr auto diag = k_srcg_group_diag;
    static constexpr auto check = k_srcg_group_check;
};
using SrcgGroup = GroupOf<SrcgGroupUnit>;

// The launch loop with u in p's buffer: the prologue fences, and nothing runs between the step and the halo of u.
int group_run(const SrcgGroup& G, int nrhs, int max_iter, double tol, HaloLaunch halo, int* niters, double* normr,
              double* wall)
{
    const SrcgGroupLaunch<Workspace, SrcgArgs> S{launch_spmm64<SrcgGroupUnit>, p_buf, true};
    return group_run_srcg<SrcgGroupUnit>(G, nrhs, max_iter, tol, halo, S, niters, normr, wall);
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_group_srcg_abi_version(void) { return 1; }

int hpccg_hip_group_srcg_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                      const long long* ldb, double* const* X_dev, const long long* ldx,
                                      const double* const* minv_dev, int max_iter, double tolerance, int* niters,
                                      double* normr, double* times)
{
    return group_diag_solve_device<SrcgGroupUnit>(Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter,
                                                  tolerance, niters, normr, times, group_run);
}

int hpccg_hip_group_srcg_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    return group_last_trace<SrcgGroupUnit>(Ms, nranks, col, out, cap);
}

int hpccg_hip_group_srcg_release(hpccg_hip_matrix* M) { return unit_release<SrcgGroupUnit>(M); }

int hpccg_hip_group_srcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<SrcgGroupUnit>(M, bytes);
}

int hpccg_hip_group_srcg_live_workspaces(int* count) { return unit_live_workspaces<SrcgGroupUnit>(count); }

}  // extern "C"
