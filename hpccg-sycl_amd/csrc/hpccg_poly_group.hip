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
// hpccg_poly32.hip; the dispatch of a launch on a chunk's columns and SpMM form
// and the bookkeeping exports are hpccg_onerank_host.h, shared with
// hpccg_pcg.hip and the rest; the members' preconditioner, the argument checks
// and the staging of a group solve are hpccg_group_host.h, shared with
// hpccg_pcg_group.hip and hpccg_srcg_group.hip; the members' bound, the update
// phase with the halos of z (group_poly_update: the ordering argument is
// written there) and the solve are hpccg_poly_group_host.h, shared with
// hpccg_poly32_group.hip. This unit keeps its kernels and its traits. Ordering
// between the members is by stream events only. No kernel here waits on another
// block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_poly_group.h"
#include "hpccg_poly_group_host.h"

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
// host: hpccg_poly_group_host.h over this unit's kernels
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

// What the shared host code runs: this unit's kernels, on a member's rows.
struct GroupPoly {
    using Args = PolyArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "group poly";
    // diagnostics: the halos by copies, the A/B of k_poly_group_halo (tools/group_poly_bench.py)
    static constexpr const char* halo_env = "HPCCG_GROUP_POLY_HALO_COPIES";
    static long long row0(const Workspace* w) { return w->p0; }
    static int image(Workspace*, int) { return 0; }  // (the fp64 image the matrix holds)

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
    static constexpr auto sum = k_poly_group_sum;
    static constexpr auto halo = k_poly_group_halo;
    static constexpr auto diag = k_poly_group_diag;
    static constexpr auto check = k_poly_group_check;
    static constexpr auto q = k_poly_group_q;
    static constexpr auto bound = k_poly_group_bound;
    static constexpr auto bound_top = k_poly_group_bound_top;

    // the SpMM and every step from the fp64 image
    static void launch_spmm(const Workspace* w, Args a, bool prologue) { launch_spmm64<GroupPoly>(w, a, prologue); }
    static void launch_step(const Workspace* w, Args a) { launch_step64<GroupPoly>(w, a); }
};

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
    return group_poly_solve_device<GroupPoly>(Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax,
                                              max_iter, tolerance, niters, normr, times);
}

int hpccg_hip_group_poly_bound(hpccg_hip_matrix* const* Ms, int nranks, const double* const* minv_dev, double* lmax)
{
    return group_poly_bound<GroupPoly>(Ms, nranks, minv_dev, lmax);
}

int hpccg_hip_group_poly_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin, double* lmax)
{
    return group_poly_last_spectrum<GroupPoly>(Ms, nranks, lmin, lmax);
}

int hpccg_hip_group_poly_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    return group_last_trace<GroupPoly>(Ms, nranks, col, out, cap);
}

int hpccg_hip_group_poly_release(hpccg_hip_matrix* M) { return unit_release<GroupPoly>(M); }

int hpccg_hip_group_poly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<GroupPoly>(M, bytes);
}

int hpccg_hip_group_poly_live_workspaces(int* count) { return unit_live_workspaces<GroupPoly>(count); }

}  // extern "C"
