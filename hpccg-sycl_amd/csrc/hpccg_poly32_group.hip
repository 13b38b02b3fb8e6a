// hpccg_poly32_group.hip -- Chebyshev polynomial preconditioned CG over an
// in-process rank group whose polynomial steps stream an fp32 image of every
// member's rows (include/hpccg_hip_poly32_group.h,
// lib/libhpccg_hip_poly32_group.so): kernels and host code of the ninth library.
//
// hpccg_poly_group.hip's recurrence, statement for statement, on every member;
// the polynomial steps alone differ: member r's row sums w = A~ z read its own
// fp32 image A~ = fl32(A) of its rows (hpccg_spmm32.h's Image32 and loops, as
// hpccg_poly32.hip on one rank), every value widened in the register. m, the
// Gershgorin bound, the coefficients, the z buffers with their ghost planes,
// the halos and the group sums are the fp64 group library's.
//   convert   k_poly32_group_convert: a member's fp64 image -> its fp32 image,
//             with the counts of the values that do not survive the round trip
//             and of those outside fp32 range
//   update    k_poly32_group_update<kR, kCheb>: with step 0 into z buffer 0
//                                                  -> halo of buffer 0 (d >= 1)
//   step j    k_poly32_group_step<kW, kR, kNT> | k_poly32_group_step_sell<kR, kNT>:
//             the fp32 loops over the member's image, the ghost planes of z
//             buffer (j - 1) & 1 read, hpccg_poly_bodies.h's PolyStep as the
//             end; dd, z' into buffer j & 1        -> halo of z' unless j == d
//             (this unit has no fp64 step kernel)
//   finalize  k_poly32_group_finalize with store_total, then
//   sum       k_poly32_group_sum on member 0's stream: the totals in rank order
//   p update  k_poly32_group_p<kR, kPre>             -> halo of p
//   SpMM      per member: where its image is exact (it is the member's rows)
//             k_poly32_group_spmm_a<kW, kR, kNT> | k_poly32_group_spmm_sell<kR, kNT>
//             over the fp32 image, the same bits as the fp64 loops; else
//             k_poly32_group_spmm64_a<kW, kR, kWaves> | k_poly32_group_spmm64_sell<kR>,
//             the fp64 loops with the poly library's plan choices
//   halo      k_poly32_group_halo: fp64 planes, as k_poly_group_halo
//   bound, diagonal: k_poly32_group_q, k_poly32_group_bound,
//             k_poly32_group_bound_top, k_poly32_group_diag, k_poly32_group_check
//             over the shared bodies and the fp64 image
// The 27-wide four-column fp32 forms take the x-triple plan on interior slices
// (hpccg_spmm32.h). Degree 0 applies no polynomial: the launches are the group
// pcg's on an inexact image.
//
// The host code is hpccg_poly_group_host.h (shared with hpccg_poly_group.hip)
// over hpccg_group.h, hpccg_poly_host.h and hpccg_onerank_host.h (the launch
// dispatch and the bookkeeping exports); what this unit adds is every
// member's image, built before its preconditioner, and the choice of the SpMM
// and step forms. Ordering between the members is by stream events only. No
// kernel here waits on another block.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/hpccg_hip_poly32_group.h"
#include "hpccg_poly_group_host.h"
#include "hpccg_spmm32.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// (PolyArgs' p and z buffers: a guard zone around each column, ghost_lo rows
// below row 0, ghost_hi rows from row n; xsell: -ghost_lo)
struct Poly32GroupArgs : PolyArgs {
    const float* img;  // the member's fp32 values (hpccg_spmm32.h's layout)
};

__global__ __launch_bounds__(kBlock) void k_poly32_group_convert(const double* __restrict__ vals,
                                                                 const unsigned int* __restrict__ base_tab, int width,
                                                                 float* __restrict__ img, unsigned long long* flags)
{
    convert32_body(vals, base_tab, width, img, flags);
}

__global__ void k_poly32_group_init(Poly32GroupArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// kPre: p = m r + beta p (degree 0). Else a.r is the stored z_d: p = z + beta p.
template <int kR, bool kPre>
__global__ __launch_bounds__(kBlock) void k_poly32_group_p(Poly32GroupArgs a, bool prologue)
{
    col_p<kR, kPre>(a, prologue);
}

// The outer SpMM of a member whose image is exact: the fp32 loops with the
// engine's end (hpccg_poly32.hip's forms and register budget).
template <int kW, int kR, bool kNT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_poly32_group_spmm_a(
    Poly32GroupArgs a, bool prologue)
{
    spmm32_a_body<kW, kR, kNT>(a, prologue);
}

template <int kR, bool kNT>
__global__ __launch_bounds__(kBlock) void k_poly32_group_spmm_sell(Poly32GroupArgs a, bool prologue)
{
    spmm32_sell_body<kR, kNT>(a, prologue);
}

// ... and of a member whose image is inexact: the fp64 loops, the poly
// library's forms and plan choices.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_poly32_group_spmm64_a(
    Poly32GroupArgs a, bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_poly32_group_spmm64_sell(Poly32GroupArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

template <int kR, bool kCheb>
__global__ __launch_bounds__(kBlock) void k_poly32_group_update(Poly32GroupArgs a, bool prologue)
{
    if constexpr (kCheb)
        poly_update0<kR>(a, prologue);
    else
        col_update<kR, true>(a, prologue);
}

// The fp32 loops with hpccg_poly_bodies.h's ends: step j applied to the row sums in registers.
template <int kW, int kR, bool kNT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_poly32_group_step(
    Poly32GroupArgs a)
{
    spmm32_a_body<kW, kR, kNT, Poly32GroupArgs, PolyStep>(a, false);
}

template <int kR, bool kNT>
__global__ __launch_bounds__(kBlock) void k_poly32_group_step_sell(Poly32GroupArgs a)
{
    spmm32_sell_body<kR, kNT, Poly32GroupArgs, PolyStep>(a, false);
}

// store_total: the totals are this member's parts of the dots and the state is
// left to k_poly32_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_poly32_group_finalize(Poly32GroupArgs a, int which, int store_total)
{
    col_finalize<true>(a, which, store_total);
}

__global__ void k_poly32_group_sum(Poly32GroupArgs a, GroupTotals g, int which)
{
    col_group_sum<true>(a, g, which);
}

// The halo of every column of one guarded buffer in one launch per member (hpccg_group.h).
__global__ __launch_bounds__(kHaloThreads) void k_poly32_group_halo(HaloArgs h)
{
    halo_body(h);
}

__global__ __launch_bounds__(kBlock) void k_poly32_group_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_poly32_group_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// The bound's kernels (hpccg_poly_bodies.h), on a member's rows of the fp64 image.
__global__ void k_poly32_group_q(const double* __restrict__ m, int n, double* __restrict__ q)
{
    poly_q_body(m, n, q);
}

__global__ __launch_bounds__(kBlock) void k_poly32_group_bound(DiagArgs a, const double* __restrict__ q,
                                                               double* __restrict__ smax)
{
    poly_bound_body(a, q, smax);
}

__global__ __launch_bounds__(kBlock) void k_poly32_group_bound_top(const double* __restrict__ smax, int nslices,
                                                                   double* __restrict__ out)
{
    poly_bound_top_body(smax, nslices, out);
}

// ---------------------------------------------------------------------------
// host: hpccg_poly_group_host.h over this unit's kernels, with every member's
// fp32 image (hpccg_spmm32.h) and the choice of the SpMM and step forms
// ---------------------------------------------------------------------------
// One member's workspace: the group poly library's, with the member's image.
struct Workspace : PolyWorkspace, GroupMember, Image32 {
    void free_own_rest()
    {
        PolyWorkspace::free_own_rest();
        destroy_events();
        free_image();
    }
    long long total_bytes() const { return PolyWorkspace::total_bytes() + img_bytes; }
};

template <bool kV>
using bool_c = std::integral_constant<bool, kV>;

// The fp32 forms of a chunk over the A image: f(width, kR, kNT), kNT from the view's flag.
template <class F>
void with_spmm32_form(const Poly32GroupArgs& a, int R, F f)
{
    using std::integral_constant;
    auto nt = [&](auto wd, auto r) {
        if (a.nt)
            f(wd, r, bool_c<true>{});
        else
            f(wd, r, bool_c<false>{});
    };
    if (a.a_width == 27)
        with_columns(R, [&](auto r) { nt(integral_constant<int, 27>{}, r); });
    else if (a.a_width == 7)
        with_columns(R, [&](auto r) { nt(integral_constant<int, 7>{}, r); });
    else
        with_columns(R, [&](auto r) { nt(integral_constant<int, 0>{}, r); });
}

// ... and over the SELL-512 image: f(kR, kNT).
template <class F>
void with_sell32_form(const Poly32GroupArgs& a, int R, F f)
{
    with_columns(R, [&](auto r) {
        if (a.nt)
            f(r, bool_c<true>{});
        else
            f(r, bool_c<false>{});
    });
}

struct GroupPoly32 {
    using Args = Poly32GroupArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "group poly32";
    // diagnostics: the halos by copies, the A/B of k_poly32_group_halo (tools/group_poly32_bench.py)
    static constexpr const char* halo_env = "HPCCG_GROUP_POLY32_HALO_COPIES";
    static long long row0(const Workspace* w) { return w->p0; }
    // member r's fp32 image: before its preconditioner, at every degree (one
    // verdict per member matrix; a refusal names the member)
    static int image(Workspace* w, int r)
    {
        char name[48];
        std::snprintf(name, sizeof name, "%s: member %d", who, r);
        return ensure_image32(w, w->v, k_poly32_group_convert, name);
    }

    static constexpr auto init = k_poly32_group_init;
    template <int kR, bool kPre>
    static constexpr auto p = k_poly32_group_p<kR, kPre>;
    // (the fp64 forms: the outer SpMM of a member whose image is inexact)
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_poly32_group_spmm64_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_poly32_group_spmm64_sell<kR>;
    template <int kR, bool kCheb>
    static constexpr auto update = k_poly32_group_update<kR, kCheb>;
    static constexpr auto finalize = k_poly32_group_finalize;
    static constexpr auto sum = k_poly32_group_sum;
    static constexpr auto halo = k_poly32_group_halo;
    static constexpr auto diag = k_poly32_group_diag;
    static constexpr auto check = k_poly32_group_check;
    static constexpr auto q = k_poly32_group_q;
    static constexpr auto bound = k_poly32_group_bound;
    static constexpr auto bound_top = k_poly32_group_bound_top;

    // Ap = A p on a member's rows: from its fp32 image where that is its rows
    // of the matrix, else from the fp64 image. Members may differ: the bits are
    // the same either way where the image is exact.
    static void launch_spmm(const Workspace* w, Args a, bool prologue)
    {
        if (w->inexact != 0) return launch_spmm64<GroupPoly32>(w, a, prologue);
        const dim3 g(a.grid), b(kBlock);
        hipStream_t s = w->v.stream;
        a.img = w->img;
        for_chunks(a.nrhs, true, [&](int c0, int R) {
            a.c0 = c0;
            if (!w->v.has_a)
                with_sell32_form(a, R, [&](auto r, auto nt) {
                    hipLaunchKernelGGL((k_poly32_group_spmm_sell<decltype(r)::value, decltype(nt)::value>), g, b, 0, s,
                                       a, prologue);
                });
            else
                with_spmm32_form(a, R, [&](auto wd, auto r, auto nt) {
                    hipLaunchKernelGGL(
                        (k_poly32_group_spmm_a<decltype(wd)::value, decltype(r)::value, decltype(nt)::value>), g, b, 0,
                        s, a, prologue);
                });
        });
    }

    // One step's launches on a member: always over its fp32 image.
    static void launch_step(const Workspace* w, Args a)
    {
        const dim3 g(a.grid), b(kBlock);
        hipStream_t s = w->v.stream;
        a.img = w->img;
        for_chunks(a.nrhs, true, [&](int c0, int R) {
            a.c0 = c0;
            if (!w->v.has_a)
                with_sell32_form(a, R, [&](auto r, auto nt) {
                    hipLaunchKernelGGL((k_poly32_group_step_sell<decltype(r)::value, decltype(nt)::value>), g, b, 0, s,
                                       a);
                });
            else
                with_spmm32_form(a, R, [&](auto wd, auto r, auto nt) {
                    hipLaunchKernelGGL(
                        (k_poly32_group_step<decltype(wd)::value, decltype(r)::value, decltype(nt)::value>), g, b, 0, s,
                        a);
                });
        });
    }
};

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_group_poly32_abi_version(void) { return 1; }

int hpccg_hip_group_poly32_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                        const long long* ldb, double* const* X_dev, const long long* ldx,
                                        const double* const* minv_dev, int degree, double lmin, double lmax,
                                        int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return group_poly_solve_device<GroupPoly32>(Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax,
                                                max_iter, tolerance, niters, normr, times);
}

int hpccg_hip_group_poly32_bound(hpccg_hip_matrix* const* Ms, int nranks, const double* const* minv_dev, double* lmax)
{
    return group_poly_bound<GroupPoly32>(Ms, nranks, minv_dev, lmax);
}

int hpccg_hip_group_poly32_last_spectrum(hpccg_hip_matrix* const* Ms, int nranks, double* lmin, double* lmax)
{
    return group_poly_last_spectrum<GroupPoly32>(Ms, nranks, lmin, lmax);
}

int hpccg_hip_group_poly32_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    return group_last_trace<GroupPoly32>(Ms, nranks, col, out, cap);
}

int hpccg_hip_group_poly32_info(hpccg_hip_matrix* const* Ms, int nranks, long long* out)
{
    TRY(check_group_args(GroupPoly32::who, Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "group poly32: out is NULL");
    for (int r = 0; r < nranks; r++)
        if (!Ms[r]) return fail(HPCCG_HIP_EINVAL, "group poly32: Ms[%d] is NULL", r);  // (before any is looked at)
    GroupOf<GroupPoly32> G;
    TRY(check_group(GroupPoly32::who, Ms, nranks, kOneForwarded, &G));
    return keep_device([&]() -> int {
        for (int r = 0; r < nranks; r++) {
            Workspace* w = nullptr;
            TRY(g_ws<Workspace>.record(Ms[r], G.v[r], &w));
            TRY(GroupPoly32::image(w, r));
            out[4 * r + 0] = w->inexact == 0 ? 1 : 0;
            out[4 * r + 1] = w->img_bytes;
            out[4 * r + 2] = w->inexact;
            out[4 * r + 3] = 0;
        }
        return 0;
    });
}

int hpccg_hip_group_poly32_release(hpccg_hip_matrix* M) { return unit_release<GroupPoly32>(M); }

int hpccg_hip_group_poly32_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<GroupPoly32>(M, bytes);
}

int hpccg_hip_group_poly32_live_workspaces(int* count) { return unit_live_workspaces<GroupPoly32>(count); }

}  // extern "C"
