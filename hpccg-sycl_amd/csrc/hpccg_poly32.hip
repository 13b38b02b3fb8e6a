// hpccg_poly32.hip -- Chebyshev polynomial preconditioned CG whose polynomial
// steps stream an fp32 image of the matrix (include/hpccg_hip_poly32.h,
// lib/libhpccg_hip_poly32.so): kernels and host code of the eighth library.
//
// hpccg_poly.hip's recurrence, statement for statement, with the matrix values
// of the steps read from an fp32 image A~ = fl32(A) (a value is widened in the
// register; every vector, product and sum is fp64). The preconditioner does not
// have to be exact: a polynomial in diag(m) A~ times diag(m) is still a fixed
// symmetric positive definite operator, so CG on the fp64 system keeps its
// theory and its fp64 answer. The outer SpMM (Ap = A p) streams the image only
// where it IS the matrix (every value survives the round trip through float);
// otherwise it streams the fp64 image through hpccg_spmm.h's loops, exactly as
// hpccg_poly.hip does. A step is then a pass over 4 B per slot instead of 8.
//   convert   k_poly32_convert: fp64 image -> fp32 image (hpccg_spmm32.h's
//             layout, the mixed library's), counts the values that do not
//             survive the round trip and those outside fp32 range
//   p update  k_poly32_p<kR, kPre>: the engine's body, as k_poly_p
//   SpMM      exact image: k_poly32_spmm_a<kW, kR, kNT> |
//             k_poly32_spmm_sell<kR, kNT>, the fp32 loops of hpccg_spmm32.h with
//             the engine's end; else k_poly32_spmm64_a<kW, kR, kWaves> |
//             k_poly32_spmm64_sell<kR>, the fp64 loops of hpccg_spmm.h (the poly
//             library's forms)
//   update    k_poly32_update<kR, kCheb>: as k_poly_update
//   step      k_poly32_step<kW, kR, kNT> | k_poly32_step_sell<kR, kNT>: the fp32
//             loops reading column c's z, with hpccg_poly_bodies.h's PolyStep as
//             the end: step j applied in registers (A~ z is never stored), the
//             last step forms the r.z slice partial
//   finalize, bound, diagonal: k_poly32_finalize, k_poly32_q, k_poly32_bound,
//             k_poly32_bound_top, k_poly32_diag, k_poly32_check over the shared
//             bodies; m, the bound and the coefficients come from the fp64 image
// The 27-wide four-column fp32 forms take the x-triple plan on interior slices,
// as the fp64 forms do (hpccg_spmm32.h: the same bits, a third of the x loads).
// z alternates between two buffers as in hpccg_poly.hip; per iteration and
// chunk of columns 5 + d launches. No kernel here waits on another block.
// The host code is hpccg_poly_host.h over hpccg_onerank_host.h, shared with
// hpccg_poly.hip (the latter also with hpccg_pcg.hip and hpccg_srcg.hip); what
// this unit adds is the image (hpccg_spmm32.h's Image32, built before the
// preconditioner) and the choice of the SpMM and step forms.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_poly32.h"
#include "hpccg_poly_host.h"
#include "hpccg_spmm32.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct Poly32Args : PolyArgs {
    const float* img;  // the fp32 values (hpccg_spmm32.h's layout)
};

// fp64 image -> fp32 image with the two counts: hpccg_spmm32.h's body.
__global__ __launch_bounds__(kBlock) void k_poly32_convert(const double* __restrict__ vals,
                                                           const unsigned int* __restrict__ base_tab, int width,
                                                           float* __restrict__ img, unsigned long long* flags)
{
    convert32_body(vals, base_tab, width, img, flags);
}

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_poly32_init(Poly32Args a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// kPre: p = m r + beta p (degree 0). Else a.r is the stored z (degree >= 1):
// p = z + beta p, the plain body.
template <int kR, bool kPre>
__global__ __launch_bounds__(kBlock) void k_poly32_p(Poly32Args a, bool prologue)
{
    col_p<kR, kPre>(a, prologue);
}

// The outer SpMM of an exact image: the fp32 loops with the engine's end.
// amdgpu_waves_per_eu(4): the register budget (at most 128 VGPRs), as the
// mixed library's forms.
template <int kW, int kR, bool kNT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_poly32_spmm_a(Poly32Args a,
                                                                                                 bool prologue)
{
    spmm32_a_body<kW, kR, kNT>(a, prologue);
}

template <int kR, bool kNT>
__global__ __launch_bounds__(kBlock) void k_poly32_spmm_sell(Poly32Args a, bool prologue)
{
    spmm32_sell_body<kR, kNT>(a, prologue);
}

// The outer SpMM of an inexact image: the fp64 loops, the poly library's forms
// and plan choices (kWaves 5 for the 27-wide four-column form over images
// streamed from HBM, else 4).
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_poly32_spmm64_a(Poly32Args a,
                                                                                                        bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_poly32_spmm64_sell(Poly32Args a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

// kCheb: hpccg_poly_bodies.h's update with step 0 in r's pass; else the engine's kPre body.
template <int kR, bool kCheb>
__global__ __launch_bounds__(kBlock) void k_poly32_update(Poly32Args a, bool prologue)
{
    if constexpr (kCheb)
        poly_update0<kR>(a, prologue);
    else
        col_update<kR, true>(a, prologue);
}

// The fp32 loops with hpccg_poly_bodies.h's ends: step j applied to the row sums in registers.
template <int kW, int kR, bool kNT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_poly32_step(Poly32Args a)
{
    spmm32_a_body<kW, kR, kNT, Poly32Args, PolyStep>(a, false);
}

template <int kR, bool kNT>
__global__ __launch_bounds__(kBlock) void k_poly32_step_sell(Poly32Args a)
{
    spmm32_sell_body<kR, kNT, Poly32Args, PolyStep>(a, false);
}

__global__ __launch_bounds__(kFinThreads) void k_poly32_finalize(Poly32Args a, int which, int store_total)
{
    col_finalize<true>(a, which, store_total);
}

// The diagonal of the image and the check of a caller's m: hpccg_jacobi.h's bodies.
__global__ __launch_bounds__(kBlock) void k_poly32_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_poly32_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// The symmetric Gershgorin bound's three kernels: hpccg_poly_bodies.h's bodies (over the fp64 image).
__global__ void k_poly32_q(const double* __restrict__ m, int n, double* __restrict__ q)
{
    poly_q_body(m, n, q);
}

__global__ __launch_bounds__(kBlock) void k_poly32_bound(DiagArgs a, const double* __restrict__ q,
                                                         double* __restrict__ smax)
{
    poly_bound_body(a, q, smax);
}

__global__ __launch_bounds__(kBlock) void k_poly32_bound_top(const double* __restrict__ smax, int nslices,
                                                             double* __restrict__ out)
{
    poly_bound_top_body(smax, nslices, out);
}

// ---------------------------------------------------------------------------
// host: hpccg_poly_host.h over this unit's kernels, with the fp32 image
// (hpccg_spmm32.h) and the choice of the SpMM and step forms
// ---------------------------------------------------------------------------
struct Workspace : PolyWorkspace, Image32 {
    void free_own_rest()
    {
        PolyWorkspace::free_own_rest();
        free_image();
    }
    long long total_bytes() const { return PolyWorkspace::total_bytes() + img_bytes; }
};

template <bool kV>
using bool_c = std::integral_constant<bool, kV>;

// The fp32 forms of a chunk over the A image: f(width, kR, kNT), kNT from the view's flag.
template <class F>
void with_spmm32_form(const Poly32Args& a, int R, F f)
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
void with_sell32_form(const Poly32Args& a, int R, F f)
{
    with_columns(R, [&](auto r) {
        if (a.nt)
            f(r, bool_c<true>{});
        else
            f(r, bool_c<false>{});
    });
}

struct Poly32 {
    using Args = Poly32Args;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "poly32";
    static constexpr const char* solve_name = "poly32";
    static long long row0(const Workspace* w) { return w->v.guard_rows; }
    // the fp32 image: before the preconditioner, at every degree (one verdict per matrix)
    static int image(Workspace* w) { return ensure_image32(w, w->v, k_poly32_convert, who); }

    static constexpr auto init = k_poly32_init;
    template <int kR, bool kPre>
    static constexpr auto p = k_poly32_p<kR, kPre>;
    // (the fp64 forms: the outer SpMM of an inexact image)
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_poly32_spmm64_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_poly32_spmm64_sell<kR>;
    template <int kR, bool kCheb>
    static constexpr auto update = k_poly32_update<kR, kCheb>;
    static constexpr auto finalize = k_poly32_finalize;
    static constexpr auto diag = k_poly32_diag;
    static constexpr auto check = k_poly32_check;
    static constexpr auto q = k_poly32_q;
    static constexpr auto bound = k_poly32_bound;
    static constexpr auto bound_top = k_poly32_bound_top;

    // Ap = A p: from the fp32 image where it is the matrix, else from the fp64 image.
    static void launch_spmm(const Workspace* w, Args a, bool prologue)
    {
        if (w->inexact != 0) return launch_spmm64<Poly32>(w, a, prologue);
        const dim3 g(a.grid), b(kBlock);
        hipStream_t s = w->v.stream;
        a.img = w->img;
        for_chunks(a.nrhs, true, [&](int c0, int R) {
            a.c0 = c0;
            if (!w->v.has_a)
                with_sell32_form(a, R, [&](auto r, auto nt) {
                    hipLaunchKernelGGL((k_poly32_spmm_sell<decltype(r)::value, decltype(nt)::value>), g, b, 0, s, a,
                                       prologue);
                });
            else
                with_spmm32_form(a, R, [&](auto wd, auto r, auto nt) {
                    hipLaunchKernelGGL((k_poly32_spmm_a<decltype(wd)::value, decltype(r)::value, decltype(nt)::value>),
                                       g, b, 0, s, a, prologue);
                });
        });
    }

    // One step's launches: always over the fp32 image.
    static void launch_step(const Workspace* w, Args a)
    {
        const dim3 g(a.grid), b(kBlock);
        hipStream_t s = w->v.stream;
        a.img = w->img;
        for_chunks(a.nrhs, true, [&](int c0, int R) {
            a.c0 = c0;
            if (!w->v.has_a)
                with_sell32_form(a, R, [&](auto r, auto nt) {
                    hipLaunchKernelGGL((k_poly32_step_sell<decltype(r)::value, decltype(nt)::value>), g, b, 0, s, a);
                });
            else
                with_spmm32_form(a, R, [&](auto wd, auto r, auto nt) {
                    hipLaunchKernelGGL((k_poly32_step<decltype(wd)::value, decltype(r)::value, decltype(nt)::value>),
                                       g, b, 0, s, a);
                });
        });
    }
};

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_poly32_abi_version(void) { return 1; }

int hpccg_hip_poly32_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                  long long ldx, const double* minv_dev, int degree, double lmin, double lmax,
                                  int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_common<Poly32>(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance,
                                niters, normr, times, false, Poly32::image);
}

int hpccg_hip_poly32_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                           const double* minv, int degree, double lmin, double lmax, int max_iter, double tolerance,
                           int* niters, double* normr, double* times)
{
    return solve_common<Poly32>(M, nrhs, B, ldb, X, ldx, minv, degree, lmin, lmax, max_iter, tolerance, niters, normr,
                                times, true, Poly32::image);
}

int hpccg_hip_poly32_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax)
{
    return poly_bound<Poly32>(M, minv_dev, lmax);
}

int hpccg_hip_poly32_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax)
{
    return poly_last_spectrum<Poly32>(M, lmin, lmax);
}

int hpccg_hip_poly32_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    return unit_last_trace<Poly32>(M, col, out, cap);
}

int hpccg_hip_poly32_info(hpccg_hip_matrix* M, long long out[4])
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    MatrixView v;
    TRY(check_matrix(Poly32::who, M, &v));
    out[0] = 1;
    out[1] = out[2] = out[3] = 0;
    if (v.n == 0) return 0;
    return keep_device([&]() -> int {
        Workspace* w = nullptr;
        TRY(g_ws<Workspace>.record(M, v, &w));
        TRY(Poly32::image(w));
        out[0] = w->inexact == 0 ? 1 : 0;
        out[1] = w->img_bytes;
        out[2] = w->inexact;
        return 0;
    });
}

int hpccg_hip_poly32_release(hpccg_hip_matrix* M) { return unit_release<Poly32>(M); }

int hpccg_hip_poly32_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Poly32>(M, bytes);
}

int hpccg_hip_poly32_live_workspaces(int* count) { return unit_live_workspaces<Poly32>(count); }

}  // extern "C"
