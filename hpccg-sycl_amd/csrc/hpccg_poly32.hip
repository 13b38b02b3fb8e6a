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
// The host code follows hpccg_poly.hip's function for function (that unit is
// left as it is, so its code object keeps its bits); what differs is the image
// and the choice of the SpMM and step forms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "../../include/hpccg_hip_poly32.h"
#include "hpccg_columns.h"
#include "hpccg_jacobi.h"
#include "hpccg_poly_bodies.h"
#include "hpccg_poly_coeffs.h"
#include "hpccg_spmm.h"
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
// host
// ---------------------------------------------------------------------------
struct Workspace : TraceWorkspace, JacobiCache {
    // the fp32 image (kept while the columns grow; counted in img_bytes)
    float* img = nullptr;
    long long img_bytes = 0;
    bool built = false;
    long long inexact = 0, out_of_range = 0;
    double *r = nullptr, *x = nullptr, *b = nullptr;
    double *dd = nullptr, *zbuf = nullptr;  // zbuf: two sets of cap columns in p's layout
    // the bound's vectors (kept while the columns grow, counted in rest_bytes)
    double *qbuf = nullptr, *smax = nullptr, *lmax_dev = nullptr;
    bool jac_lmax_built = false;
    double jac_lmax = 0.0;  // the bound with m = 1 / a_ii
    // the call being run
    int degree = 0;
    double cheb0 = 0.0, aj[kPolyMaxDegree + 1] = {}, bj[kPolyMaxDegree + 1] = {};
    bool solved = false;
    double last_lmin = 0.0, last_lmax = 0.0;

    Workspace() { ndots = 3; }

    void free_own_vectors()
    {
        for (double* q : {r, x, b, dd, zbuf})
            if (q) (void)hipFree(q);
        r = x = b = dd = zbuf = nullptr;
    }
    void free_bound_vectors()
    {
        for (double* q : {qbuf, smax, lmax_dev})
            if (q) (void)hipFree(q);
        qbuf = smax = lmax_dev = nullptr;
    }
    void free_own_rest()
    {
        free_bound_vectors();
        free_cache();
        if (img) (void)hipFree(img);
        img = nullptr;
        img_bytes = 0;
    }
};

long long p_column(const MatrixView& v)
{
    return (long long)v.npad + 2 * v.guard_rows;  // [guard | rows (padded) | guard]
}

// What the library runs on: one rank, no halo.
int check_matrix(hpccg_hip_matrix* M, MatrixView* v)
{
    TRY(hpccg_hip_internal_view(M, v));
    if (v->in_group) return fail(HPCCG_HIP_EINVAL, "poly32: the matrix is a member of an in-process group (one rank only)");
    if (v->nranks > 1) return fail(HPCCG_HIP_EINVAL, "poly32: the matrix belongs to a communicator of %d ranks (one rank only)", v->nranks);
    if (v->ghost_lo || v->ghost_hi) return fail(HPCCG_HIP_EINVAL, "poly32: the matrix has halo rows (one rank only)");
    if (!v->has_a && !v->has_sell) return fail(HPCCG_HIP_EINVAL, "poly32: the matrix holds no device image");
    return 0;
}

int out_of_range(const Workspace* w)
{
    return fail(HPCCG_HIP_EINVAL,
                "poly32: the matrix is outside fp32 range (%lld stored values with no finite, normal fp32 image)",
                w->out_of_range);
}

// The fp32 image, built once per matrix on the device from the image it holds.
int ensure_image(Workspace* w)
{
    if (w->built) return w->out_of_range ? out_of_range(w) : 0;
    const MatrixView& v = w->v;
    hipStream_t s = v.stream;
    HIP_TRY(hipSetDevice(v.device));
    const double* vals = v.has_a ? v.aval : v.vals;
    const unsigned int* tab = v.has_a ? v.abase : v.slice_base;
    const int width = v.has_a ? v.a_width : 0;
    long long slot_rows = (long long)v.nslices * width;
    if (width <= 0) {
        unsigned int last = 0;
        HIP_TRY(hipMemcpyAsync(&last, tab + v.nslices, sizeof last, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        slot_rows = last;
    }
    const size_t bytes = sizeof(float) * (size_t)std::max<long long>(slot_rows, 1) * kSliceRows;
    unsigned long long* flags = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w->img), bytes));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&flags), 2 * sizeof *flags);
    unsigned long long h[2] = {0, 0};
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, 2 * sizeof *flags, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_poly32_convert, dim3(v.nslices), dim3(kBlock), 0, s, vals, tab, width, w->img, flags);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (flags) (void)hipFree(flags);
    if (e != hipSuccess) {
        (void)hipFree(w->img);
        w->img = nullptr;
        return fail(e == hipErrorOutOfMemory ? HPCCG_HIP_ENOMEM : HPCCG_HIP_EHIP, "poly32: building the fp32 image: %s",
                    hipGetErrorString(e));
    }
    w->built = true;
    w->inexact = (long long)h[0];
    w->out_of_range = (long long)h[1];
    w->img_bytes = (long long)bytes;
    if (w->out_of_range) {  // never solved with: the image goes, the verdict stays
        (void)hipFree(w->img);
        w->img = nullptr;
        w->img_bytes = 0;
        return out_of_range(w);
    }
    return 0;
}

// Jacobi: the cached 1.0 / a_ii, or the refusal of a matrix it does not exist for.
int ensure_jacobi(Workspace* w)
{
    int row = -1;
    TRY(build_jacobi(w, k_poly32_diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "poly32: Jacobi needs a finite diagonal > 0 in every row; row %d is the first whose diagonal is "
                    "missing, not finite or <= 0",
                    row);
    return 0;
}

// A call's own m: into the padded muser, every entry finite and > 0.
int stage_minv(Workspace* w, const double* minv, bool host)
{
    int row = -1;
    TRY(load_minv(w, minv, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, k_poly32_check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "poly32: minv[%d] is not finite and > 0 (the first such entry)", row);
    return 0;
}

// The bound's vectors (zeroed: q's guard zones and its rows past n are read and never stored).
int ensure_bound_vectors(Workspace* w)
{
    if (w->qbuf) return 0;
    HIP_TRY(hipSetDevice(w->v.device));
    const long long before = w->bytes;  // (alloc_zero counts into bytes: the columns')
    int rc = alloc_zero(w, &w->qbuf, (size_t)p_column(w->v));
    if (!rc) rc = alloc_zero(w, &w->smax, (size_t)std::max(w->v.nslices, 1));
    if (!rc) rc = alloc_zero(w, &w->lmax_dev, 1);
    if (rc)
        w->free_bound_vectors();
    else
        w->rest_bytes += w->bytes - before;
    w->bytes = before;
    return rc;
}

// The symmetric Gershgorin bound with the padded device vector m (the fp64 image's).
int compute_bound(Workspace* w, const double* m, double* lmax)
{
    const MatrixView& v = w->v;
    hipStream_t s = v.stream;
    TRY(ensure_bound_vectors(w));
    double* q = w->qbuf + v.guard_rows;
    hipLaunchKernelGGL(k_poly32_q, dim3((v.n + 255) / 256), dim3(256), 0, s, m, v.n, q);
    hipLaunchKernelGGL(k_poly32_bound, dim3(v.nslices), dim3(kBlock), 0, s, diag_args(v), (const double*)q, w->smax);
    hipLaunchKernelGGL(k_poly32_bound_top, dim3(1), dim3(kBlock), 0, s, (const double*)w->smax, v.nslices,
                       w->lmax_dev);
    HIP_TRY(hipGetLastError());
    double h = 0.0;
    HIP_TRY(hipMemcpyAsync(&h, w->lmax_dev, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!(h > 0.0 && std::isfinite(h)))
        return fail(HPCCG_HIP_EINVAL, "poly32: the Gershgorin bound of the matrix is %g (finite and > 0 needed)", h);
    *lmax = h;
    return 0;
}

// Jacobi's bound: cached with 1 / a_ii.
int jacobi_bound(Workspace* w, double* lmax)
{
    if (!w->jac_lmax_built) {
        TRY(compute_bound(w, w->jac, &w->jac_lmax));
        w->jac_lmax_built = true;
    }
    *lmax = w->jac_lmax;
    return 0;
}

// Room for ncols columns and a history of max_iter + 1 entries per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter)
{
    const size_t npad = (size_t)w->v.npad;
    const long long pcs = p_column(w->v);
    return ensure_columns(w, ncols, max_iter, true, pcs, 0, [&](int cap) {
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        TRY(alloc_zero(w, &w->dd, npad * cap));
        // zeroed: z's guard zones and the rows past n are read and never stored
        TRY(alloc_zero(w, &w->zbuf, 2 * (size_t)pcs * cap));
        return 0;
    });
}

// z buffer `which` (0, 1): local row 0 of column 0
double* z_of(const Workspace* w, int which)
{
    return w->zbuf + (size_t)which * (size_t)w->pcs * (size_t)w->cap + w->v.guard_rows;
}

Poly32Args make_args(const Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    Poly32Args a{};
    fill_args(&a, w, nrhs);
    a.tri = 1;
    a.p = w->pbuf + v.guard_rows;
    a.r = w->r;
    a.rcs = w->vcs;
    a.x = w->x;
    a.b = w->b;
    a.minv = m;
    a.aval = v.aval;
    a.vals = v.vals;
    a.dd = w->dd;
    a.cheb0 = w->cheb0;
    a.img = w->img;
    return a;
}

template <bool kV>
using bool_c = std::integral_constant<bool, kV>;

// f(std::integral_constant<int, kR>) for the chunk's column count R = 1, 2, 4.
template <class F>
void with_columns(int R, F f)
{
    if (R == 4)
        f(std::integral_constant<int, 4>{});
    else if (R == 2)
        f(std::integral_constant<int, 2>{});
    else
        f(std::integral_constant<int, 1>{});
}

// The fp64 SpMM forms of a chunk (the poly library's plan choices): f(width, kR, kWaves).
template <class F>
void with_spmm64_form(const Poly32Args& a, int R, F f)
{
    using std::integral_constant;
    if (a.a_width == 27 && R == 4 && a.nt)
        f(integral_constant<int, 27>{}, integral_constant<int, 4>{}, integral_constant<int, 5>{});
    else if (a.a_width == 27)
        with_columns(R, [&](auto r) { f(integral_constant<int, 27>{}, r, integral_constant<int, 4>{}); });
    else if (a.a_width == 7)
        with_columns(R, [&](auto r) { f(integral_constant<int, 7>{}, r, integral_constant<int, 4>{}); });
    else
        with_columns(R, [&](auto r) { f(integral_constant<int, 0>{}, r, integral_constant<int, 4>{}); });
}

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

// Ap = A p: from the fp32 image where it is the matrix, else from the fp64 image.
void launch_spmm(const Workspace* w, Poly32Args a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    const bool exact = w->inexact == 0;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (exact && !w->v.has_a)
            with_sell32_form(a, R, [&](auto r, auto nt) {
                hipLaunchKernelGGL((k_poly32_spmm_sell<decltype(r)::value, decltype(nt)::value>), g, b, 0, s, a,
                                   prologue);
            });
        else if (exact)
            with_spmm32_form(a, R, [&](auto wd, auto r, auto nt) {
                hipLaunchKernelGGL((k_poly32_spmm_a<decltype(wd)::value, decltype(r)::value, decltype(nt)::value>), g,
                                   b, 0, s, a, prologue);
            });
        else if (!w->v.has_a)
            with_columns(R, [&](auto r) {
                hipLaunchKernelGGL((k_poly32_spmm64_sell<decltype(r)::value>), g, b, 0, s, a, prologue);
            });
        else
            with_spmm64_form(a, R, [&](auto wd, auto r, auto wv) {
                hipLaunchKernelGGL((k_poly32_spmm64_a<decltype(wd)::value, decltype(r)::value, decltype(wv)::value>),
                                   g, b, 0, s, a, prologue);
            });
    });
}

// d == 0: z = m r in the register; else the last step's z in r's place.
void launch_p(const Workspace* w, Poly32Args a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    const int d = w->degree;
    if (d > 0) {
        a.r = z_of(w, d & 1);
        a.rcs = a.pcs;
    }
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        with_columns(R, [&](auto r) {
            if (d > 0)
                hipLaunchKernelGGL((k_poly32_p<decltype(r)::value, false>), g, b, 0, s, a, prologue);
            else
                hipLaunchKernelGGL((k_poly32_p<decltype(r)::value, true>), g, b, 0, s, a, prologue);
        });
    });
}

// One step's launches: always over the fp32 image.
void launch_step(const Workspace* w, Poly32Args a)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            with_sell32_form(a, R, [&](auto r, auto nt) {
                hipLaunchKernelGGL((k_poly32_step_sell<decltype(r)::value, decltype(nt)::value>), g, b, 0, s, a);
            });
        else
            with_spmm32_form(a, R, [&](auto wd, auto r, auto nt) {
                hipLaunchKernelGGL((k_poly32_step<decltype(wd)::value, decltype(r)::value, decltype(nt)::value>), g, b,
                                   0, s, a);
            });
    });
}

// The update with step 0, then steps 1 .. d: z_d ends in buffer d & 1.
void launch_update(const Workspace* w, Poly32Args a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    const int d = w->degree;
    a.zout = z_of(w, 0);
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        with_columns(R, [&](auto r) {
            if (d > 0)
                hipLaunchKernelGGL((k_poly32_update<decltype(r)::value, true>), g, b, 0, s, a, prologue);
            else
                hipLaunchKernelGGL((k_poly32_update<decltype(r)::value, false>), g, b, 0, s, a, prologue);
        });
    });
    for (int j = 1; j <= d; j++) {
        a.zin = z_of(w, (j - 1) & 1);
        a.zout = z_of(w, j & 1);
        a.aj = w->aj[j];
        a.bj = w->bj[j];
        a.last = j == d;
        launch_step(w, a);
    }
}

void launch_finalize(const Workspace* w, const Poly32Args& a, int which, int store_total = 0)
{
    hipLaunchKernelGGL(k_poly32_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, store_total);
}

// The preconditioned CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    hipStream_t s = w->v.stream;
    const Poly32Args a = make_args(w, nrhs, m);
    HIP_TRY(hipEventRecord(w->ev0, s));
    hipLaunchKernelGGL(k_poly32_init, dim3((nrhs + 63) / 64), dim3(64), 0, s, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p, launch_spmm, launch_update, launch_finalize));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

// A caller's bounds: each finite and >= 0 (0.0: the default); both given, lmin < lmax.
int check_bounds(double lmin, double lmax)
{
    if (!(std::isfinite(lmin) && std::isfinite(lmax) && lmin >= 0.0 && lmax >= 0.0))
        return fail(HPCCG_HIP_EINVAL,
                    "poly32: spectrum bounds lmin %g, lmax %g (finite and >= 0 needed; 0: the default)", lmin, lmax);
    if (lmax > 0.0 && lmin >= lmax)
        return fail(HPCCG_HIP_EINVAL, "poly32: spectrum bounds lmin %g >= lmax %g", lmin, lmax);
    return 0;
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int degree, double lmin, double lmax, int max_iter, double tol, int* niters,
                 double* normr, double* times, bool host)
{
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "poly32: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "poly32: max_iter %d is negative", max_iter);
    // (below every row count, so refused before the matrix is looked at)
    if (ldb < 0 || ldx < 0)
        return fail(HPCCG_HIP_EINVAL, "poly32: leading dimensions %lld, %lld are negative", ldb, ldx);
    if (degree < 0 || degree > kPolyMaxDegree)
        return fail(HPCCG_HIP_EINVAL, "poly32: degree %d (0 to %d)", degree, kPolyMaxDegree);
    TRY(check_bounds(lmin, lmax));
    MatrixView v;
    TRY(check_matrix(M, &v));
    if (ldb < v.n || ldx < v.n)
        return fail(HPCCG_HIP_EINVAL, "poly32: leading dimensions %lld, %lld below the %d rows", ldb, ldx, v.n);
    if (times) std::fill(times, times + 7, 0.0);
    if (v.n == 0) {
        for (int c = 0; c < nrhs; c++) {
            niters[c] = 0;
            normr[c] = 0.0;
        }
        return 0;
    }
    if (max_iter < 1) max_iter = 1;
    return keep_device([&]() -> int {
        Workspace* w = nullptr;
        TRY(g_ws<Workspace>.record(M, v, &w));
        // the image first (at every degree: one verdict per matrix), then the
        // preconditioner: a refused call leaves X as it is
        TRY(ensure_image(w));
        TRY(ensure_cache(w));
        if (minv)
            TRY(stage_minv(w, minv, host));
        else
            TRY(ensure_jacobi(w));
        const double* m = minv ? w->muser : w->jac;
        // the interval (degree 0 applies no polynomial and needs none)
        if (degree > 0) {
            if (lmax == 0.0) TRY(minv ? compute_bound(w, m, &lmax) : jacobi_bound(w, &lmax));
            if (lmin == 0.0) lmin = lmax / kPolyEigRatio;
            if (!(lmin > 0.0 && lmin < lmax))
                return fail(HPCCG_HIP_EINVAL, "poly32: spectrum bounds lmin %g >= lmax %g", lmin, lmax);
            poly_coefficients(lmin, lmax, degree, &w->cheb0, w->aj, w->bj);
        } else if (lmin == 0.0 && lmax > 0.0) {
            lmin = lmax / kPolyEigRatio;
        }
        TRY(ensure_vectors(w, nrhs, max_iter));
        w->degree = degree;
        w->last_lmin = lmin;
        w->last_lmax = lmax;
        w->solved = true;
        const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        const hipMemcpyKind out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        const auto t0 = std::chrono::steady_clock::now();
        TRY(copy_cols(w, w->b, w->vcs, B, ldb, nrhs, in));
        TRY(copy_cols(w, w->x, w->vcs, X, ldx, nrhs, in));
        if (host) HIP_TRY(hipStreamSynchronize(v.stream));
        const auto t1 = std::chrono::steady_clock::now();
        double wall = 0.0;
        TRY(run_cg(w, nrhs, m, max_iter, tol, niters, normr, &wall));
        const auto t2 = std::chrono::steady_clock::now();
        TRY(copy_cols(w, X, ldx, w->x, w->vcs, nrhs, out));
        HIP_TRY(hipStreamSynchronize(v.stream));
        const auto t3 = std::chrono::steady_clock::now();
        if (times) {
            times[0] = wall;
            if (host) times[6] = std::chrono::duration<double>((t1 - t0) + (t3 - t2)).count();
        }
        return 0;
    });
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_poly32_abi_version(void) { return 1; }

int hpccg_hip_poly32_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                  long long ldx, const double* minv_dev, int degree, double lmin, double lmax,
                                  int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance, niters,
                        normr, times, false);
}

int hpccg_hip_poly32_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                           const double* minv, int degree, double lmin, double lmax, int max_iter, double tolerance,
                           int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B, ldb, X, ldx, minv, degree, lmin, lmax, max_iter, tolerance, niters, normr, times,
                        true);
}

int hpccg_hip_poly32_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax)
{
    if (!M || !lmax) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    MatrixView v;
    TRY(check_matrix(M, &v));
    if (v.n == 0) {
        *lmax = 0.0;
        return 0;
    }
    return keep_device([&]() -> int {
        Workspace* w = nullptr;
        TRY(g_ws<Workspace>.record(M, v, &w));
        TRY(ensure_cache(w));
        if (minv_dev) {
            TRY(stage_minv(w, minv_dev, false));
            return compute_bound(w, w->muser, lmax);
        }
        TRY(ensure_jacobi(w));
        return jacobi_bound(w, lmax);
    });
}

int hpccg_hip_poly32_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax)
{
    if (!M || !lmin || !lmax) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    if (!w || !w->solved) return fail(HPCCG_HIP_EINVAL, "poly32: no spectrum (no poly32 solve ran on the matrix)");
    *lmin = w->last_lmin;
    *lmax = w->last_lmax;
    return 0;
}

int hpccg_hip_poly32_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "poly32: no trace of column %d (the last poly32 solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

int hpccg_hip_poly32_info(hpccg_hip_matrix* M, long long out[4])
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    MatrixView v;
    TRY(check_matrix(M, &v));
    out[0] = 1;
    out[1] = out[2] = out[3] = 0;
    if (v.n == 0) return 0;
    return keep_device([&]() -> int {
        Workspace* w = nullptr;
        TRY(g_ws<Workspace>.record(M, v, &w));
        TRY(ensure_image(w));
        out[0] = w->inexact == 0 ? 1 : 0;
        out[1] = w->img_bytes;
        out[2] = w->inexact;
        return 0;
    });
}

int hpccg_hip_poly32_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    g_ws<Workspace>.drop(M);
    return 0;
}

int hpccg_hip_poly32_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    *bytes = w ? w->bytes + w->rest_bytes + w->img_bytes : 0;
    return 0;
}

int hpccg_hip_poly32_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "poly32: NULL argument");
    *count = g_ws<Workspace>.live();
    return 0;
}

}  // extern "C"
