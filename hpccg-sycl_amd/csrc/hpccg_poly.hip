// hpccg_poly.hip -- Chebyshev polynomial preconditioned CG
// (include/hpccg_hip_poly.h, lib/libhpccg_hip_poly.so): kernels and host code
// of the sixth library.
//
// The pcg library's preconditioner is a diagonal, which repairs bad row
// scaling and nothing else. This unit applies a fixed polynomial in M^-1 A
// times M^-1 (M^-1 = diag(m), by default Jacobi) in its place: the Chebyshev
// iteration of degree d on the interval [lmin, lmax] of M^-1 A's spectrum, from
// a zero start. Per column (the header has the whole recurrence):
//   step 0:  t = m r;  dd = c0 t;  z = dd
//   step j:  w = A z;  t = m (r - w);  dd = a_j dd + b_j t;  z = z + dd
// It costs d more passes over the matrix per iteration and buys iterations.
//   p update  k_poly_p<kR, kPre>: the engine's body; d == 0: z = m r in the
//             register (kPre), d >= 1: the stored z in r's place
//   SpMM      k_poly_spmm_a<kW, kR, kWaves> | k_poly_spmm_sell<kR>: Ap = A p,
//             the fp64 loops of hpccg_spmm.h (the pcg library's forms)
//   update    k_poly_update<kR, false>: the engine's kPre body (d == 0) |
//             <kR, true>: its statements with step 0 in r's pass (dd and z
//             stored, no r.z partial: the last step forms it)
//   step      k_poly_step<kW, kR, kWaves> | k_poly_step_sell<kR>: the same
//             loops reading column c's z; the epilogue applies step j in
//             registers (A z is never stored) and, in the last step, forms the
//             r.z slice partial
//   finalize  k_poly_finalize: the engine's kPre body
//   bound     k_poly_q, k_poly_bound, k_poly_bound_top: the symmetric
//             Gershgorin bound max_i q_i sum_j |a_ij| q_j, q = sqrt(m)
//   diagonal  k_poly_diag | k_poly_check (hpccg_jacobi.h's bodies)
// z is read at neighbour offsets by other blocks of a step's launch, so it
// lives in two buffers of p's column layout that the steps alternate between:
// step j reads buffer (j - 1) & 1 and stores buffer j & 1. Per iteration and
// chunk of columns 5 + d launches: p, SpMM, finalize, update, d steps,
// finalize. No kernel here waits on another block.
// The device code of the application -- PolyArgs, the update with step 0, the
// steps' ends, the bound's bodies -- is hpccg_poly_bodies.h, shared with the
// unit over an in-process rank group (hpccg_poly_group.hip); the __global__
// entry points here are wrappers over it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "../../include/hpccg_hip_poly.h"
#include "hpccg_columns.h"
#include "hpccg_jacobi.h"
#include "hpccg_poly_bodies.h"
#include "hpccg_poly_coeffs.h"
#include "hpccg_spmm.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_poly_init(PolyArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// kPre: p = m r + beta p (degree 0). Else a.r is the stored z (degree >= 1):
// p = z + beta p, the plain body.
template <int kR, bool kPre>
__global__ __launch_bounds__(kBlock) void k_poly_p(PolyArgs a, bool prologue)
{
    col_p<kR, kPre>(a, prologue);
}

// The pcg library's plan choices: kWaves 5 for the 27-wide four-column form
// over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_poly_spmm_a(PolyArgs a,
                                                                                                    bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_poly_spmm_sell(PolyArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

// kCheb: hpccg_poly_bodies.h's update with step 0 in r's pass; else the engine's kPre body.
template <int kR, bool kCheb>
__global__ __launch_bounds__(kBlock) void k_poly_update(PolyArgs a, bool prologue)
{
    if constexpr (kCheb)
        poly_update0<kR>(a, prologue);
    else
        col_update<kR, true>(a, prologue);
}

// The SpMM loops with hpccg_poly_bodies.h's ends: step j applied to the row sums in registers.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_poly_step(PolyArgs a)
{
    spmm_a_body<kW, kR, PolyArgs, PolyStep>(a, false);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_poly_step_sell(PolyArgs a)
{
    spmm_sell_body<kR, PolyArgs, PolyStep>(a, false);
}

__global__ __launch_bounds__(kFinThreads) void k_poly_finalize(PolyArgs a, int which, int store_total)
{
    col_finalize<true>(a, which, store_total);
}

// The diagonal of the image and the check of a caller's m: hpccg_jacobi.h's bodies.
__global__ __launch_bounds__(kBlock) void k_poly_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_poly_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// The symmetric Gershgorin bound's three kernels: hpccg_poly_bodies.h's bodies.
// q_i = sqrt(m_i) for the n rows (q: local row 0 of the guarded copy)
__global__ void k_poly_q(const double* __restrict__ m, int n, double* __restrict__ q)
{
    poly_q_body(m, n, q);
}

// One block per slice, a thread its two rows: smax[s] = max of g over the slice's rows < n.
__global__ __launch_bounds__(kBlock) void k_poly_bound(DiagArgs a, const double* __restrict__ q,
                                                       double* __restrict__ smax)
{
    poly_bound_body(a, q, smax);
}

// One block: *out = max of the nslices slice maxima.
__global__ __launch_bounds__(kBlock) void k_poly_bound_top(const double* __restrict__ smax, int nslices,
                                                           double* __restrict__ out)
{
    poly_bound_top_body(smax, nslices, out);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct Workspace : TraceWorkspace, JacobiCache {
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
    if (v->in_group) return fail(HPCCG_HIP_EINVAL, "poly: the matrix is a member of an in-process group (one rank only)");
    if (v->nranks > 1) return fail(HPCCG_HIP_EINVAL, "poly: the matrix belongs to a communicator of %d ranks (one rank only)", v->nranks);
    if (v->ghost_lo || v->ghost_hi) return fail(HPCCG_HIP_EINVAL, "poly: the matrix has halo rows (one rank only)");
    if (!v->has_a && !v->has_sell) return fail(HPCCG_HIP_EINVAL, "poly: the matrix holds no device image");
    return 0;
}

// Jacobi: the cached 1.0 / a_ii, or the refusal of a matrix it does not exist for.
int ensure_jacobi(Workspace* w)
{
    int row = -1;
    TRY(build_jacobi(w, k_poly_diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "poly: Jacobi needs a finite diagonal > 0 in every row; row %d is the first whose diagonal is "
                    "missing, not finite or <= 0",
                    row);
    return 0;
}

// A call's own m: into the padded muser, every entry finite and > 0.
int stage_minv(Workspace* w, const double* minv, bool host)
{
    int row = -1;
    TRY(load_minv(w, minv, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, k_poly_check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "poly: minv[%d] is not finite and > 0 (the first such entry)", row);
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

// The symmetric Gershgorin bound with the padded device vector m.
int compute_bound(Workspace* w, const double* m, double* lmax)
{
    const MatrixView& v = w->v;
    hipStream_t s = v.stream;
    TRY(ensure_bound_vectors(w));
    double* q = w->qbuf + v.guard_rows;
    hipLaunchKernelGGL(k_poly_q, dim3((v.n + 255) / 256), dim3(256), 0, s, m, v.n, q);
    hipLaunchKernelGGL(k_poly_bound, dim3(v.nslices), dim3(kBlock), 0, s, diag_args(v), (const double*)q, w->smax);
    hipLaunchKernelGGL(k_poly_bound_top, dim3(1), dim3(kBlock), 0, s, (const double*)w->smax, v.nslices, w->lmax_dev);
    HIP_TRY(hipGetLastError());
    double h = 0.0;
    HIP_TRY(hipMemcpyAsync(&h, w->lmax_dev, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!(h > 0.0 && std::isfinite(h)))
        return fail(HPCCG_HIP_EINVAL, "poly: the Gershgorin bound of the matrix is %g (finite and > 0 needed)", h);
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

PolyArgs make_args(const Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    PolyArgs a{};
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
    return a;
}

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

// The SpMM forms of a chunk (the pcg library's plan choices): f(width, kR, kWaves).
template <class F>
void with_spmm_form(const PolyArgs& a, int R, F f)
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

void launch_spmm(const Workspace* w, PolyArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            with_columns(R, [&](auto r) {
                hipLaunchKernelGGL((k_poly_spmm_sell<decltype(r)::value>), g, b, 0, s, a, prologue);
            });
        else
            with_spmm_form(a, R, [&](auto wd, auto r, auto wv) {
                hipLaunchKernelGGL((k_poly_spmm_a<decltype(wd)::value, decltype(r)::value, decltype(wv)::value>), g, b,
                                   0, s, a, prologue);
            });
    });
}

// d == 0: z = m r in the register; else the last step's z in r's place.
void launch_p(const Workspace* w, PolyArgs a, bool prologue)
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
                hipLaunchKernelGGL((k_poly_p<decltype(r)::value, false>), g, b, 0, s, a, prologue);
            else
                hipLaunchKernelGGL((k_poly_p<decltype(r)::value, true>), g, b, 0, s, a, prologue);
        });
    });
}

// One step's launches: the SpMM's forms.
void launch_step(const Workspace* w, PolyArgs a)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            with_columns(R, [&](auto r) { hipLaunchKernelGGL((k_poly_step_sell<decltype(r)::value>), g, b, 0, s, a); });
        else
            with_spmm_form(a, R, [&](auto wd, auto r, auto wv) {
                hipLaunchKernelGGL((k_poly_step<decltype(wd)::value, decltype(r)::value, decltype(wv)::value>), g, b, 0,
                                   s, a);
            });
    });
}

// The update with step 0, then steps 1 .. d: z_d ends in buffer d & 1.
void launch_update(const Workspace* w, PolyArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    const int d = w->degree;
    a.zout = z_of(w, 0);
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        with_columns(R, [&](auto r) {
            if (d > 0)
                hipLaunchKernelGGL((k_poly_update<decltype(r)::value, true>), g, b, 0, s, a, prologue);
            else
                hipLaunchKernelGGL((k_poly_update<decltype(r)::value, false>), g, b, 0, s, a, prologue);
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

void launch_finalize(const Workspace* w, const PolyArgs& a, int which, int store_total = 0)
{
    hipLaunchKernelGGL(k_poly_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, store_total);
}

// The preconditioned CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    hipStream_t s = w->v.stream;
    const PolyArgs a = make_args(w, nrhs, m);
    HIP_TRY(hipEventRecord(w->ev0, s));
    hipLaunchKernelGGL(k_poly_init, dim3((nrhs + 63) / 64), dim3(64), 0, s, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p, launch_spmm, launch_update, launch_finalize));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

// A caller's bounds: each finite and >= 0 (0.0: the default); both given, lmin < lmax.
int check_bounds(double lmin, double lmax)
{
    if (!(std::isfinite(lmin) && std::isfinite(lmax) && lmin >= 0.0 && lmax >= 0.0))
        return fail(HPCCG_HIP_EINVAL, "poly: spectrum bounds lmin %g, lmax %g (finite and >= 0 needed; 0: the default)",
                    lmin, lmax);
    if (lmax > 0.0 && lmin >= lmax)
        return fail(HPCCG_HIP_EINVAL, "poly: spectrum bounds lmin %g >= lmax %g", lmin, lmax);
    return 0;
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int degree, double lmin, double lmax, int max_iter, double tol, int* niters,
                 double* normr, double* times, bool host)
{
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "poly: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "poly: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "poly: max_iter %d is negative", max_iter);
    // (below every row count, so refused before the matrix is looked at)
    if (ldb < 0 || ldx < 0) return fail(HPCCG_HIP_EINVAL, "poly: leading dimensions %lld, %lld are negative", ldb, ldx);
    if (degree < 0 || degree > kPolyMaxDegree)
        return fail(HPCCG_HIP_EINVAL, "poly: degree %d (0 to %d)", degree, kPolyMaxDegree);
    TRY(check_bounds(lmin, lmax));
    MatrixView v;
    TRY(check_matrix(M, &v));
    if (ldb < v.n || ldx < v.n)
        return fail(HPCCG_HIP_EINVAL, "poly: leading dimensions %lld, %lld below the %d rows", ldb, ldx, v.n);
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
        TRY(ensure_cache(w));
        // the preconditioner first: a refused one leaves X as it is
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
                return fail(HPCCG_HIP_EINVAL, "poly: spectrum bounds lmin %g >= lmax %g", lmin, lmax);
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

int hpccg_hip_poly_abi_version(void) { return 1; }

int hpccg_hip_poly_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                long long ldx, const double* minv_dev, int degree, double lmin, double lmax,
                                int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance, niters,
                        normr, times, false);
}

int hpccg_hip_poly_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                         const double* minv, int degree, double lmin, double lmax, int max_iter, double tolerance,
                         int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B, ldb, X, ldx, minv, degree, lmin, lmax, max_iter, tolerance, niters, normr, times,
                        true);
}

int hpccg_hip_poly_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax)
{
    if (!M || !lmax) return fail(HPCCG_HIP_EINVAL, "poly: NULL argument");
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

int hpccg_hip_poly_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax)
{
    if (!M || !lmin || !lmax) return fail(HPCCG_HIP_EINVAL, "poly: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    if (!w || !w->solved) return fail(HPCCG_HIP_EINVAL, "poly: no spectrum (no polynomial solve ran on the matrix)");
    *lmin = w->last_lmin;
    *lmax = w->last_lmax;
    return 0;
}

int hpccg_hip_poly_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "poly: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "poly: no trace of column %d (the last polynomial solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

int hpccg_hip_poly_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "poly: NULL argument");
    g_ws<Workspace>.drop(M);
    return 0;
}

int hpccg_hip_poly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "poly: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    *bytes = w ? w->bytes + w->rest_bytes : 0;
    return 0;
}

int hpccg_hip_poly_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "poly: NULL argument");
    *count = g_ws<Workspace>.live();
    return 0;
}

}  // extern "C"
