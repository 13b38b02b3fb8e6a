// hpccg_poly_host.h -- the host code of the Chebyshev polynomial preconditioned
// CG, shared by the polynomial units (hpccg_poly.hip, hpccg_poly32.hip and,
// under hpccg_poly_group_host.h, hpccg_poly_group.hip and
// hpccg_poly32_group.hip): the workspace's polynomial state, the dispatch on a
// chunk's columns and fp64 SpMM form, the kernel arguments, the launchers, the
// checks of a caller's bounds and the interval with its coefficients; for the
// one-rank units (poly, poly32) also the matrix check, the preconditioner, the
// Gershgorin bound, the solve and the bodies of their extern "C" functions.
// A unit hands over one traits struct U:
//   Args, Workspace       its kernel arguments (a PolyArgs) and its workspace (a
//                         PolyWorkspace)
//   row0(w)               local row 0 inside a guarded column: the guard rows
//                         (one rank) or the member's p0 (group)
//   init, p<kR, kPre>, update<kR, kCheb>, finalize, spmm_a<kW, kR, kWaves>,
//   spmm_sell<kR>         its kernels, as (templates of) kernel pointers; with
//   step<kW, kR, kWaves>, step_sell<kR> where it runs the fp64 steps
// and a one-rank unit further
//   who, solve_name       the name in front of its messages ("poly") and in
//                         "the last <solve_name> solve"
//   diag, check, q, bound, bound_top   the preconditioner's and the bound's kernels
//   launch_spmm(w, a, prologue), launch_step(w, a)   where poly32 differs: the
//                         SpMM and one step over the chunks of columns
// The __global__ entry points and the extern "C" definitions stay in the units.
// The launchers are plain functions and the launch loops take them as function
// pointers (hpccg_columns.h, hpccg_group.h); nothing here allocates per launch.
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <type_traits>

#include "hpccg_columns.h"
#include "hpccg_jacobi.h"
#include "hpccg_poly_bodies.h"
#include "hpccg_poly_coeffs.h"
#include "hpccg_spmm.h"

namespace hpccg {

namespace {

// A polynomial unit's workspace (a group member's adds GroupMember).
struct PolyWorkspace : TraceWorkspace, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;
    double *dd = nullptr, *zbuf = nullptr;  // zbuf: two sets of cap columns in p's (guarded) layout
    // the bound's vectors (kept while the columns grow, counted in rest_bytes);
    // qbuf: one guarded column
    double *qbuf = nullptr, *smax = nullptr, *lmax_dev = nullptr;
    bool jac_lmax_built = false;
    double jac_lmax = 0.0;  // the bound with m = 1 / a_ii (a member: its rows' part)
    // the call being run
    int degree = 0;
    double cheb0 = 0.0, aj[kPolyMaxDegree + 1] = {}, bj[kPolyMaxDegree + 1] = {};
    bool solved = false;  // (a group: member 0)
    double last_lmin = 0.0, last_lmax = 0.0;

    PolyWorkspace() { ndots = 3; }

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
    long long total_bytes() const { return bytes + rest_bytes; }
};

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

// The fp64 SpMM forms of a chunk (the pcg library's plan choices): f(width, kR,
// kWaves), kWaves 5 for the 27-wide four-column form over images streamed from
// HBM, else 4.
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

// z buffer `which` (0, 1): local row 0 of column 0
template <class U>
double* z_of(const typename U::Workspace* w, int which)
{
    return w->zbuf + (size_t)which * (size_t)w->pcs * (size_t)w->cap + U::row0(w);
}

// (what a unit's Args add to PolyArgs is set where its launchers use it)
template <class U>
typename U::Args make_args(const typename U::Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    typename U::Args a{};
    fill_args(&a, w, nrhs);
    a.tri = 1;
    a.p = w->pbuf + U::row0(w);
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

template <class U>
void launch_init(const typename U::Workspace* w, const typename U::Args& a, int max_iter, double tol)
{
    hipLaunchKernelGGL(U::init, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, max_iter, tol);
}

// d == 0: z = m r in the register; else the last step's z (buffer d & 1, the
// unit's own rows only) in r's place.
template <class U>
void launch_p(const typename U::Workspace* w, typename U::Args a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    const int d = w->degree;
    if (d > 0) {
        a.r = z_of<U>(w, d & 1);
        a.rcs = a.pcs;
    }
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        with_columns(R, [&](auto r) {
            if (d > 0)
                hipLaunchKernelGGL((U::template p<decltype(r)::value, false>), g, b, 0, s, a, prologue);
            else
                hipLaunchKernelGGL((U::template p<decltype(r)::value, true>), g, b, 0, s, a, prologue);
        });
    });
}

// Ap = A p from the fp64 image.
template <class U>
void launch_spmm64(const typename U::Workspace* w, typename U::Args a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            with_columns(R, [&](auto r) {
                hipLaunchKernelGGL((U::template spmm_sell<decltype(r)::value>), g, b, 0, s, a, prologue);
            });
        else
            with_spmm_form(a, R, [&](auto wd, auto r, auto wv) {
                hipLaunchKernelGGL((U::template spmm_a<decltype(wd)::value, decltype(r)::value, decltype(wv)::value>),
                                   g, b, 0, s, a, prologue);
            });
    });
}

// The update with step 0 into z buffer 0 where d >= 1 (d == 0: the engine's kPre update).
template <class U>
void launch_update0(const typename U::Workspace* w, typename U::Args a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    const int d = w->degree;
    a.zout = z_of<U>(w, 0);
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        with_columns(R, [&](auto r) {
            if (d > 0)
                hipLaunchKernelGGL((U::template update<decltype(r)::value, true>), g, b, 0, s, a, prologue);
            else
                hipLaunchKernelGGL((U::template update<decltype(r)::value, false>), g, b, 0, s, a, prologue);
        });
    });
}

// Step j's buffers and scalars: it reads z buffer (j - 1) & 1 and stores buffer j & 1.
template <class U>
typename U::Args step_args(const typename U::Workspace* w, typename U::Args a, int j)
{
    a.zin = z_of<U>(w, (j - 1) & 1);
    a.zout = z_of<U>(w, j & 1);
    a.aj = w->aj[j];
    a.bj = w->bj[j];
    a.last = j == w->degree;
    return a;
}

// One step's launches from the fp64 image: the SpMM's forms.
template <class U>
void launch_step64(const typename U::Workspace* w, typename U::Args a)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            with_columns(R, [&](auto r) {
                hipLaunchKernelGGL((U::template step_sell<decltype(r)::value>), g, b, 0, s, a);
            });
        else
            with_spmm_form(a, R, [&](auto wd, auto r, auto wv) {
                hipLaunchKernelGGL((U::template step<decltype(wd)::value, decltype(r)::value, decltype(wv)::value>), g,
                                   b, 0, s, a);
            });
    });
}

template <class U>
void launch_finalize(const typename U::Workspace* w, const typename U::Args& a, int which, int store_total)
{
    hipLaunchKernelGGL(U::finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, store_total);
}

// A caller's bounds: each finite and >= 0 (0.0: the default); both given, lmin < lmax.
int check_bounds(const char* who, double lmin, double lmax)
{
    if (!(std::isfinite(lmin) && std::isfinite(lmax) && lmin >= 0.0 && lmax >= 0.0))
        return fail(HPCCG_HIP_EINVAL, "%s: spectrum bounds lmin %g, lmax %g (finite and >= 0 needed; 0: the default)",
                    who, lmin, lmax);
    if (lmax > 0.0 && lmin >= lmax)
        return fail(HPCCG_HIP_EINVAL, "%s: spectrum bounds lmin %g >= lmax %g", who, lmin, lmax);
    return 0;
}

// The interval of a call and the polynomial's coefficients on it. *lmax == 0.0:
// bound(lmax), the unit's Gershgorin bound; *lmin == 0.0: lmax / kPolyEigRatio.
// Degree 0 applies no polynomial and needs no interval (what the caller gave is
// kept for last_spectrum).
template <class Bound>
int resolve_interval(const char* who, int degree, double* lmin, double* lmax, double* cheb0, double* aj, double* bj,
                     Bound bound)
{
    if (degree > 0) {
        if (*lmax == 0.0) TRY(bound(lmax));
        if (*lmin == 0.0) *lmin = *lmax / kPolyEigRatio;
        if (!(*lmin > 0.0 && *lmin < *lmax))
            return fail(HPCCG_HIP_EINVAL, "%s: spectrum bounds lmin %g >= lmax %g", who, *lmin, *lmax);
        poly_coefficients(*lmin, *lmax, degree, cheb0, aj, bj);
    } else if (*lmin == 0.0 && *lmax > 0.0) {
        *lmin = *lmax / kPolyEigRatio;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// The one-rank units (poly, poly32)
// ---------------------------------------------------------------------------
inline long long p_column(const MatrixView& v)
{
    return (long long)v.npad + 2 * v.guard_rows;  // [guard | rows (padded) | guard]
}

// What a one-rank unit runs on: one rank, no halo.
inline int check_matrix(const char* who, hpccg_hip_matrix* M, MatrixView* v)
{
    TRY(hpccg_hip_internal_view(M, v));
    if (v->in_group)
        return fail(HPCCG_HIP_EINVAL, "%s: the matrix is a member of an in-process group (one rank only)", who);
    if (v->nranks > 1)
        return fail(HPCCG_HIP_EINVAL, "%s: the matrix belongs to a communicator of %d ranks (one rank only)", who,
                    v->nranks);
    if (v->ghost_lo || v->ghost_hi) return fail(HPCCG_HIP_EINVAL, "%s: the matrix has halo rows (one rank only)", who);
    if (!v->has_a && !v->has_sell) return fail(HPCCG_HIP_EINVAL, "%s: the matrix holds no device image", who);
    return 0;
}

// Jacobi: the cached 1.0 / a_ii, or the refusal of a matrix it does not exist for.
template <class U>
int ensure_jacobi(typename U::Workspace* w)
{
    int row = -1;
    TRY(build_jacobi(w, U::diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "%s: Jacobi needs a finite diagonal > 0 in every row; row %d is the first whose diagonal is "
                    "missing, not finite or <= 0",
                    U::who, row);
    return 0;
}

// A call's own m: into the padded muser, every entry finite and > 0.
template <class U>
int stage_minv(typename U::Workspace* w, const double* minv, bool host)
{
    int row = -1;
    TRY(load_minv(w, minv, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, U::check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "%s: minv[%d] is not finite and > 0 (the first such entry)", U::who, row);
    return 0;
}

// The bound's vectors (zeroed: q's guard zones and its rows past n are read and
// never stored; a member's ghost planes by the halo only). pcs: the guarded column.
int ensure_bound_vectors(PolyWorkspace* w, long long pcs)
{
    if (w->qbuf) return 0;
    HIP_TRY(hipSetDevice(w->v.device));
    const long long before = w->bytes;  // (alloc_zero counts into bytes: the columns')
    int rc = alloc_zero(w, &w->qbuf, (size_t)pcs);
    if (!rc) rc = alloc_zero(w, &w->smax, (size_t)std::max(w->v.nslices, 1));
    if (!rc) rc = alloc_zero(w, &w->lmax_dev, 1);
    if (rc)
        w->free_bound_vectors();
    else
        w->rest_bytes += w->bytes - before;
    w->bytes = before;
    return rc;
}

// The symmetric Gershgorin bound with the padded device vector m (always over
// the fp64 image).
template <class U>
int compute_bound(typename U::Workspace* w, const double* m, double* lmax)
{
    const MatrixView& v = w->v;
    hipStream_t s = v.stream;
    TRY(ensure_bound_vectors(w, p_column(v)));
    double* q = w->qbuf + v.guard_rows;
    hipLaunchKernelGGL(U::q, dim3((v.n + 255) / 256), dim3(256), 0, s, m, v.n, q);
    hipLaunchKernelGGL(U::bound, dim3(v.nslices), dim3(kBlock), 0, s, diag_args(v), (const double*)q, w->smax);
    hipLaunchKernelGGL(U::bound_top, dim3(1), dim3(kBlock), 0, s, (const double*)w->smax, v.nslices, w->lmax_dev);
    HIP_TRY(hipGetLastError());
    double h = 0.0;
    HIP_TRY(hipMemcpyAsync(&h, w->lmax_dev, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!(h > 0.0 && std::isfinite(h)))
        return fail(HPCCG_HIP_EINVAL, "%s: the Gershgorin bound of the matrix is %g (finite and > 0 needed)", U::who, h);
    *lmax = h;
    return 0;
}

// Jacobi's bound: cached with 1 / a_ii.
template <class U>
int jacobi_bound(typename U::Workspace* w, double* lmax)
{
    if (!w->jac_lmax_built) {
        TRY(compute_bound<U>(w, w->jac, &w->jac_lmax));
        w->jac_lmax_built = true;
    }
    *lmax = w->jac_lmax;
    return 0;
}

// Room for ncols columns of the guarded width pcs and a history of max_iter + 1
// entries per column; ntot: totals per column (a group member's).
int ensure_vectors(PolyWorkspace* w, int ncols, int max_iter, long long pcs, int ntot)
{
    const size_t npad = (size_t)w->v.npad;
    return ensure_columns(w, ncols, max_iter, true, pcs, ntot, [&](int cap) {
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        TRY(alloc_zero(w, &w->dd, npad * cap));
        // zeroed: z's guard zones and the rows past n are read and never stored
        // (a member's ghost planes by the halo only)
        TRY(alloc_zero(w, &w->zbuf, 2 * (size_t)pcs * cap));
        return 0;
    });
}

// The update with step 0, then steps 1 .. d: z_d ends in buffer d & 1.
template <class U>
void launch_update(const typename U::Workspace* w, typename U::Args a, bool prologue)
{
    launch_update0<U>(w, a, prologue);
    for (int j = 1; j <= w->degree; j++) U::launch_step(w, step_args<U>(w, a, j));
}

// The preconditioned CG on the columns staged in the workspace's b and x.
template <class U>
int run_cg(typename U::Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr,
           double* wall)
{
    const typename U::Args a = make_args<U>(w, nrhs, m);
    HIP_TRY(hipEventRecord(w->ev0, w->v.stream));
    launch_init<U>(w, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p<U>, U::launch_spmm, launch_update<U>, launch_finalize<U>));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

// prepare (may be null): what the unit builds per matrix before the
// preconditioner (poly32: the fp32 image, whose verdict comes first).
template <class U>
int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int degree, double lmin, double lmax, int max_iter, double tol, int* niters,
                 double* normr, double* times, bool host, int (*prepare)(typename U::Workspace*) = nullptr)
{
    using W = typename U::Workspace;
    const char* who = U::who;
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", who);
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "%s: nrhs %d (at least 1)", who, nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "%s: max_iter %d is negative", who, max_iter);
    // (below every row count, so refused before the matrix is looked at)
    if (ldb < 0 || ldx < 0)
        return fail(HPCCG_HIP_EINVAL, "%s: leading dimensions %lld, %lld are negative", who, ldb, ldx);
    if (degree < 0 || degree > kPolyMaxDegree)
        return fail(HPCCG_HIP_EINVAL, "%s: degree %d (0 to %d)", who, degree, kPolyMaxDegree);
    TRY(check_bounds(who, lmin, lmax));
    MatrixView v;
    TRY(check_matrix(who, M, &v));
    if (ldb < v.n || ldx < v.n)
        return fail(HPCCG_HIP_EINVAL, "%s: leading dimensions %lld, %lld below the %d rows", who, ldb, ldx, v.n);
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
        W* w = nullptr;
        TRY(g_ws<W>.record(M, v, &w));
        // the unit's own first, then the preconditioner: a refused call leaves X as it is
        if (prepare) TRY(prepare(w));
        TRY(ensure_cache(w));
        if (minv)
            TRY(stage_minv<U>(w, minv, host));
        else
            TRY(ensure_jacobi<U>(w));
        const double* m = minv ? w->muser : w->jac;
        TRY(resolve_interval(who, degree, &lmin, &lmax, &w->cheb0, w->aj, w->bj, [&](double* top) {
            return minv ? compute_bound<U>(w, m, top) : jacobi_bound<U>(w, top);
        }));
        TRY(ensure_vectors(w, nrhs, max_iter, p_column(v), 0));
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
        TRY(run_cg<U>(w, nrhs, m, max_iter, tol, niters, normr, &wall));
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

// The bodies of a one-rank unit's extern "C" functions beside the solves.
template <class U>
int poly_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax)
{
    using W = typename U::Workspace;
    if (!M || !lmax) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    MatrixView v;
    TRY(check_matrix(U::who, M, &v));
    if (v.n == 0) {
        *lmax = 0.0;
        return 0;
    }
    return keep_device([&]() -> int {
        W* w = nullptr;
        TRY(g_ws<W>.record(M, v, &w));
        TRY(ensure_cache(w));
        if (minv_dev) {
            TRY(stage_minv<U>(w, minv_dev, false));
            return compute_bound<U>(w, w->muser, lmax);
        }
        TRY(ensure_jacobi<U>(w));
        return jacobi_bound<U>(w, lmax);
    });
}

template <class U>
int poly_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax)
{
    if (!M || !lmin || !lmax) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(M);
    if (!w || !w->solved)
        return fail(HPCCG_HIP_EINVAL, "%s: no spectrum (no %s solve ran on the matrix)", U::who, U::solve_name);
    *lmin = w->last_lmin;
    *lmax = w->last_lmax;
    return 0;
}

template <class U>
int poly_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(M);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "%s: no trace of column %d (the last %s solve had %d)", U::who, col,
                    U::solve_name, w ? (int)w->trace.size() : 0);
    return n;
}

template <class U>
int poly_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    g_ws<typename U::Workspace>.drop(M);
    return 0;
}

template <class U>
int poly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(M);
    *bytes = w ? w->total_bytes() : 0;
    return 0;
}

template <class U>
int poly_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    *count = g_ws<typename U::Workspace>.live();
    return 0;
}

}  // namespace

}  // namespace hpccg
