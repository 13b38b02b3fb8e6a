// hpccg_onerank_host.h -- the host code that the units solving on one rank
// share (hpccg_pcg.hip, hpccg_srcg.hip and, through hpccg_poly_host.h,
// hpccg_poly.hip, hpccg_poly32.hip and hpccg_srpoly.hip; the single-reduction
// launch loop over it is hpccg_srcg_host.h): the dispatch of a launch on a chunk's
// columns and fp64 SpMM form, the matrix check, the diagonal preconditioner
// with its refusals, the solve (argument checks, the empty matrix, staging B
// and X, the two `times` slots) and the bodies of the bookkeeping exports.
// The group units take the dispatch and the bookkeeping bodies through
// hpccg_group_host.h (hpccg_pcg_group.hip, hpccg_srcg_group.hip; hpccg_poly_group.hip
// and hpccg_poly32_group.hip under hpccg_poly_group_host.h); hpccg_batch.hip and hpccg_mixed.hip, whose launchers
// and solves are their own, take the matrix check and the bookkeeping bodies.
// A unit hands over one traits struct U with what it uses of
//   Args, Workspace       its kernel arguments (a ColArgs) and its workspace (a
//                         ColWorkspace with total_bytes())
//   who, solve_name       the name in front of its messages ("pcg") and in
//                         "the last <solve_name> solve"
//   init, finalize, spmm_a<kW, kR, kWaves>, spmm_sell<kR>, diag, check
//                         its kernels, as (templates of) kernel pointers
// The __global__ entry points and the extern "C" definitions stay in the units.
// The launchers are plain functions and the launch loops take them as function
// pointers (hpccg_columns.h, hpccg_group.h); nothing here allocates per launch.
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include <algorithm>
#include <chrono>
#include <type_traits>

#include "hpccg_columns.h"
#include "hpccg_jacobi.h"
#include "hpccg_spmm.h"

namespace hpccg {

namespace {

// ---------------------------------------------------------------------------
// The dispatch of a launch on a chunk of columns
// ---------------------------------------------------------------------------
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
void with_spmm_form(const ColArgs& a, int R, F f)
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

// One kernel per chunk of columns: kernel_of(std::integral_constant<int, kR>)
// is the unit's (Args, bool prologue) kernel for kR columns. Only what
// kernel_of names is instantiated.
template <class W, class A, class K>
void launch_chunks(const W* w, A a, bool prologue, K kernel_of)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        with_columns(R, [&](auto r) { hipLaunchKernelGGL(kernel_of(r), g, b, 0, s, a, prologue); });
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

template <class U>
void launch_init(const typename U::Workspace* w, const typename U::Args& a, int max_iter, double tol)
{
    hipLaunchKernelGGL(U::init, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, max_iter, tol);
}

template <class U>
void launch_finalize(const typename U::Workspace* w, const typename U::Args& a, int which, int store_total)
{
    hipLaunchKernelGGL(U::finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, store_total);
}

// ---------------------------------------------------------------------------
// The matrix of a one-rank unit and its diagonal preconditioner
// ---------------------------------------------------------------------------
inline long long p_column(const MatrixView& v)
{
    return (long long)v.npad + 2 * v.guard_rows;  // [guard | rows (padded) | guard]
}

// What a one-rank unit runs on: one rank, no halo (group1: also the one member
// of a one-rank in-process group, which is that).
inline int check_matrix(const char* who, hpccg_hip_matrix* M, MatrixView* v, bool group1 = false)
{
    TRY(hpccg_hip_internal_view(M, v));
    if (v->in_group && !(group1 && v->nranks == 1))
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

// ---------------------------------------------------------------------------
// A solve of nrhs columns with M^-1 = diag(m), m a call's minv or Jacobi's.
//   own_checks()            the unit's own argument checks, after the shared
//                           ones that need no matrix and before the matrix's
//   prepare(w)              (may be null) what the unit builds per matrix
//                           before the preconditioner (poly32: the fp32 image,
//                           whose verdict comes first)
//   setup(w, m, max_iter)   the unit's per-call state and its vectors, with
//                           the padded device m in hand
//   run_cg(w, nrhs, m, max_iter, tol, niters, normr, wall)   the recurrence on
//                           the columns staged in the workspace's b and x
// ---------------------------------------------------------------------------
template <class U, class Checks, class Setup>
int solve_onerank(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                  const double* minv, int max_iter, double tol, int* niters, double* normr, double* times, bool host,
                  Checks own_checks, int (*prepare)(typename U::Workspace*), Setup setup,
                  int (*run_cg)(typename U::Workspace*, int, const double*, int, double, int*, double*, double*))
{
    using W = typename U::Workspace;
    const char* who = U::who;
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", who);
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "%s: nrhs %d (at least 1)", who, nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "%s: max_iter %d is negative", who, max_iter);
    // (below every row count, so refused before the matrix is looked at)
    if (ldb < 0 || ldx < 0)
        return fail(HPCCG_HIP_EINVAL, "%s: leading dimensions %lld, %lld are negative", who, ldb, ldx);
    TRY(own_checks());
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
        TRY(setup(w, m, max_iter));
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

// ---------------------------------------------------------------------------
// The bodies of a unit's bookkeeping exports
// ---------------------------------------------------------------------------
template <class U>
int unit_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
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
int unit_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    g_ws<typename U::Workspace>.drop(M);
    return 0;
}

template <class U>
int unit_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(M);
    *bytes = w ? w->total_bytes() : 0;
    return 0;
}

template <class U>
int unit_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    *count = g_ws<typename U::Workspace>.live();
    return 0;
}

}  // namespace

}  // namespace hpccg
