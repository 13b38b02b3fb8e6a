// hpccg_srcg.hip -- single-reduction preconditioned CG (include/hpccg_hip_srcg.h,
// lib/libhpccg_hip_srcg.so): kernels and host code of the tenth library.
//
// The recurrence of hpccg_columns.h has two dependent reduction points per
// iteration (p.Ap for alpha, then r.r and r.z for beta): five launches. This
// unit runs the Chronopoulos-Gear form of the same preconditioned CG, with
// M^-1 = diag(m), by default Jacobi m_i = 1.0 / a_ii: one more recurrence
// vector (s = A p), every dot of an iteration formed together and completed by
// one finalize, three launches with one synchronisation point:
//   step      k_srcg_step<kR>: p = u + beta p, s = w + beta s, x += alpha p,
//             r -= alpha s, u = m r, + the r.u and r.r slice partials per column
//             (prologue: r = b - A t, u = m r)
//   SpMM      k_srcg_spmm_a<kW, kR, kWaves> | k_srcg_spmm_sell<kR>: the fp64 loops
//             of hpccg_spmm.h on u (w = A u, the u.w slice partial), kR = 1, 2, 4
//   finalize  k_srcg_finalize: one block per column; the three totals, then
//             alpha, beta, the history and the loop test once
//   prologue  k_srcg_t<kR>: t = x + 0 x, ahead of the prologue's first SpMM
//   diagonal  k_srcg_diag | k_srcg_check: hpccg_jacobi.h's bodies and cache
// The step and the finalize are hpccg_srcg_bodies.h; the column's state, the
// dot shapes, the workspace registry and the end of a recurrence are
// hpccg_columns.h. The launch loop is this unit's. No kernel here waits on
// another block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>

#include "../../include/hpccg_hip_srcg.h"
#include "hpccg_columns.h"
#include "hpccg_jacobi.h"
#include "hpccg_spmm.h"
#include "hpccg_srcg_bodies.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_srcg_init(SrcgArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// The prologue's t = x + 0.0*x, into u's buffer (col_p's prologue form; launched with no other).
template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_t(SrcgArgs a, bool prologue)
{
    col_p<kR, true>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_step(SrcgArgs a, bool prologue)
{
    srcg_step<kR>(a, prologue);
}

// The pcg library's plan choices (hpccg_pcg.hip): kWaves 5 for the 27-wide
// four-column form over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_srcg_spmm_a(SrcgArgs a,
                                                                                                    bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_spmm_sell(SrcgArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

__global__ __launch_bounds__(kFinThreads) void k_srcg_finalize(SrcgArgs a, int store_total)
{
    srcg_finalize(a, store_total);
}

// The diagonal of the image and the check of a caller's m: hpccg_jacobi.h's bodies.
__global__ __launch_bounds__(kBlock) void k_srcg_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_srcg_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct Workspace : TraceWorkspace, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;
    double *pd = nullptr, *sd = nullptr;  // p and s = A p (never zeroed again: k == 1 reads u and w)

    Workspace() { ndots = 3; }

    void free_own_vectors()
    {
        for (double* q : {r, x, b, pd, sd})
            if (q) (void)hipFree(q);
        r = x = b = pd = sd = nullptr;
    }
    void free_own_rest() { free_cache(); }
};

// What the library runs on: one rank, no halo.
int check_matrix(hpccg_hip_matrix* M, MatrixView* v)
{
    TRY(hpccg_hip_internal_view(M, v));
    if (v->in_group) return fail(HPCCG_HIP_EINVAL, "srcg: the matrix is a member of an in-process group (one rank only)");
    if (v->nranks > 1) return fail(HPCCG_HIP_EINVAL, "srcg: the matrix belongs to a communicator of %d ranks (one rank only)", v->nranks);
    if (v->ghost_lo || v->ghost_hi) return fail(HPCCG_HIP_EINVAL, "srcg: the matrix has halo rows (one rank only)");
    if (!v->has_a && !v->has_sell) return fail(HPCCG_HIP_EINVAL, "srcg: the matrix holds no device image");
    return 0;
}

// Jacobi: the cached 1.0 / a_ii, or the refusal of a matrix it does not exist for.
int ensure_jacobi(Workspace* w)
{
    int row = -1;
    TRY(build_jacobi(w, k_srcg_diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "srcg: Jacobi needs a finite diagonal > 0 in every row; row %d is the first whose diagonal is "
                    "missing, not finite or <= 0",
                    row);
    return 0;
}

// A call's own m: into the padded muser, every entry finite and > 0.
int stage_minv(Workspace* w, const double* minv, bool host)
{
    int row = -1;
    TRY(load_minv(w, minv, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, k_srcg_check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "srcg: minv[%d] is not finite and > 0 (the first such entry)", row);
    return 0;
}

// Room for ncols columns and a history of max_iter + 1 entries per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter)
{
    const size_t npad = (size_t)w->v.npad;
    const long long pcs = (long long)(npad + 2 * (size_t)w->v.guard_rows);  // a u column: [guard | rows (padded) | guard]
    return ensure_columns(w, ncols, max_iter, true, pcs, 0, [&](int cap) {
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        TRY(alloc_zero(w, &w->pd, npad * cap));
        TRY(alloc_zero(w, &w->sd, npad * cap));
        return 0;
    });
}

SrcgArgs make_args(const Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    SrcgArgs a{};
    fill_args(&a, w, nrhs);  // (Ap: w = A u)
    a.tri = 1;
    a.p = w->pbuf + v.guard_rows;  // u
    a.r = w->r;
    a.rcs = w->vcs;
    a.x = w->x;
    a.b = w->b;
    a.minv = m;
    a.aval = v.aval;
    a.vals = v.vals;
    a.pd = w->pd;
    a.sd = w->sd;
    return a;
}

#define HPCCG_SRCG_R(KERNEL, ...)                                                          \
    do {                                                                                   \
        if (R == 4)                                                                        \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 4>), g, b, 0, s, a, prologue);          \
        else if (R == 2)                                                                   \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 2>), g, b, 0, s, a, prologue);          \
        else                                                                               \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 1>), g, b, 0, s, a, prologue);          \
    } while (0)

// prologue: no u.w partial (the SpMM of t)
void launch_spmm(const Workspace* w, SrcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            HPCCG_SRCG_R(k_srcg_spmm_sell, );
        else if (a.a_width == 27 && R == 4 && a.nt)
            hipLaunchKernelGGL((k_srcg_spmm_a<27, 4, 5>), g, b, 0, s, a, prologue);
        else if (a.a_width == 27)
            HPCCG_SRCG_R(k_srcg_spmm_a, 27, );
        else if (a.a_width == 7)
            HPCCG_SRCG_R(k_srcg_spmm_a, 7, );
        else
            HPCCG_SRCG_R(k_srcg_spmm_a, 0, );
    });
}

void launch_t(const Workspace* w, SrcgArgs a)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    const bool prologue = true;  // (col_p's form)
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_SRCG_R(k_srcg_t, );
    });
}

void launch_step(const Workspace* w, SrcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_SRCG_R(k_srcg_step, );
    });
}
#undef HPCCG_SRCG_R

void launch_finalize(const Workspace* w, const SrcgArgs& a)
{
    hipLaunchKernelGGL(k_srcg_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, 0);
}

// One recurrence per column of the states on the device, on (b, x) of a: the
// prologue (t, A t, r and u, A u, the three totals), then iterations
// 1 .. kmax - 1 of step, SpMM, finalize, launched eagerly on the matrix's
// stream. Every kCheckEvery iterations the host reads the "columns ended" word
// and stops launching once every column has ended.
int run_iterations(Workspace* w, const SrcgArgs& a, int nrhs, int kmax)
{
    hipStream_t s = w->v.stream;
    launch_t(w, a);
    launch_spmm(w, a, true);
    launch_step(w, a, true);
    launch_spmm(w, a, false);
    launch_finalize(w, a);
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < kmax; k++) {
        launch_step(w, a, false);
        launch_spmm(w, a, false);
        launch_finalize(w, a);
        if (k % kCheckEvery == 0 && k + 1 < kmax) {
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(w->h_ended, w->ended, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (*w->h_ended >= nrhs) break;  // later launches would be no-ops for every column
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The single-reduction CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    hipStream_t s = w->v.stream;
    const SrcgArgs a = make_args(w, nrhs, m);
    HIP_TRY(hipEventRecord(w->ev0, s));
    hipLaunchKernelGGL(k_srcg_init, dim3((nrhs + 63) / 64), dim3(64), 0, s, a, max_iter, tol);
    TRY(run_iterations(w, a, nrhs, max_iter));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int max_iter, double tol, int* niters, double* normr, double* times, bool host)
{
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "srcg: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "srcg: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "srcg: max_iter %d is negative", max_iter);
    // (below every row count, so refused before the matrix is looked at)
    if (ldb < 0 || ldx < 0) return fail(HPCCG_HIP_EINVAL, "srcg: leading dimensions %lld, %lld are negative", ldb, ldx);
    MatrixView v;
    TRY(check_matrix(M, &v));
    if (ldb < v.n || ldx < v.n)
        return fail(HPCCG_HIP_EINVAL, "srcg: leading dimensions %lld, %lld below the %d rows", ldb, ldx, v.n);
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
        TRY(ensure_vectors(w, nrhs, max_iter));
        const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        const hipMemcpyKind out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        const auto t0 = std::chrono::steady_clock::now();
        TRY(copy_cols(w, w->b, w->vcs, B, ldb, nrhs, in));
        TRY(copy_cols(w, w->x, w->vcs, X, ldx, nrhs, in));
        if (host) HIP_TRY(hipStreamSynchronize(v.stream));
        const auto t1 = std::chrono::steady_clock::now();
        double wall = 0.0;
        TRY(run_cg(w, nrhs, minv ? w->muser : w->jac, max_iter, tol, niters, normr, &wall));
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

int hpccg_hip_srcg_abi_version(void) { return 1; }

int hpccg_hip_srcg_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                long long ldx, const double* minv_dev, int max_iter, double tolerance, int* niters,
                                double* normr, double* times)
{
    return solve_common(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, tolerance, niters, normr, times, false);
}

int hpccg_hip_srcg_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                         const double* minv, int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B, ldb, X, ldx, minv, max_iter, tolerance, niters, normr, times, true);
}

int hpccg_hip_srcg_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "srcg: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "srcg: no trace of column %d (the last single-reduction solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

int hpccg_hip_srcg_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "srcg: NULL argument");
    g_ws<Workspace>.drop(M);
    return 0;
}

int hpccg_hip_srcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "srcg: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    *bytes = w ? w->bytes + w->rest_bytes : 0;
    return 0;
}

int hpccg_hip_srcg_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "srcg: NULL argument");
    *count = g_ws<Workspace>.live();
    return 0;
}

}  // extern "C"
