// hpccg_pcg.hip -- diagonally preconditioned CG (include/hpccg_hip_pcg.h,
// lib/libhpccg_hip_pcg.so): kernels and host code of the fourth library.
//
// Every other solver here is the reference's unpreconditioned recurrence. On a
// badly row-scaled SPD matrix (Matrix.from_csr, read_HPC_row) that recurrence
// needs iterations a diagonal scaling makes unnecessary, so this unit runs the
// preconditioned one with M^-1 = diag(m), by default Jacobi m_i = 1.0 / a_ii:
//   z = m r (never stored), p = z + beta p, alpha = r.z / p.Ap, beta from r.z;
//   the history, the loop test and normr stay r.r's (the header has it all).
// It costs one 8-byte read of m per row in the p update and in the update
// kernel, shared by the kR columns of a launch, and one more slice partial per
// column in the update kernel; no further vector, launch or synchronisation.
//   SpMM      k_pcg_spmm_a<kW, kR, kWaves> | k_pcg_spmm_sell<kR>: the fp64 loops
//             of hpccg_spmm.h (the batch library's), kR = 1, 2, 4 columns
//   p update  k_pcg_p<kR>: p = x + 0 x (prologue) | p = m r + beta_c p
//   update    k_pcg_update<kR>: r = b - Ap (prologue) | x += alpha_c p,
//             r -= alpha_c Ap, + the r.z and r.r slice partials per column
//   finalize  k_pcg_finalize: one block per column; the r.r launch completes
//             both totals and advances the column once
//   diagonal  k_pcg_diag: a_ii from the matrix image (and 1.0 / a_ii with the
//             first row that has none) | k_pcg_check: a caller's m (the bodies
//             and the cache of both: hpccg_jacobi.h)
// The recurrence itself -- the column's state, those bodies (their kPre forms),
// the workspace registry and the launch loop -- is hpccg_columns.h. No kernel
// here waits on another block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/hpccg_hip_pcg.h"
#include "hpccg_columns.h"
#include "hpccg_jacobi.h"
#include "hpccg_spmm.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct PcgArgs : ColArgs {
    // (ColArgs' p: a guard zone around each column; minv: the call's m)
    int tri;  // width 27: slices whose offsets come in runs of three use the x-triple plan
    const double* aval;
    const double* vals;
};

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_pcg_init(PcgArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_pcg_p(PcgArgs a, bool prologue)
{
    col_p<kR, true>(a, prologue);
}

// The batch library's plan choices (hpccg_batch.hip): kWaves 5 for the 27-wide
// four-column form over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_pcg_spmm_a(PcgArgs a,
                                                                                                   bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_pcg_spmm_sell(PcgArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_pcg_update(PcgArgs a, bool prologue)
{
    col_update<kR, true>(a, prologue);
}

__global__ __launch_bounds__(kFinThreads) void k_pcg_finalize(PcgArgs a, int which, int store_total)
{
    col_finalize<true>(a, which, store_total);
}

// The diagonal of the image and the check of a caller's m: hpccg_jacobi.h's bodies.
__global__ __launch_bounds__(kBlock) void k_pcg_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_pcg_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct Workspace : TraceWorkspace, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;

    Workspace() { ndots = 3; }

    void free_own_vectors()
    {
        for (double* q : {r, x, b})
            if (q) (void)hipFree(q);
        r = x = b = nullptr;
    }
    void free_own_rest() { free_cache(); }
};

// What the library runs on: one rank, no halo.
int check_matrix(hpccg_hip_matrix* M, MatrixView* v)
{
    TRY(hpccg_hip_internal_view(M, v));
    if (v->in_group) return fail(HPCCG_HIP_EINVAL, "pcg: the matrix is a member of an in-process group (one rank only)");
    if (v->nranks > 1) return fail(HPCCG_HIP_EINVAL, "pcg: the matrix belongs to a communicator of %d ranks (one rank only)", v->nranks);
    if (v->ghost_lo || v->ghost_hi) return fail(HPCCG_HIP_EINVAL, "pcg: the matrix has halo rows (one rank only)");
    if (!v->has_a && !v->has_sell) return fail(HPCCG_HIP_EINVAL, "pcg: the matrix holds no device image");
    return 0;
}

// Jacobi: the cached 1.0 / a_ii, or the refusal of a matrix it does not exist for.
int ensure_jacobi(Workspace* w)
{
    int row = -1;
    TRY(build_jacobi(w, k_pcg_diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "pcg: Jacobi needs a finite diagonal > 0 in every row; row %d is the first whose diagonal is "
                    "missing, not finite or <= 0",
                    row);
    return 0;
}

// A call's own m: into the padded muser, every entry finite and > 0.
int stage_minv(Workspace* w, const double* minv, bool host)
{
    int row = -1;
    TRY(load_minv(w, minv, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, k_pcg_check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "pcg: minv[%d] is not finite and > 0 (the first such entry)", row);
    return 0;
}

// Room for ncols columns and a history of max_iter + 1 entries per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter)
{
    const size_t npad = (size_t)w->v.npad;
    const long long pcs = (long long)(npad + 2 * (size_t)w->v.guard_rows);  // a p column: [guard | rows (padded) | guard]
    return ensure_columns(w, ncols, max_iter, true, pcs, 0, [&](int cap) {
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        return 0;
    });
}

PcgArgs make_args(const Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    PcgArgs a{};
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
    return a;
}

#define HPCCG_PCG_R(KERNEL, ...)                                                           \
    do {                                                                                   \
        if (R == 4)                                                                        \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 4>), g, b, 0, s, a, prologue);          \
        else if (R == 2)                                                                   \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 2>), g, b, 0, s, a, prologue);          \
        else                                                                               \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 1>), g, b, 0, s, a, prologue);          \
    } while (0)

void launch_spmm(const Workspace* w, PcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            HPCCG_PCG_R(k_pcg_spmm_sell, );
        else if (a.a_width == 27 && R == 4 && a.nt)
            hipLaunchKernelGGL((k_pcg_spmm_a<27, 4, 5>), g, b, 0, s, a, prologue);
        else if (a.a_width == 27)
            HPCCG_PCG_R(k_pcg_spmm_a, 27, );
        else if (a.a_width == 7)
            HPCCG_PCG_R(k_pcg_spmm_a, 7, );
        else
            HPCCG_PCG_R(k_pcg_spmm_a, 0, );
    });
}

void launch_p(const Workspace* w, PcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_PCG_R(k_pcg_p, );
    });
}

void launch_update(const Workspace* w, PcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_PCG_R(k_pcg_update, );
    });
}
#undef HPCCG_PCG_R

void launch_finalize(const Workspace* w, const PcgArgs& a, int which, int store_total = 0)
{
    hipLaunchKernelGGL(k_pcg_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, store_total);
}

// The preconditioned CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    hipStream_t s = w->v.stream;
    const PcgArgs a = make_args(w, nrhs, m);
    HIP_TRY(hipEventRecord(w->ev0, s));
    hipLaunchKernelGGL(k_pcg_init, dim3((nrhs + 63) / 64), dim3(64), 0, s, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p, launch_spmm, launch_update, launch_finalize));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int max_iter, double tol, int* niters, double* normr, double* times, bool host)
{
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "pcg: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "pcg: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "pcg: max_iter %d is negative", max_iter);
    // (below every row count, so refused before the matrix is looked at)
    if (ldb < 0 || ldx < 0) return fail(HPCCG_HIP_EINVAL, "pcg: leading dimensions %lld, %lld are negative", ldb, ldx);
    MatrixView v;
    TRY(check_matrix(M, &v));
    if (ldb < v.n || ldx < v.n)
        return fail(HPCCG_HIP_EINVAL, "pcg: leading dimensions %lld, %lld below the %d rows", ldb, ldx, v.n);
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

int hpccg_hip_pcg_abi_version(void) { return 1; }

int hpccg_hip_pcg_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                               long long ldx, const double* minv_dev, int max_iter, double tolerance, int* niters,
                               double* normr, double* times)
{
    return solve_common(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, tolerance, niters, normr, times, false);
}

int hpccg_hip_pcg_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                        const double* minv, int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B, ldb, X, ldx, minv, max_iter, tolerance, niters, normr, times, true);
}

int hpccg_hip_pcg_diagonal(hpccg_hip_matrix* M, double* d_dev)
{
    if (!M || !d_dev) return fail(HPCCG_HIP_EINVAL, "pcg: NULL argument");
    MatrixView v;
    TRY(check_matrix(M, &v));
    if (v.n == 0) return 0;
    return keep_device([&]() -> int {
        HIP_TRY(hipSetDevice(v.device));
        hipLaunchKernelGGL(k_pcg_diag, dim3(v.nslices), dim3(kBlock), 0, v.stream, diag_args(v), d_dev,
                           (double*)nullptr, (int*)nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(v.stream));
        return 0;
    });
}

int hpccg_hip_pcg_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "pcg: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "pcg: no trace of column %d (the last preconditioned solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

int hpccg_hip_pcg_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "pcg: NULL argument");
    g_ws<Workspace>.drop(M);
    return 0;
}

int hpccg_hip_pcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "pcg: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    *bytes = w ? w->bytes + w->rest_bytes : 0;
    return 0;
}

int hpccg_hip_pcg_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "pcg: NULL argument");
    *count = g_ws<Workspace>.live();
    return 0;
}

}  // extern "C"
