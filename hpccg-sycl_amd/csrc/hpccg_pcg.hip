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
// the workspace registry and the launch loop -- is hpccg_columns.h. The host
// code around it -- the launch dispatch, the checks, the preconditioner, the
// solve, the bookkeeping exports -- is hpccg_onerank_host.h, shared with
// hpccg_srcg.hip and the polynomial units; this unit hands it its kernels. No
// kernel here waits on another block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_pcg.h"
#include "hpccg_onerank_host.h"

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
// host: hpccg_onerank_host.h over this unit's kernels
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
    long long total_bytes() const { return bytes + rest_bytes; }
};

// Room for ncols columns and a history of max_iter + 1 entries per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter)
{
    const size_t npad = (size_t)w->v.npad;
    return ensure_columns(w, ncols, max_iter, true, p_column(w->v), 0, [&](int cap) {
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

struct Pcg {
    using Args = PcgArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "pcg";
    static constexpr const char* solve_name = "preconditioned";

    static constexpr auto init = k_pcg_init;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_pcg_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_pcg_spmm_sell<kR>;
    static constexpr auto finalize = k_pcg_finalize;
    static constexpr auto diag = k_pcg_diag;
    static constexpr auto check = k_pcg_check;
};

void launch_p(const Workspace* w, PcgArgs a, bool prologue)
{
    launch_chunks(w, a, prologue, [](auto r) { return k_pcg_p<decltype(r)::value>; });
}

void launch_update(const Workspace* w, PcgArgs a, bool prologue)
{
    launch_chunks(w, a, prologue, [](auto r) { return k_pcg_update<decltype(r)::value>; });
}

// The preconditioned CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    const PcgArgs a = make_args(w, nrhs, m);
    HIP_TRY(hipEventRecord(w->ev0, w->v.stream));
    launch_init<Pcg>(w, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p, launch_spmm64<Pcg>, launch_update, launch_finalize<Pcg>));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int max_iter, double tol, int* niters, double* normr, double* times, bool host)
{
    return solve_onerank<Pcg>(
        M, nrhs, B, ldb, X, ldx, minv, max_iter, tol, niters, normr, times, host, [] { return 0; }, nullptr,
        [&](Workspace* w, const double*, int kmax) { return ensure_vectors(w, nrhs, kmax); }, run_cg);
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
    TRY(check_matrix(Pcg::who, M, &v));
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
    return unit_last_trace<Pcg>(M, col, out, cap);
}

int hpccg_hip_pcg_release(hpccg_hip_matrix* M) { return unit_release<Pcg>(M); }

int hpccg_hip_pcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Pcg>(M, bytes);
}

int hpccg_hip_pcg_live_workspaces(int* count) { return unit_live_workspaces<Pcg>(count); }

}  // extern "C"
