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
// hpccg_columns.h. The launch loop, its frame, the launchers and p and s are
// hpccg_srcg_host.h, shared with hpccg_srpoly.hip; the host code around them --
// the launch dispatch, the checks, the preconditioner, the solve, the
// bookkeeping exports -- is hpccg_onerank_host.h, shared with hpccg_pcg.hip and
// the polynomial units. This unit keeps its kernel arguments. No kernel here
// waits on another block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_srcg.h"
#include "hpccg_srcg_host.h"

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
// host: hpccg_srcg_host.h and hpccg_onerank_host.h over this unit's kernels
// ---------------------------------------------------------------------------
struct Workspace : TraceWorkspace, JacobiCache, SrcgColumns {
    double *r = nullptr, *x = nullptr, *b = nullptr;

    Workspace() { ndots = 3; }

    void free_own_vectors()
    {
        for (double* q : {r, x, b})
            if (q) (void)hipFree(q);
        r = x = b = nullptr;
        free_ps();
    }
    void free_own_rest() { free_cache(); }
    long long total_bytes() const { return bytes + rest_bytes; }
};

// Room for ncols columns (u's are guarded, as a p column) and a history of
// max_iter + 1 entries per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter)
{
    const size_t npad = (size_t)w->v.npad;
    return ensure_columns(w, ncols, max_iter, true, p_column(w->v), 0, [&](int cap) {
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        return alloc_ps(w, npad * cap);
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

struct Srcg {
    using Args = SrcgArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "srcg";
    static constexpr const char* solve_name = "single-reduction";

    static constexpr auto init = k_srcg_init;
    template <int kR>
    static constexpr auto t = k_srcg_t<kR>;
    template <int kR>
    static auto fused_step(const Workspace*)
    {
        return k_srcg_step<kR>;
    }
    // (prologue: no u.w partial, the SpMM of t)
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_srcg_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_srcg_spmm_sell<kR>;
    static constexpr auto finalize = k_srcg_finalize;
    static constexpr auto diag = k_srcg_diag;
    static constexpr auto check = k_srcg_check;
};

// The single-reduction CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    return run_srcg<Srcg>(w, make_args(w, nrhs, m), nrhs, max_iter, tol, niters, normr, wall, launch_srcg_step<Srcg>,
                          launch_spmm64<Srcg>);
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int max_iter, double tol, int* niters, double* normr, double* times, bool host)
{
    return solve_onerank<Srcg>(
        M, nrhs, B, ldb, X, ldx, minv, max_iter, tol, niters, normr, times, host, [] { return 0; }, nullptr,
        [&](Workspace* w, const double*, int kmax) { return ensure_vectors(w, nrhs, kmax); }, run_cg);
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
    return unit_last_trace<Srcg>(M, col, out, cap);
}

int hpccg_hip_srcg_release(hpccg_hip_matrix* M) { return unit_release<Srcg>(M); }

int hpccg_hip_srcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Srcg>(M, bytes);
}

int hpccg_hip_srcg_live_workspaces(int* count) { return unit_live_workspaces<Srcg>(count); }

}  // extern "C"
