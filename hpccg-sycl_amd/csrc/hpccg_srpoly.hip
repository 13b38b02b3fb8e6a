// hpccg_srpoly.hip -- single-reduction CG with the Chebyshev polynomial
// preconditioner (include/hpccg_hip_srpoly.h, lib/libhpccg_hip_srpoly.so):
// kernels and host code of the twelfth library.
//
// hpccg_poly.hip buys iterations with polynomial steps that need no dot, and
// still completes two dots per outer iteration (p.Ap, then r.r with r.z);
// hpccg_srcg.hip completes all of an iteration's dots at one point, with
// M^-1 = diag(m) only. This unit runs the Chronopoulos-Gear recurrence of the
// latter with u = P(r) of the former: 3 + d launches per iteration and chunk of
// columns, with one synchronisation point:
//   step      k_srpoly_step<kR, true>: p = u + beta p, s = w + beta s,
//             x += alpha p, r -= alpha s, then step 0 of P on the new r (dd and
//             z buffer 0) and the r.r slice partial (prologue: r = b - A t, step
//             0) | <kR, false>, degree 0: hpccg_srcg_bodies.h's step, u = m r
//   steps     k_srpoly_cheb<kW, kR, kWaves> | k_srpoly_cheb_sell<kR>, j = 1..d:
//             hpccg_poly.hip's step forms; the last forms the r.u slice partial
//   SpMM      k_srpoly_spmm_a<kW, kR, kWaves> | k_srpoly_spmm_sell<kR>: the fp64
//             loops of hpccg_spmm.h on u = z_d (buffer d & 1): w = A u, the u.w
//             slice partial
//   finalize  k_srpoly_finalize: hpccg_srcg_bodies.h's; the three totals, then
//             alpha, beta, the history and the loop test once
//   prologue  k_srpoly_t<kR>: t = x + 0 x into the guarded p buffer (which
//             holds u at degree 0), ahead of the prologue's first SpMM
//   bound     k_srpoly_q, k_srpoly_bound, k_srpoly_bound_top
//   diagonal  k_srpoly_diag | k_srpoly_check (hpccg_jacobi.h's bodies)
// The fused step is hpccg_srpoly_bodies.h; the steps' ends and the bound are
// hpccg_poly_bodies.h; the finalize is hpccg_srcg_bodies.h. The host code is
// hpccg_poly_host.h (the workspace's polynomial state, the step launchers, the
// bound, the interval) over hpccg_onerank_host.h (the dispatch, the checks, the
// preconditioner, the solve, the bookkeeping exports); the launch loop, its
// frame, the launchers of t, the fused step and the finalize, and p and s are
// hpccg_srcg_host.h, shared with hpccg_srcg.hip. This unit keeps its kernel
// arguments, the d steps after the fused one and the SpMM of u. No kernel here
// waits on another block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_srpoly.h"
#include "hpccg_poly_host.h"
#include "hpccg_srcg_host.h"
#include "hpccg_srpoly_bodies.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_srpoly_init(SrpolyArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// The prologue's t = x + 0.0*x, into p's buffer (col_p's prologue form; launched with no other).
template <int kR>
__global__ __launch_bounds__(kBlock) void k_srpoly_t(SrpolyArgs a, bool prologue)
{
    col_p<kR, true>(a, prologue);
}

// kCheb: hpccg_srpoly_bodies.h's step with step 0 in r's pass; else (degree 0) hpccg_srcg_bodies.h's.
template <int kR, bool kCheb>
__global__ __launch_bounds__(kBlock) void k_srpoly_step(SrpolyArgs a, bool prologue)
{
    if constexpr (kCheb)
        srpoly_step<kR>(a, prologue);
    else
        srcg_step<kR>(srcg_view(a), prologue);
}

// The poly library's plan choices (hpccg_poly.hip): kWaves 5 for the 27-wide
// four-column form over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_srpoly_spmm_a(SrpolyArgs a,
                                                                                                      bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srpoly_spmm_sell(SrpolyArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

// The SpMM loops with hpccg_poly_bodies.h's ends: step j applied to the row sums in registers.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_srpoly_cheb(SrpolyArgs a)
{
    spmm_a_body<kW, kR, PolyArgs, PolyStep>(a, false);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srpoly_cheb_sell(SrpolyArgs a)
{
    spmm_sell_body<kR, PolyArgs, PolyStep>(a, false);
}

__global__ __launch_bounds__(kFinThreads) void k_srpoly_finalize(SrpolyArgs a, int store_total)
{
    srcg_finalize(a, store_total);
}

// The diagonal of the image and the check of a caller's m: hpccg_jacobi.h's bodies.
__global__ __launch_bounds__(kBlock) void k_srpoly_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_srpoly_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// The symmetric Gershgorin bound's three kernels: hpccg_poly_bodies.h's bodies.
__global__ void k_srpoly_q(const double* __restrict__ m, int n, double* __restrict__ q)
{
    poly_q_body(m, n, q);
}

__global__ __launch_bounds__(kBlock) void k_srpoly_bound(DiagArgs a, const double* __restrict__ q,
                                                         double* __restrict__ smax)
{
    poly_bound_body(a, q, smax);
}

__global__ __launch_bounds__(kBlock) void k_srpoly_bound_top(const double* __restrict__ smax, int nslices,
                                                             double* __restrict__ out)
{
    poly_bound_top_body(smax, nslices, out);
}

// ---------------------------------------------------------------------------
// host: hpccg_poly_host.h and hpccg_srcg_host.h over this unit's kernels
// ---------------------------------------------------------------------------
// hpccg_poly_host.h's workspace with the recurrence's plain columns (w = A u is
// the engine's Ap).
struct Workspace : PolyWorkspace, SrcgColumns {
    void free_own_vectors()
    {
        PolyWorkspace::free_own_vectors();
        free_ps();
    }
};

struct Srpoly {
    using Args = SrpolyArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "srpoly";
    static constexpr const char* solve_name = "single-reduction polynomial";
    static long long row0(const Workspace* w) { return w->v.guard_rows; }

    static constexpr auto init = k_srpoly_init;
    template <int kR>
    static constexpr auto t = k_srpoly_t<kR>;
    // (degree 0: hpccg_srcg_bodies.h's step)
    template <int kR>
    static auto fused_step(const Workspace* w)
    {
        return w->degree > 0 ? k_srpoly_step<kR, true> : k_srpoly_step<kR, false>;
    }
    // (prologue: no u.w partial, the SpMM of t)
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_srpoly_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_srpoly_spmm_sell<kR>;
    template <int kW, int kR, int kWaves>
    static constexpr auto step = k_srpoly_cheb<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto step_sell = k_srpoly_cheb_sell<kR>;
    static constexpr auto finalize = k_srpoly_finalize;
    static constexpr auto diag = k_srpoly_diag;
    static constexpr auto check = k_srpoly_check;
    static constexpr auto q = k_srpoly_q;
    static constexpr auto bound = k_srpoly_bound;
    static constexpr auto bound_top = k_srpoly_bound_top;
};

SrpolyArgs make_srpoly_args(const Workspace* w, int nrhs, const double* m)
{
    SrpolyArgs a = make_args<Srpoly>(w, nrhs, m);  // (p: the guarded buffer of t; degree 0: of u)
    a.u = z_of<Srpoly>(w, w->degree & 1);
    a.zout = z_of<Srpoly>(w, 0);  // the step's: step 0's z
    a.pd = w->pd;
    a.sd = w->sd;
    return a;
}

// The fused step, then steps 1 .. d: u = z_d ends in buffer d & 1 (degree 0: u = m r in p's buffer).
void launch_step(const Workspace* w, const SrpolyArgs& a, bool prologue)
{
    launch_srcg_step<Srpoly>(w, a, prologue);
    for (int j = 1; j <= w->degree; j++) launch_step64<Srpoly>(w, step_args<Srpoly>(w, a, j));
}

// w = A u and the u.w slice partial: the SpMM with u in p's place.
void launch_spmm_u(const Workspace* w, SrpolyArgs a, bool prologue)
{
    if (w->degree > 0) a.p = const_cast<double*>(a.u);
    launch_spmm64<Srpoly>(w, a, prologue);
}

// The recurrence on the columns staged in the workspace's b and x.
int run_srpoly(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr,
               double* wall)
{
    return run_srcg<Srpoly>(w, make_srpoly_args(w, nrhs, m), nrhs, max_iter, tol, niters, normr, wall, launch_step,
                            launch_spmm_u);
}

// The solve: hpccg_poly_host.h's, with p and s beside its vectors and this unit's recurrence.
int solve_srpoly(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int degree, double lmin, double lmax, int max_iter, double tol, int* niters,
                 double* normr, double* times, bool host)
{
    return solve_common<Srpoly>(
        M, nrhs, B, ldb, X, ldx, minv, degree, lmin, lmax, max_iter, tol, niters, normr, times, host, nullptr,
        [](Workspace* w, int cap) { return alloc_ps(w, (size_t)w->v.npad * cap); }, run_srpoly);
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_srpoly_abi_version(void) { return 1; }

int hpccg_hip_srpoly_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                  long long ldx, const double* minv_dev, int degree, double lmin, double lmax,
                                  int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_srpoly(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance, niters,
                        normr, times, false);
}

int hpccg_hip_srpoly_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                           const double* minv, int degree, double lmin, double lmax, int max_iter, double tolerance,
                           int* niters, double* normr, double* times)
{
    return solve_srpoly(M, nrhs, B, ldb, X, ldx, minv, degree, lmin, lmax, max_iter, tolerance, niters, normr, times,
                        true);
}

int hpccg_hip_srpoly_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax)
{
    return poly_bound<Srpoly>(M, minv_dev, lmax);
}

int hpccg_hip_srpoly_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax)
{
    return poly_last_spectrum<Srpoly>(M, lmin, lmax);
}

int hpccg_hip_srpoly_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    return unit_last_trace<Srpoly>(M, col, out, cap);
}

int hpccg_hip_srpoly_release(hpccg_hip_matrix* M) { return unit_release<Srpoly>(M); }

int hpccg_hip_srpoly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Srpoly>(M, bytes);
}

int hpccg_hip_srpoly_live_workspaces(int* count) { return unit_live_workspaces<Srpoly>(count); }

}  // extern "C"
