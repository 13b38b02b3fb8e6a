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
// entry points here are wrappers over it. The host code -- the workspace, the
// launchers, the bound, the interval -- is hpccg_poly_host.h, shared with that
// unit and with hpccg_poly32.hip, over hpccg_onerank_host.h (the dispatch, the
// checks, the preconditioner, the solve, the bookkeeping exports), shared with
// hpccg_pcg.hip and hpccg_srcg.hip; this unit hands them its kernels.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_poly.h"
#include "hpccg_poly_host.h"

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
// host: hpccg_poly_host.h over this unit's kernels
// ---------------------------------------------------------------------------
struct Poly {
    using Args = PolyArgs;
    using Workspace = PolyWorkspace;
    static constexpr const char* who = "poly";
    static constexpr const char* solve_name = "polynomial";
    static long long row0(const Workspace* w) { return w->v.guard_rows; }

    static constexpr auto init = k_poly_init;
    template <int kR, bool kPre>
    static constexpr auto p = k_poly_p<kR, kPre>;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_poly_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_poly_spmm_sell<kR>;
    template <int kR, bool kCheb>
    static constexpr auto update = k_poly_update<kR, kCheb>;
    template <int kW, int kR, int kWaves>
    static constexpr auto step = k_poly_step<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto step_sell = k_poly_step_sell<kR>;
    static constexpr auto finalize = k_poly_finalize;
    static constexpr auto diag = k_poly_diag;
    static constexpr auto check = k_poly_check;
    static constexpr auto q = k_poly_q;
    static constexpr auto bound = k_poly_bound;
    static constexpr auto bound_top = k_poly_bound_top;

    // the SpMM and the steps stream the fp64 image
    static void launch_spmm(const Workspace* w, Args a, bool prologue) { launch_spmm64<Poly>(w, a, prologue); }
    static void launch_step(const Workspace* w, Args a) { launch_step64<Poly>(w, a); }
};

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_poly_abi_version(void) { return 1; }

int hpccg_hip_poly_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                long long ldx, const double* minv_dev, int degree, double lmin, double lmax,
                                int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_common<Poly>(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, degree, lmin, lmax, max_iter, tolerance,
                              niters, normr, times, false);
}

int hpccg_hip_poly_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                         const double* minv, int degree, double lmin, double lmax, int max_iter, double tolerance,
                         int* niters, double* normr, double* times)
{
    return solve_common<Poly>(M, nrhs, B, ldb, X, ldx, minv, degree, lmin, lmax, max_iter, tolerance, niters, normr,
                              times, true);
}

int hpccg_hip_poly_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax)
{
    return poly_bound<Poly>(M, minv_dev, lmax);
}

int hpccg_hip_poly_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax)
{
    return poly_last_spectrum<Poly>(M, lmin, lmax);
}

int hpccg_hip_poly_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    return unit_last_trace<Poly>(M, col, out, cap);
}

int hpccg_hip_poly_release(hpccg_hip_matrix* M) { return unit_release<Poly>(M); }

int hpccg_hip_poly_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Poly>(M, bytes);
}

int hpccg_hip_poly_live_workspaces(int* count) { return unit_live_workspaces<Poly>(count); }

}  // extern "C"
