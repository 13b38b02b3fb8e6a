// hpccg_mixed.hip -- mixed-precision CG (include/hpccg_hip_mixed.h,
// lib/libhpccg_hip_mixed.so): kernels and host code of the third library.
//
// The solve is HBM-bound on the matrix values, so they are held a second time
// in fp32 and streamed from there; every vector, every product and every sum is
// fp64 (a value is widened in the register). Where every value survives the
// round trip through float (exact) the fp32 image IS the matrix, and a column's
// solve is bitwise hpccg_hip_solve_device of it. Otherwise the fp32 image is the
// inner operator of an iterative refinement against the fp64 matrix.
//
// The fp32 image follows the image the matrix holds (SELL-512-A where it
// exists, else SELL-512), slice by slice with the same slot-row bases, so the
// offset tables / int32 columns are shared. Inside a slice the slots are
// interleaved in pairs: slot pair (2q, 2q + 1) is [512 rows][2 slots] laid out
// so that thread t (rows 2t, 2t + 1) reads one float4
//   { v[2q][2t], v[2q][2t + 1], v[2q + 1][2t], v[2q + 1][2t + 1] }
// at (base + 2q) * 512 + 4t: the value stream is 16 B per lane. An odd width's
// last slot is a plain [512 rows] run read 8 B per lane (one load in 14 at
// width 27), so the image is exactly 4 B per slot and no padded slot exists.
//
//   convert   k_mixed_convert: fp64 image -> fp32 image, counts the values that
//             do not survive the round trip and those outside fp32 range
//   SpMM      k_mixed_spmm_a<kW, kR> | k_mixed_spmm_sell<kR>: the fp64 slot
//             loops over the fp32 image, kR = 1, 2, 4 columns
//   p update, update, finalize: k_mixed_p, k_mixed_update, k_mixed_finalize
//             over the column engine's bodies (hpccg_columns.h), the loop
//             test's tolerance and iteration limit set per column by the host
//   residual  k_mixed_residual: r = b - A x from an fp64 A x with the r.r slice
//             partials | x = x + d (refinement)
// The recurrence itself -- the column's state, those bodies, the workspace
// registry and the launch loop -- is hpccg_columns.h; the image -- its convert
// body, its slot loops, its record and builder on the host -- is
// hpccg_spmm32.h, shared with hpccg_poly32.hip; the matrix check and the bodies
// of the release, workspace_bytes and live_workspaces exports are
// hpccg_onerank_host.h. This unit adds the frames of its two SpMM kernels and
// the refinement. Every dot keeps the rounding shape of hpccg_device.h. No
// kernel here waits on another block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/hpccg_hip_mixed.h"
#include "hpccg_onerank_host.h"
#include "hpccg_spmm32.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct MixedArgs : ColArgs {
    // (ColArgs' x and b: the caller's, ox and ob, where the fp32 image is the
    // matrix; the refinement's correction d and residual r_s otherwise; tot:
    // [cap] r.r totals of the residual step)
    double* ox;        // the caller's x
    double* ob;        // the caller's b
    const float* img;  // the fp32 values (layout above)
};

// fp64 image -> fp32 image with the two counts: hpccg_spmm32.h's body.
__global__ __launch_bounds__(kBlock) void k_mixed_convert(const double* __restrict__ vals,
                                                          const unsigned int* __restrict__ base_tab, int width,
                                                          float* __restrict__ img, unsigned long long* flags)
{
    convert32_body(vals, base_tab, width, img, flags);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_mixed_p(MixedArgs a, bool prologue)
{
    col_p<kR>(a, prologue);
}

// ---------------------------------------------------------------------------
// SpMM over the fp32 SELL-512-A image: hpccg_spmm32.h's slot loop (two slots
// per 16-B value load) in this unit's own frame, without the x-triple plan
// (this library's 27-wide four-column form is the plain slot loop). The frames
// of the two SpMM kernels stay here: as wrappers over spmm32_a_body /
// spmm32_sell_body the compiler lays out the four-column forms' address
// arithmetic differently (profiles/poly_host_refactor/README.md).
// kNT: the value loads are non-temporal. A template parameter of the kernel,
// chosen on the host from the view's nt flag: as a branch inside the kernel
// the two arms differ in the hint alone, the optimiser merges them and the
// hint is lost (so it was with one column, where no other arm keeps them apart).
// amdgpu_waves_per_eu(4): the register budget (at most 128 VGPRs; the batch
// library's default), not a tuned target.
// ---------------------------------------------------------------------------
template <int kW, bool kNT, int kR>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_mixed_spmm_a(MixedArgs a,
                                                                                                bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    bool act[kR], all;
    if (!active_cols<kR>(a, act, all)) return;
    const int wdt = kW > 0 ? kW : (int)(sld(a.abase + s + 1) - sld(a.abase + s));
    const size_t vb = kW > 0 ? (size_t)s * kW : (size_t)sld(a.abase + s);
    const float* __restrict__ base = a.img + vb * kSliceRows;
    const int* __restrict__ off = a.aoff + (size_t)s * kAMax;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    const double* __restrict__ xr = a.p + (size_t)a.c0 * a.pcs + row;  // column c0 + c: x of column row + off at xr[c * pcs + off]
    double sum[kR][kRpt];
#pragma unroll
    for (int c = 0; c < kR; c++)
#pragma unroll
        for (int i = 0; i < kRpt; i++) sum[c][i] = 0.0;
    if (all)
        spmm32_a_slots<kW, kR, kNT, true>(a, base, off, wdt, xr, act, sum);
    else
        spmm32_a_slots<kW, kR, kNT, false>(a, base, off, wdt, xr, act, sum);
    spmm_rows_out<kR>(a, prologue, s, row, act, sum);
}

// ---------------------------------------------------------------------------
// SpMM over the fp32 SELL-512 image (the shared int32 columns; matrices
// without an A image): hpccg_spmm32.h's slot step. Padding slots (column -1,
// value 0) add +0.
// ---------------------------------------------------------------------------
template <bool kNT, int kR>
__global__ __launch_bounds__(kBlock) void k_mixed_spmm_sell(MixedArgs a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    bool act[kR], all;
    if (!active_cols<kR>(a, act, all)) return;
    const size_t sb = (size_t)sld(a.slice_base + s) * kSliceRows;
    const int w = (int)(sld(a.slice_base + s + 1) - sld(a.slice_base + s));
    const float* __restrict__ base = a.img + sb;
    const int* __restrict__ cp = a.cols + sb + (size_t)threadIdx.x * kRpt;
    const double* __restrict__ x0 = a.p + ((long long)a.c0 * a.pcs + a.xsell);
    double sum[kR][kRpt];
#pragma unroll
    for (int c = 0; c < kR; c++)
#pragma unroll
        for (int i = 0; i < kRpt; i++) sum[c][i] = 0.0;
    typedef int i2v __attribute__((ext_vector_type(2)));
    const int np = w >> 1;
#pragma unroll 2
    for (int q = 0; q < np; q++) {
        const f4v v = ld_f4<kNT>(base + (size_t)(2 * q) * kSliceRows + (size_t)threadIdx.x * 4);
        const i2v ca = *reinterpret_cast<const i2v*>(cp + (size_t)(2 * q) * kSliceRows);
        const i2v cb = *reinterpret_cast<const i2v*>(cp + (size_t)(2 * q + 1) * kSliceRows);
        slot32_sell<kR>(a, v.x, v.y, ca.x, ca.y, x0, act, sum);
        slot32_sell<kR>(a, v.z, v.w, cb.x, cb.y, x0, act, sum);
    }
    if (w & 1) {  // (block-uniform) the odd width's last slot
        const f2v v = ld_f2<kNT>(base + (size_t)(w - 1) * kSliceRows + (size_t)threadIdx.x * 2);
        const i2v ca = *reinterpret_cast<const i2v*>(cp + (size_t)(w - 1) * kSliceRows);
        slot32_sell<kR>(a, v.x, v.y, ca.x, ca.y, x0, act, sum);
    }
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    spmm_rows_out<kR>(a, prologue, s, row, act, sum);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_mixed_update(MixedArgs a, bool prologue)
{
    col_update<kR>(a, prologue);
}

// ---------------------------------------------------------------------------
// The refinement's fp64 steps, per column marked running:
//   residual (correct 0): r_s = b + (-1.0)*(A x), A x in Ap from the fp64
//            matrix; stored as the inner recurrence's right-hand side, with
//            the r_s.r_s slice partials
//   correct 1: x = x + d
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_mixed_residual(MixedArgs a, int correct)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    for (int c = 0; c < a.nrhs; c++) {
        if (!a.st[c].run) continue;  // (block-uniform)
        const size_t co = (size_t)c * a.vcs;
        if (correct) {
            const Rows xv = ld(a.ox + co + row);
            const Rows dv = ld(a.x + co + row);
            Rows xn;
#pragma unroll
            for (int i = 0; i < kRpt; i++) xn.v[i] = xv.v[i] + dv.v[i];
            st_rows(a.ox + co, row, a.n, xn);
            continue;
        }
        const Rows bv = ld(a.ob + co + row);
        const Rows av = ld(a.Ap + co + row);
        Rows rn;
#pragma unroll
        for (int i = 0; i < kRpt; i++) rn.v[i] = bv.v[i] + (-1.0) * av.v[i];
        st_rows(a.b + co, row, a.n, rn);
        rr_slice_partial(a, s, row, c, rn);
    }
}

// store_total (the refinement's residual step): the r.r total is stored in
// tot[c] and the state is left alone.
__global__ __launch_bounds__(kFinThreads) void k_mixed_finalize(MixedArgs a, int which, int store_total)
{
    col_finalize(a, which, store_total);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
constexpr double kInnerRtolDefault = 0x1p-20;

// What the last solve did on one column.
struct ColRecord {
    std::vector<double> trace;  // the inner recurrences' normr, sweep after sweep
    std::vector<int> iters;     // it_s
    std::vector<double> resid;  // rho_s, then the final residual
};

struct Workspace : ColWorkspace, Image32 {
    // the vectors of its own
    bool refine = false;  // x, b are buffers of their own (the refinement's d, r_s)
    double *r = nullptr, *x = nullptr, *b = nullptr, *ox = nullptr, *ob = nullptr;
    std::vector<ColState> hst;
    std::vector<ColRecord> rec;  // per column of the last solve

    void free_own_vectors()
    {
        for (double* q : {r, x, b, ox, ob})
            if (q) (void)hipFree(q);
        r = x = b = ox = ob = nullptr;
        refine = false;
    }
    void free_own_rest() { free_image(); }
    long long total_bytes() const { return bytes + img_bytes; }
};

// The fp32 image, built once per matrix (hpccg_spmm32.h).
int ensure_image(Workspace* w)
{
    return ensure_image32(w, w->v, k_mixed_convert, "mixed");
}

// Room for ncols columns and a history of max_iter + 1 entries per column;
// refine: the refinement's two further vectors per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter, bool refine)
{
    refine = refine || w->refine;
    const size_t npad = (size_t)w->v.npad;
    const long long pcs = (long long)(npad + 2 * (size_t)w->v.guard_rows);  // a p column: [guard | rows (padded) | guard]
    return ensure_columns(w, ncols, max_iter, refine == w->refine, pcs, 1, [&](int cap) {
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->ox, npad * cap));
        TRY(alloc_zero(w, &w->ob, npad * cap));
        if (refine) TRY(alloc_zero(w, &w->x, npad * cap));
        if (refine) TRY(alloc_zero(w, &w->b, npad * cap));
        w->refine = refine;
        return 0;
    });
}

// What hpccg_onerank_host.h's matrix check and bookkeeping bodies go by.
struct Mixed {
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "mixed";
};

// inner: the recurrence runs on the refinement's (r_s, d) instead of (b, x)
MixedArgs make_args(const Workspace* w, int nrhs, bool inner)
{
    MixedArgs a{};
    fill_args(&a, w, nrhs);
    a.nt = a.nt && !std::getenv("HPCCG_MIXED_NO_NT");  // (diagnostics: the A/B of the non-temporal value loads)
    a.p = w->pbuf + w->v.guard_rows;
    a.r = w->r;
    a.rcs = w->vcs;
    a.ox = w->ox;
    a.ob = w->ob;
    a.x = inner ? w->x : w->ox;
    a.b = inner ? w->b : w->ob;
    a.img = w->img;
    return a;
}

#define HPCCG_MIXED_R(KERNEL, ...)                                                         \
    do {                                                                                   \
        if (R == 4)                                                                        \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 4>), g, b, 0, s, a, prologue);          \
        else if (R == 2)                                                                   \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 2>), g, b, 0, s, a, prologue);          \
        else                                                                               \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 1>), g, b, 0, s, a, prologue);          \
    } while (0)

void launch_spmm(const Workspace* w, MixedArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
#define HPCCG_MIXED_NT(KERNEL, ...)                      \
    do {                                                \
        if (a.nt)                                       \
            HPCCG_MIXED_R(KERNEL, __VA_ARGS__ true, );  \
        else                                            \
            HPCCG_MIXED_R(KERNEL, __VA_ARGS__ false, ); \
    } while (0)
        if (!w->v.has_a)
            HPCCG_MIXED_NT(k_mixed_spmm_sell, );
        else if (a.a_width == 27)
            HPCCG_MIXED_NT(k_mixed_spmm_a, 27, );
        else if (a.a_width == 7)
            HPCCG_MIXED_NT(k_mixed_spmm_a, 7, );
        else
            HPCCG_MIXED_NT(k_mixed_spmm_a, 0, );
#undef HPCCG_MIXED_NT
    });
}

void launch_p(const Workspace* w, MixedArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_MIXED_R(k_mixed_p, );
    });
}

void launch_update(const Workspace* w, MixedArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_MIXED_R(k_mixed_update, );
    });
}
#undef HPCCG_MIXED_R

void launch_finalize(const Workspace* w, const MixedArgs& a, int which, int store_total = 0)
{
    hipLaunchKernelGGL(k_mixed_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, store_total);
}

// The columns' states for the next launches: column c runs (fresh, with its
// tolerance and limit) where run[c]. (Every upload is followed by a host
// synchronisation before hst changes again.)
int set_states(Workspace* w, int nrhs, const std::vector<char>& run, const std::vector<double>& tol,
               const std::vector<int>& max_iter)
{
    w->hst.assign(nrhs, ColState{});
    for (int c = 0; c < nrhs; c++) {
        w->hst[c].run = run[c] ? 1 : 0;
        w->hst[c].tol = tol[c];
        w->hst[c].max_iter = max_iter[c];
    }
    HIP_TRY(hipMemcpyAsync(w->st, w->hst.data(), sizeof(ColState) * nrhs, hipMemcpyHostToDevice, w->v.stream));
    HIP_TRY(hipMemsetAsync(w->ended, 0, sizeof(int), w->v.stream));
    return 0;
}

// One CG recurrence per column marked run in the states just set: on (b, x) of
// a. it[c] and the trace appended to rec[c] for those columns.
int run_cg(Workspace* w, const MixedArgs& a, const std::vector<char>& run, const std::vector<int>& max_iter,
           std::vector<int>& it)
{
    const int nrhs = a.nrhs;
    int nrun = 0, kmax = 1;
    for (int c = 0; c < nrhs; c++)
        if (run[c]) {
            nrun++;
            kmax = std::max(kmax, max_iter[c]);
        }
    TRY(run_recurrence(w, a, nrun, kmax, launch_p, launch_spmm, launch_update, launch_finalize));
    std::vector<ColState> st;
    std::vector<double> hist;
    TRY(read_columns(w, nrhs, &st, &hist));
    for (int c = 0; c < nrhs; c++)
        if (run[c]) it[c] = column_trace(st[c], hist.data() + (size_t)c * (size_t)w->hstride, &w->rec[c].trace);
    return 0;
}

// The solve on the columns staged in the workspace's ob and ox.
int run_solve(hpccg_hip_matrix* M, Workspace* w, int nrhs, int max_iter, double tol, int max_sweeps, double inner_rtol,
              int* niters, double* normr)
{
    hipStream_t s = w->v.stream;
    w->rec.assign(nrhs, {});
    std::vector<char> live(nrhs, 1);
    std::vector<double> tols(nrhs, tol);
    std::vector<int> limit(nrhs, max_iter), it(nrhs, 0);
    if (w->inexact == 0) {  // the fp32 image is the matrix: the solve itself
        const MixedArgs a = make_args(w, nrhs, false);
        TRY(set_states(w, nrhs, live, tols, limit));
        TRY(run_cg(w, a, live, limit, it));
        for (int c = 0; c < nrhs; c++) {
            ColRecord& rc = w->rec[c];
            niters[c] = it[c];
            normr[c] = rc.trace[it[c]];
            rc.iters = {it[c]};
            rc.resid = {rc.trace[0], normr[c]};
        }
        return 0;
    }
    const MixedArgs a = make_args(w, nrhs, true);
    std::vector<int> left(nrhs, max_iter - 1);
    std::vector<double> rr(nrhs, 0.0);
    for (int c = 0; c < nrhs; c++) niters[c] = 0;
    for (int sweep = 0;; sweep++) {
        // 1. r_s = b - A x_s against the fp64 matrix, rho_s
        for (int c = 0; c < nrhs; c++)
            if (live[c]) TRY(hpccg_hip_sparsemv(M, w->ox + (size_t)c * w->vcs, w->Ap + (size_t)c * w->vcs));
        TRY(set_states(w, nrhs, live, tols, limit));
        hipLaunchKernelGGL(k_mixed_residual, dim3(a.grid), dim3(kBlock), 0, s, a, 0);
        launch_finalize(w, a, kDotRR, 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rr.data(), w->tot, sizeof(double) * nrhs, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // 2. the columns that stop here
        bool any = false;
        for (int c = 0; c < nrhs; c++) {
            if (!live[c]) continue;
            const double rho = std::sqrt(rr[c]);
            w->rec[c].resid.push_back(rho);
            normr[c] = rho;
            // (a residual that is not finite or exactly zero gives the inner
            // recurrence nothing to solve for, whatever the tolerance: x stays)
            if (rho <= tol || !std::isfinite(rho) || rho == 0.0 || sweep == max_sweeps || left[c] == 0) {
                live[c] = 0;
                continue;
            }
            any = true;
            tols[c] = std::max(tol, inner_rtol * rho);
            limit[c] = left[c] + 1;
            HIP_TRY(hipMemsetAsync(w->x + (size_t)c * w->vcs, 0, sizeof(double) * (size_t)w->vcs, s));
        }
        if (!any) return 0;
        // 3. the recurrence on A~ d = r_s from d = 0
        TRY(set_states(w, nrhs, live, tols, limit));
        TRY(run_cg(w, a, live, limit, it));
        // 4. x_{s+1} = x_s + d
        TRY(set_states(w, nrhs, live, tols, limit));
        hipLaunchKernelGGL(k_mixed_residual, dim3(a.grid), dim3(kBlock), 0, s, a, 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        for (int c = 0; c < nrhs; c++) {
            if (!live[c]) continue;
            w->rec[c].iters.push_back(it[c]);
            left[c] -= it[c];
            niters[c] += it[c];
        }
    }
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx, int max_iter,
                 double tol, int max_sweeps, double inner_rtol, int* niters, double* normr, double* times, bool host)
{
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "mixed: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "mixed: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "mixed: max_iter %d is negative", max_iter);
    if (max_sweeps < 1) return fail(HPCCG_HIP_EINVAL, "mixed: max_sweeps %d (at least 1)", max_sweeps);
    if (std::isnan(inner_rtol) || inner_rtol >= 1.0)
        return fail(HPCCG_HIP_EINVAL, "mixed: inner_rtol %g (in [0, 1); negative: the default)", inner_rtol);
    if (inner_rtol < 0.0) inner_rtol = kInnerRtolDefault;
    MatrixView v;
    TRY(check_matrix(Mixed::who, M, &v));
    if (ldb < v.n || ldx < v.n)
        return fail(HPCCG_HIP_EINVAL, "mixed: leading dimensions %lld, %lld below the %d rows", ldb, ldx, v.n);
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
        TRY(ensure_image(w));
        TRY(ensure_vectors(w, nrhs, max_iter, w->inexact != 0));
        const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        const hipMemcpyKind out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        const auto t0 = std::chrono::steady_clock::now();
        TRY(copy_cols(w, w->ob, w->vcs, B, ldb, nrhs, in));
        TRY(copy_cols(w, w->ox, w->vcs, X, ldx, nrhs, in));
        if (host) HIP_TRY(hipStreamSynchronize(v.stream));
        const auto t1 = std::chrono::steady_clock::now();
        HIP_TRY(hipEventRecord(w->ev0, v.stream));
        TRY(run_solve(M, w, nrhs, max_iter, tol, max_sweeps, inner_rtol, niters, normr));
        HIP_TRY(hipEventRecord(w->ev1, v.stream));
        const auto t2 = std::chrono::steady_clock::now();
        TRY(copy_cols(w, X, ldx, w->ox, w->vcs, nrhs, out));
        HIP_TRY(hipStreamSynchronize(v.stream));
        const auto t3 = std::chrono::steady_clock::now();
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, w->ev0, w->ev1));
        if (times) {
            times[0] = 1e-3 * ms;
            if (host) times[6] = std::chrono::duration<double>((t1 - t0) + (t3 - t2)).count();
        }
        return 0;
    });
}

const ColRecord* find_record(const hpccg_hip_matrix* M, int col, const char* what)
{
    const Workspace* w = g_ws<Workspace>.find(M);
    if (!w || col < 0 || col >= (int)w->rec.size()) {
        fail(HPCCG_HIP_EINVAL, "mixed: no %s of column %d (the last mixed solve had %d)", what, col,
             w ? (int)w->rec.size() : 0);
        return nullptr;
    }
    return &w->rec[col];
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_mixed_abi_version(void) { return 1; }

int hpccg_hip_mixed_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                 long long ldx, int max_iter, double tolerance, int max_sweeps, double inner_rtol,
                                 int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B_dev, ldb, X_dev, ldx, max_iter, tolerance, max_sweeps, inner_rtol, niters, normr,
                        times, false);
}

int hpccg_hip_mixed_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                          int max_iter, double tolerance, int max_sweeps, double inner_rtol, int* niters, double* normr,
                          double* times)
{
    return solve_common(M, nrhs, B, ldb, X, ldx, max_iter, tolerance, max_sweeps, inner_rtol, niters, normr, times,
                        true);
}

int hpccg_hip_mixed_sparsemv(hpccg_hip_matrix* M, int nrhs, const double* X_dev, long long ldx, double* Y_dev,
                             long long ldy)
{
    if (!M || !X_dev || !Y_dev) return fail(HPCCG_HIP_EINVAL, "mixed: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "mixed: nrhs %d (at least 1)", nrhs);
    MatrixView v;
    TRY(check_matrix(Mixed::who, M, &v));
    if (ldx < v.n || ldy < v.n)
        return fail(HPCCG_HIP_EINVAL, "mixed: leading dimensions %lld, %lld below the %d rows", ldx, ldy, v.n);
    if (v.n == 0) return 0;
    return keep_device([&]() -> int {
        Workspace* w = nullptr;
        TRY(g_ws<Workspace>.record(M, v, &w));
        TRY(ensure_image(w));
        TRY(ensure_vectors(w, nrhs, 1, false));
        // x into the guarded p columns, Ap = A~ p, Ap out
        MixedArgs a = make_args(w, nrhs, false);
        a.force = 1;
        TRY(copy_cols(w, a.p, w->pcs, X_dev, ldx, nrhs, hipMemcpyDeviceToDevice));
        launch_spmm(w, a, true);
        HIP_TRY(hipGetLastError());
        TRY(copy_cols(w, Y_dev, ldy, w->Ap, w->vcs, nrhs, hipMemcpyDeviceToDevice));
        HIP_TRY(hipStreamSynchronize(v.stream));
        return 0;
    });
}

int hpccg_hip_mixed_info(hpccg_hip_matrix* M, long long out[4])
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "mixed: NULL argument");
    MatrixView v;
    TRY(check_matrix(Mixed::who, M, &v));
    out[0] = 1;
    out[1] = out[2] = out[3] = 0;
    if (v.n == 0) return 0;
    return keep_device([&]() -> int {
        Workspace* w = nullptr;
        TRY(g_ws<Workspace>.record(M, v, &w));
        TRY(ensure_image(w));
        out[0] = w->inexact == 0 ? 1 : 0;
        out[1] = w->img_bytes;
        out[2] = w->bytes;
        out[3] = w->inexact;
        return 0;
    });
}

int hpccg_hip_mixed_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "mixed: NULL argument");
    const ColRecord* r = find_record(M, col, "trace");
    if (!r) return HPCCG_HIP_EINVAL;
    const int n = std::min<int>(std::max(cap, 0), (int)r->trace.size());
    for (int i = 0; i < n; i++) out[i] = r->trace[i];
    return n;
}

int hpccg_hip_mixed_last_sweeps(const hpccg_hip_matrix* M, int col, int* iters, double* resid, int cap)
{
    if (!M || !iters || !resid) return fail(HPCCG_HIP_EINVAL, "mixed: NULL argument");
    const ColRecord* r = find_record(M, col, "sweeps");
    if (!r) return HPCCG_HIP_EINVAL;
    cap = std::max(cap, 0);
    for (int i = 0; i < std::min<int>(cap, (int)r->iters.size()); i++) iters[i] = r->iters[i];
    for (int i = 0; i < std::min<int>(cap, (int)r->resid.size()); i++) resid[i] = r->resid[i];
    return (int)r->iters.size();
}

int hpccg_hip_mixed_release(hpccg_hip_matrix* M) { return unit_release<Mixed>(M); }

int hpccg_hip_mixed_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Mixed>(M, bytes);
}

int hpccg_hip_mixed_live_workspaces(int* count) { return unit_live_workspaces<Mixed>(count); }

}  // extern "C"
