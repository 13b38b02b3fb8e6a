// hpccg_batch.hip -- batched multi-right-hand-side CG (include/hpccg_hip_batch.h,
// lib/libhpccg_hip_batch.so): kernels and host code of the second library.
//
// The single solve is HBM-bound on the matrix image (27-pt: 216 B per row per
// iteration against a few tens of bytes of vectors), so several right-hand
// sides against one matrix are solved by reading every value slot once for kR
// columns (SpMM). Every column is an independent CG recurrence with the single
// solve's expressions and the single solve's dot shape (hpccg_device.h), so
// column c is bitwise hpccg_hip_solve_device of that column:
//   SpMM      k_batch_spmm_a<kW, kR> (SELL-512-A, x read at the slice's
//             offsets, k_spmv_a's slot order) | k_batch_spmm_sell<kR> (SELL-512,
//             int32 columns) + the p.Ap slice partial per column
//   p update  k_batch_p<kR>: p = x + 0 x (prologue) | p = r + beta_c p
//   update    k_batch_update<kR>: r = b - Ap (prologue) | x += alpha_c p,
//             r -= alpha_c Ap, + the r.r slice partial per column
//   finalize  k_batch_finalize: one block per column; slice partials -> groups
//             of 64 -> top level, then the column's scalar state on the device
//             (alpha, beta, rtrans, hist, the reference's loop test)
// Launches are eager on the matrix's stream with no host synchronisation per
// iteration; every kCheckEvery iterations the host reads one word (columns
// ended) and stops launching when all have. A column that has ended is frozen:
// its blocks skip its loads and stores (block-uniform branches). No kernel here
// waits on another block.
//
// Over an in-process rank group (include/hpccg_hip_batch_group.h; the last part
// of the host code): every member runs these kernels on its rows, the ghost
// planes of every column's p are copied between the members' p columns after
// k_batch_p, k_batch_finalize stores each member's local total only (local),
// and k_batch_group_sum adds the totals in rank order and advances the column's
// state on every member. Column c is bitwise hpccg_hip_group_solve of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/hpccg_hip_batch.h"
#include "../../include/hpccg_hip_batch_group.h"
#include "hpccg_device.h"
#include "hpccg_internal.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// Per-column scalar state, advanced by k_batch_finalize only (a group member's:
// by k_batch_group_sum only).
struct ColState {
    double rtrans;     // r_{k-1}.r_{k-1} of the iteration k about to run (HPCCG.cpp: rtrans)
    double oldrtrans;  // r_{k-2}.r_{k-2}
    double pap;        // p_k.Ap_k
    double alpha;      // rtrans / pap
    double beta;       // rtrans / oldrtrans (0.0 for k = 1)
    int k;             // the iteration about to run (0: the prologue)
    int run;           // 1: iteration k runs (the prologue always does)
    int niters;        // iterations done once the column has ended
    int pad;
};

enum Dot : int { kDotRR = 0, kDotPAP = 1 };

struct BatchArgs {
    int n, nslices, grid;
    int nrhs;      // columns of the batch
    int c0;        // first column of this launch (it covers c0 .. c0 + kR - 1, those < nrhs)
    int cap;       // columns the workspace holds (stride of the partials)
    int ng;        // ceil(nslices / kGroup)
    int max_iter;
    double tol;
    int force;     // 1: every column runs whatever its state (the plain SpMM)
    int nt, a_width;
    int tri;       // width 27: slices whose offsets come in runs of three use the x-triple plan
    double* p;    // local row 0 of column 0; column c at p + c * pcs (guard zones around each;
                  // a group member: ghost_lo rows below row 0, ghost_hi rows from row n)
    long long xsell;  // SELL-512 column 0 relative to local row 0 (a group member: -ghost_lo)
    double* tot;      // [2][cap] a group member's local dot totals (k_batch_finalize, local)
    double* r;
    double* Ap;    // column c at Ap + c * vcs
    double* x;
    double* b;
    long long pcs, vcs;
    double* partial;  // [2][cap][nslices] slice partials (r.r, then p.Ap)
    double* gsum;     // [2][cap][ng] group sums (beyond the finalize block's LDS only)
    ColState* st;     // [cap]
    double* hist;     // [cap][hstride]: hist[c][k] = r_k.r_k
    long long hstride;
    int* ended;       // columns whose loop has ended
    const double* aval;
    const int* aoff;
    const unsigned int* abase;
    const unsigned int* slice_base;
    const int* cols;
    const double* vals;
};

// Wave-uniform table loads through the scalar cache (tables no kernel writes).
template <class T>
__device__ __forceinline__ T sld(const T* p)
{
    return *(const __attribute__((address_space(4))) T*)(p);
}

template <int kR>
__device__ __forceinline__ bool active_cols(const BatchArgs& a, bool (&act)[kR], bool& all)
{
    bool any = false;
    all = true;
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        act[j] = c < a.nrhs && (a.force || a.st[c].run != 0);
        any = any || act[j];
        all = all && act[j];
    }
    return any;
}

__device__ __forceinline__ double* slice_partials(const BatchArgs& a, int which, int c)
{
    return a.partial + ((size_t)which * a.cap + c) * (size_t)a.nslices;
}

__global__ void k_batch_init(BatchArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) *a.ended = 0;
    if (c >= a.nrhs) return;
    ColState s;
    s.rtrans = s.oldrtrans = s.pap = s.alpha = s.beta = 0.0;
    s.k = 0;
    s.run = 1;
    s.niters = 0;
    s.pad = 0;
    a.st[c] = s;
}

// ---------------------------------------------------------------------------
// p = x + 0.0*x (prologue, HPCCG.cpp:347) | p = r + beta*p (k_p_update's
// expression: k == 1 reads r for p, beta 0.0), per running column.
// ---------------------------------------------------------------------------
template <int kR>
__global__ __launch_bounds__(kBlock) void k_batch_p(BatchArgs a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        if (c >= a.nrhs) break;
        double* __restrict__ pc = a.p + (size_t)c * a.pcs;
        Rows o;
        if (prologue) {
            const Rows xv = ld(a.x + (size_t)c * a.vcs + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) o.v[i] = xv.v[i] + 0.0 * xv.v[i];
        } else {
            if (!a.st[c].run) continue;
            const int k = a.st[c].k;
            const double beta = a.st[c].beta;
            const Rows rv = ld(a.r + (size_t)c * a.pcs + row);
            const Rows yv = (k == 1) ? rv : ld(pc + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) o.v[i] = rv.v[i] + beta * yv.v[i];
        }
        st_rows(pc, row, a.n, o);
    }
}

// The SpMM epilogue of one column's two rows: store Ap; the rows' p.Ap terms
// in spmv_rows_out's order, the slice partial by block_sum.
template <int kR>
__device__ __forceinline__ void spmm_rows_out(const BatchArgs& a, bool prologue, int s, int row, const bool (&act)[kR],
                                              const double (&sum)[kR][kRpt])
{
#pragma unroll
    for (int j = 0; j < kR; j++) {
        if (!act[j]) continue;  // (block-uniform)
        const int c = a.c0 + j;
        st_rows(a.Ap + (size_t)c * a.vcs, row, a.n, Rows{{sum[j][0], sum[j][1]}});
        if (prologue) continue;  // HPCCG.cpp:351: the prologue SpMV has no p.Ap
        const Rows pv = ld(a.p + (size_t)c * a.pcs + row);
        double d = 0.0;
#pragma unroll
        for (int i = 0; i < kRpt; i++)
            if (row + i < a.n) d += pv.v[i] * sum[j][i];
        const double bs = block_sum<kBlock>(d);
        if (threadIdx.x == 0) slice_partials(a, kDotPAP, c)[s] = bs;
        __syncthreads();  // block_sum's LDS words are free for the next column
    }
}

// ---------------------------------------------------------------------------
// SpMM over SELL-512-A: k_spmv_a's slot loop with kR running sums per row. A
// value slot pair is loaded once; column c's x is p_c at the slice's offsets
// (holes: 0.0 times a finite word of p_c's zeroed guard zone or a real
// neighbour). Per row and column the products are added in slot order with no
// contraction: the single kernel's row sum.
// ---------------------------------------------------------------------------
template <int kW, int kR, bool kNT, bool kAll>
__device__ __forceinline__ void spmm_a_slots(const BatchArgs& a, const double* __restrict__ vp,
                                             const int* __restrict__ off, int wdt, const double* __restrict__ xr,
                                             const bool (&act)[kR], double (&sum)[kR][kRpt])
{
#pragma unroll kW > 0 ? kW : 4
    for (int j = 0; j < wdt; j++) {
        const Rows v = ld_m<kNT>(vp + (size_t)j * kSliceRows);
        const int oj = sld(off + j);
#pragma unroll
        for (int c = 0; c < kR; c++) {
            if (kAll || act[c]) {
                const Rows xv = ld_u(xr + ((long long)c * a.pcs + oj));
#pragma unroll
                for (int i = 0; i < kRpt; i++) sum[c][i] = sum[c][i] + v.v[i] * xv.v[i];
            }
        }
    }
}

// The x-triple plan of the 27-point width (k_spmv_a's kTri, here for nine
// triples): an interior slice's ascending offsets come in runs o - 1, o, o + 1
// (the x neighbours of each of the nine (y, z) neighbours). One 16-B load of
// the centre pair serves the run: row 2t's left neighbour and row 2t + 1's
// right neighbour come from the adjacent lanes (wave_shr1 / wave_shl1), lanes 0
// and 63 load their one outside value. The same x values in the same products
// in slot order: the same bits, a third of the x loads. With kR columns the
// gathers, not the value stream, set this kernel's time (27 x kR 16-B loads per
// thread from L2; 200^3, four columns: 616 us a launch against 430 us for its
// bytes at the update kernel's rate). Same-box A/B of the plan, two rounds:
// 200^3 four columns 3803 -> 4008 RHS-iterations/s, 100^3 29 970 -> 30 620
// (DESIGN.md 10).
constexpr int kTriples = 9;

template <int kR, bool kNT>
__device__ __forceinline__ void spmm_a_triples(const BatchArgs& a, const double* __restrict__ vp,
                                               const int* __restrict__ off, const double* __restrict__ xr,
                                               double (&sum)[kR][kRpt])
{
    const int lane = threadIdx.x & (kWave - 1);
    // (one run of kR columns in flight per thread: fully unrolled the
    // scheduler hoists every load of the slice, 280-430 VGPRs; three runs 158)
#pragma unroll 1
    for (int g = 0; g < kTriples; g++) {
        const Rows v0 = ld_m<kNT>(vp + (size_t)(3 * g) * kSliceRows);
        const Rows v1 = ld_m<kNT>(vp + (size_t)(3 * g + 1) * kSliceRows);
        const Rows v2 = ld_m<kNT>(vp + (size_t)(3 * g + 2) * kSliceRows);
        const int o = sld(off + 3 * g + 1);  // the run's centre offset
#pragma unroll
        for (int c = 0; c < kR; c++) {
            const double* __restrict__ xc = xr + ((long long)c * a.pcs + o);
            const Rows ctr = ld_u(xc);
            double left = wave_shr1(ctr.v[1]);
            double right = wave_shl1(ctr.v[0]);
            if (lane == 0) left = xc[-1];
            if (lane == kWave - 1) right = xc[2];
            sum[c][0] = sum[c][0] + v0.v[0] * left;
            sum[c][1] = sum[c][1] + v0.v[1] * ctr.v[0];
            sum[c][0] = sum[c][0] + v1.v[0] * ctr.v[0];
            sum[c][1] = sum[c][1] + v1.v[1] * ctr.v[1];
            sum[c][0] = sum[c][0] + v2.v[0] * ctr.v[1];
            sum[c][1] = sum[c][1] + v2.v[1] * right;
        }
    }
}

// kWaves: the occupancy the kernel is compiled for (waves per SIMD). The
// 27-wide four-column form exists twice: at 5 (92 VGPRs) for images streamed
// from HBM and at 4 (102) for images the Infinity Cache holds -- same box,
// against the sequential solves: 200^3 1.59x at 5 and 1.52x at 4, 100^3 1.30x
// at 5 and 1.38x at 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_batch_spmm_a(BatchArgs a,
                                                                                                     bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    bool act[kR], all;
    if (!active_cols<kR>(a, act, all)) return;
    const int wdt = kW > 0 ? kW : (int)(sld(a.abase + s + 1) - sld(a.abase + s));
    const size_t vb = kW > 0 ? (size_t)s * kW : (size_t)sld(a.abase + s);
    const double* __restrict__ vp = a.aval + vb * kSliceRows + (size_t)threadIdx.x * kRpt;
    const int* __restrict__ off = a.aoff + (size_t)s * kAMax;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    const double* __restrict__ xr = a.p + (size_t)a.c0 * a.pcs + row;  // column c0 + c: x of column row + off at xr[c * pcs + off]
    double sum[kR][kRpt];
#pragma unroll
    for (int c = 0; c < kR; c++)
#pragma unroll
        for (int i = 0; i < kRpt; i++) sum[c][i] = 0.0;
    bool tri = false;
    // (four columns only: with two the plan's registers cost the kernel a wave
    // per SIMD, 200^3 1.20x the sequential solves against 1.23x without it)
    constexpr bool kTri = kW == 3 * kTriples && kR >= 4;
    if constexpr (kTri) {
        tri = all && a.tri;
#pragma unroll
        for (int g = 0; g < kTriples; g++) {
            const int o0 = sld(off + 3 * g);
            tri = tri && sld(off + 3 * g + 1) == o0 + 1 && sld(off + 3 * g + 2) == o0 + 2;
        }
    }
    if (tri) {  // (block-uniform)
        if constexpr (kTri) {
            if (a.nt)
                spmm_a_triples<kR, true>(a, vp, off, xr, sum);
            else
                spmm_a_triples<kR, false>(a, vp, off, xr, sum);
        }
    } else if (all) {
        if (a.nt)
            spmm_a_slots<kW, kR, true, true>(a, vp, off, wdt, xr, act, sum);
        else
            spmm_a_slots<kW, kR, false, true>(a, vp, off, wdt, xr, act, sum);
    } else {
        spmm_a_slots<kW, kR, false, false>(a, vp, off, wdt, xr, act, sum);
    }
    spmm_rows_out<kR>(a, prologue, s, row, act, sum);
}

// ---------------------------------------------------------------------------
// SpMM over SELL-512 (int32 columns; matrices without an A image): k_spmv_sell's
// loop, x gathered from p_c. Padding slots (column -1, value 0) add +0.
// ---------------------------------------------------------------------------
template <int kR>
__global__ __launch_bounds__(kBlock) void k_batch_spmm_sell(BatchArgs a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    bool act[kR], all;
    if (!active_cols<kR>(a, act, all)) return;
    const size_t base = (size_t)sld(a.slice_base + s) * kSliceRows + (size_t)threadIdx.x * kRpt;
    const int w = (int)(sld(a.slice_base + s + 1) - sld(a.slice_base + s));
    const double* __restrict__ vp = a.vals + base;
    const int* __restrict__ cp = a.cols + base;
    const double* __restrict__ x0 = a.p + ((long long)a.c0 * a.pcs + a.xsell);
    double sum[kR][kRpt];
#pragma unroll
    for (int c = 0; c < kR; c++)
#pragma unroll
        for (int i = 0; i < kRpt; i++) sum[c][i] = 0.0;
#pragma unroll 3
    for (int j = 0; j < w; j++) {
        typedef int i2v __attribute__((ext_vector_type(2)));
        const i2v ct = *reinterpret_cast<const i2v*>(cp + (size_t)j * kSliceRows);
        const int col[kRpt] = {ct.x, ct.y};
        const Rows v = ld(vp + (size_t)j * kSliceRows);
#pragma unroll
        for (int c = 0; c < kR; c++) {
            if (!act[c]) continue;  // (block-uniform)
            const double* __restrict__ x = x0 + (size_t)c * a.pcs;
#pragma unroll
            for (int i = 0; i < kRpt; i++) {
                const double xv = (col[i] >= 0) ? x[col[i]] : 0.0;
                sum[c][i] = sum[c][i] + v.v[i] * xv;
            }
        }
    }
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    spmm_rows_out<kR>(a, prologue, s, row, act, sum);
}

// ---------------------------------------------------------------------------
// prologue: r = b + (-1)*Ap                         (HPCCG.cpp:352)
// loop:     x = x + alpha*p; r = r + (-alpha)*Ap    (HPCCG.cpp:382-384)
// then the r.r slice partial (k_update's expressions), per running column.
// ---------------------------------------------------------------------------
template <int kR>
__global__ __launch_bounds__(kBlock) void k_batch_update(BatchArgs a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        if (c >= a.nrhs) break;
        if (!prologue && !a.st[c].run) continue;  // (block-uniform)
        double* __restrict__ rc = a.r + (size_t)c * a.pcs;
        const Rows apv = ld(a.Ap + (size_t)c * a.vcs + row);
        Rows rn;
        if (prologue) {
            const Rows bv = ld(a.b + (size_t)c * a.vcs + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) rn.v[i] = bv.v[i] + (-1.0) * apv.v[i];
        } else {
            const double alpha = a.st[c].alpha;
            const Rows rv = ld(rc + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) rn.v[i] = rv.v[i] + (-alpha) * apv.v[i];
            double* __restrict__ xc = a.x + (size_t)c * a.vcs;
            const Rows xv = ld(xc + row);
            const Rows pv = ld(a.p + (size_t)c * a.pcs + row);
            Rows xn;
#pragma unroll
            for (int i = 0; i < kRpt; i++) xn.v[i] = xv.v[i] + alpha * pv.v[i];
            st_rows(xc, row, a.n, xn);
        }
        st_rows(rc, row, a.n, rn);
        double d = 0.0;
#pragma unroll
        for (int i = 0; i < kRpt; i++)
            if (row + i < a.n) d += rn.v[i] * rn.v[i];
        const double bs = block_sum<kBlock>(d);
        if (threadIdx.x == 0) slice_partials(a, kDotRR, c)[s] = bs;
        __syncthreads();  // block_sum's LDS words are free for the next column
    }
}

// ---------------------------------------------------------------------------
// One block per column: the dot's two upper levels (finalize_groups' and
// k_finalize's shapes: a 64-lane butterfly per group of 64 slice partials,
// top_sum_wave over the group sums), then the column's scalars.
//   p.Ap: alpha = rtrans / p.Ap                       (HPCCG.cpp:381-382)
//   r.r of iteration k: hist[k]; oldrtrans, rtrans, beta for iteration k + 1
//         and its loop test k + 1 < max_iter && normr > tol, normr being the
//         value iteration k computed, sqrt(r_{k-1}.r_{k-1}) (HPCCG.cpp:358,
//         as cg_run restates it; sqrt(r_0.r_0) for k + 1 = 1).
// ---------------------------------------------------------------------------
constexpr int kFinThreads = 1024;
constexpr int kFinLds = 2048;  // group sums kept in LDS up to 128 K slices

// The column's scalars once a dot's total is known (one lane).
__device__ __forceinline__ void advance_column(const BatchArgs& a, ColState* st, int c, int which, double tot)
{
    if (which == kDotPAP) {
        st->pap = tot;
        st->alpha = st->rtrans / tot;
        return;
    }
    const int k = st->k;
    const double old = st->rtrans;  // r_{k-1}.r_{k-1} (k >= 1)
    a.hist[(size_t)c * a.hstride + k] = tot;
    st->oldrtrans = old;
    st->rtrans = tot;
    st->beta = (k == 0) ? 0.0 : tot / old;
    st->k = k + 1;
    const bool run = k + 1 < a.max_iter && sqrt(k == 0 ? tot : old) > a.tol;
    if (!run) {
        st->run = 0;
        st->niters = k;
        atomicAdd(a.ended, 1);
    }
}

// local (a member of an in-process group): the total is this member's part of
// the dot; it is stored in tot[which][c] and the state is left to
// k_batch_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_batch_finalize(BatchArgs a, int which, int local)
{
    __shared__ double gs[kFinLds];
    const int c = blockIdx.x;
    ColState* const st = a.st + c;
    if (!st->run) return;  // (block-uniform) a frozen column keeps its state
    const int ng = a.ng;
    const bool in_lds = ng <= kFinLds;
    const double* const sp = slice_partials(a, which, c);
    double* const gp = a.gsum + ((size_t)which * a.cap + c) * (size_t)ng;
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int kWaves = kFinThreads / kWave;
    constexpr int kB = 4;  // groups per wave per round, their loads issued before the sums
    for (int g0 = threadIdx.x / kWave; g0 < ng; g0 += kWaves * kB) {
        double v[kB];
#pragma unroll
        for (int b = 0; b < kB; b++) {
            const int g = g0 + b * kWaves;
            const int i = g * kGroup + lane;
            v[b] = (g < ng && i < a.nslices) ? sp[i] : 0.0;
        }
#pragma unroll
        for (int b = 0; b < kB; b++) {
            const int g = g0 + b * kWaves;
            const double w = wave_sum(v[b]);
            if (lane == 0 && g < ng) {
                if (in_lds)
                    gs[g] = w;
                else
                    gp[g] = w;
            }
        }
    }
    if (!in_lds) __threadfence_block();
    __syncthreads();  // group sums written by this block
    if (threadIdx.x >= kWave) return;
    const double tot = in_lds ? top_sum_wave([&](int i) { return gs[i]; }, ng, lane)
                              : top_sum_wave([gp](int i) { return gp[i]; }, ng, lane);
    if (lane != 0) return;
    if (local) {
        a.tot[(size_t)which * a.cap + c] = tot;
        return;
    }
    advance_column(a, st, c, which, tot);
}

// ---------------------------------------------------------------------------
// In-process group: one thread per column on member 0's stream, after every
// member's local finalize. The global dot is the members' local totals added
// in rank order from 0.0 (k_group_sum's sum in hpccg_kernels.hip); the column's
// state advances as in k_batch_finalize and is stored into every member's
// state array (peer pointers across devices), so all members freeze a column
// together. hist and the "columns ended" word are member 0's (a: its args).
// ---------------------------------------------------------------------------
constexpr int kMaxMembers = kMaxGroupRanks;

struct GroupTotals {
    int nranks;
    int cap[kMaxMembers];            // stride of member r's totals
    const double* tot[kMaxMembers];  // member r's [2][cap] local totals
    ColState* st[kMaxMembers];       // member r's column states
};

__global__ void k_batch_group_sum(BatchArgs a, GroupTotals g, int which)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nrhs) return;
    ColState s = a.st[c];
    if (!s.run) return;  // frozen on every member
    double v = 0.0;
    for (int r = 0; r < g.nranks; r++) v += g.tot[r][(size_t)which * g.cap[r] + c];
    advance_column(a, &s, c, which, v);
    for (int r = 0; r < g.nranks; r++) g.st[r][c] = s;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return hpccg_hip_internal_set_error(code, buf);
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? HPCCG_HIP_ENOMEM : HPCCG_HIP_EHIP,         \
                        "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);   \
    } while (0)

#define TRY(expr)                     \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != 0) return rc_;     \
    } while (0)

constexpr int kCheckEvery = 32;  // iterations between two reads of the "columns ended" word

struct Workspace {
    MatrixView v;
    int cap = 0;  // columns
    long long pcs = 0, vcs = 0;
    double *pbuf = nullptr, *rbuf = nullptr, *Ap = nullptr, *x = nullptr, *b = nullptr;
    double *partial = nullptr, *gsum = nullptr;
    long long p0 = 0;       // local row 0 inside a p / r column (guard zone + the padded ghost_lo rows)
    double* tot = nullptr;  // [2][cap] local dot totals (a group member)
    hipEvent_t evr = nullptr, evs = nullptr;  // group: this member's stream is ready | member 0: the sum is done
    ColState* st = nullptr;
    int* ended = nullptr;
    double* hist = nullptr;
    long long hstride = 0;
    int* h_ended = nullptr;  // pinned
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    long long bytes = 0;
    std::vector<std::vector<double>> trace;  // per column of the last batch solve
};

std::mutex g_mu;
std::map<const hpccg_hip_matrix*, Workspace*> g_ws;

void free_device(Workspace* w)
{
    if (w->v.stream) (void)hipStreamSynchronize(w->v.stream);
    for (void* q : {(void*)w->pbuf, (void*)w->rbuf, (void*)w->Ap, (void*)w->x, (void*)w->b, (void*)w->partial,
                    (void*)w->gsum, (void*)w->st, (void*)w->ended, (void*)w->hist, (void*)w->tot})
        if (q) (void)hipFree(q);
    w->pbuf = w->rbuf = w->Ap = w->x = w->b = w->partial = w->gsum = w->hist = w->tot = nullptr;
    w->st = nullptr;
    w->ended = nullptr;
    w->cap = 0;
    w->hstride = 0;
    w->bytes = 0;
}

void drop_workspace(const hpccg_hip_matrix* M)
{
    Workspace* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_ws.find(M);
        if (it == g_ws.end()) return;
        w = it->second;
        g_ws.erase(it);
    }
    (void)hipSetDevice(w->v.device);
    free_device(w);
    if (w->h_ended) (void)hipHostFree(w->h_ended);
    if (w->ev0) (void)hipEventDestroy(w->ev0);
    if (w->ev1) (void)hipEventDestroy(w->ev1);
    if (w->evr) (void)hipEventDestroy(w->evr);
    if (w->evs) (void)hipEventDestroy(w->evs);
    delete w;
}

// the destroy hook (ctx: the matrix, the workspace's key; a no-op once released)
void on_matrix_destroy(void* ctx) { drop_workspace(static_cast<const hpccg_hip_matrix*>(ctx)); }

Workspace* find_workspace(const hpccg_hip_matrix* M)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ws.find(M);
    return it == g_ws.end() ? nullptr : it->second;
}

template <class T>
int alloc_zero(Workspace* w, T** p, size_t count)
{
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), bytes));
    HIP_TRY(hipMemsetAsync(*p, 0, bytes, w->v.stream));
    w->bytes += (long long)bytes;
    return 0;
}

// The matrix's workspace record with room for nrhs columns (ncols 0: the record
// only) and a history of max_iter + 1 entries per column.
int get_workspace(hpccg_hip_matrix* M, const MatrixView& v, int ncols, int max_iter, Workspace** out)
{
    Workspace* w = find_workspace(M);
    if (!w) {
        w = new Workspace;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            g_ws[M] = w;
        }
        w->v = v;
        const int rc = hpccg_hip_internal_on_destroy(M, on_matrix_destroy, M);
        if (rc) {
            drop_workspace(M);
            return rc;
        }
    }
    w->v = v;
    *out = w;
    if (ncols <= 0) return 0;
    HIP_TRY(hipSetDevice(v.device));
    if (!w->h_ended) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w->h_ended), sizeof(int), hipHostMallocDefault));
    if (!w->ev0) HIP_TRY(hipEventCreate(&w->ev0));
    if (!w->ev1) HIP_TRY(hipEventCreate(&w->ev1));
    if (v.in_group && !w->evr) HIP_TRY(hipEventCreateWithFlags(&w->evr, hipEventDisableTiming));
    if (v.in_group && !w->evs) HIP_TRY(hipEventCreateWithFlags(&w->evs, hipEventDisableTiming));
    const long long hneed = (long long)max_iter + 1;
    if (ncols <= w->cap && hneed <= w->hstride) return 0;
    const int cap = std::max(ncols, w->cap);
    const long long hstride = std::max(hneed, w->hstride);
    free_device(w);
    const size_t npad = (size_t)v.npad;
    const size_t ng = (size_t)(v.nslices + kGroup - 1) / kGroup;
    // a p column: [guard | ghost_lo (padded) | local rows (padded) | ghost_hi's spill (padded) | guard].
    // The ghost_hi rows start at local row n (where the single solve's p has
    // them): inside the last slice's padding rows and, past npad, in ghi_pad.
    // glo_pad is whole slices, so local row 0 keeps the buffer's alignment.
    const size_t glo_pad = ((size_t)v.ghost_lo + kSliceRows - 1) / kSliceRows * kSliceRows;
    const size_t ghi_pad = v.ghost_hi ? ((size_t)v.ghost_hi + 2 + kSliceRows - 1) / kSliceRows * kSliceRows : 0;
    w->p0 = (long long)((size_t)v.guard_rows + glo_pad);
    w->pcs = (long long)(npad + glo_pad + ghi_pad + 2 * (size_t)v.guard_rows);
    w->vcs = (long long)npad;
    // zeroed: the guard zones and the rows past n of p and r are read (holes,
    // full-width loads) and never stored by a kernel (p's ghost rows: by the
    // group's halo copies only)
    int rc = alloc_zero(w, &w->pbuf, (size_t)w->pcs * cap);
    if (!rc) rc = alloc_zero(w, &w->rbuf, (size_t)w->pcs * cap);
    if (!rc) rc = alloc_zero(w, &w->Ap, npad * cap);
    if (!rc) rc = alloc_zero(w, &w->x, npad * cap);
    if (!rc) rc = alloc_zero(w, &w->b, npad * cap);
    if (!rc) rc = alloc_zero(w, &w->partial, 2 * (size_t)cap * std::max(v.nslices, 1));
    if (!rc) rc = alloc_zero(w, &w->gsum, 2 * (size_t)cap * std::max<size_t>(ng, 1));
    if (!rc) rc = alloc_zero(w, &w->st, (size_t)cap);
    if (!rc && v.in_group) rc = alloc_zero(w, &w->tot, 2 * (size_t)cap);
    if (!rc) rc = alloc_zero(w, &w->ended, 1);
    if (!rc) rc = alloc_zero(w, &w->hist, (size_t)cap * (size_t)hstride);
    if (rc) {
        free_device(w);
        return rc;
    }
    w->cap = cap;
    w->hstride = hstride;
    return 0;
}

// What the batch runs on: one rank, no halo (group1: also the one member of a
// one-rank in-process group, which is that).
int check_matrix(hpccg_hip_matrix* M, MatrixView* v, bool group1 = false)
{
    TRY(hpccg_hip_internal_view(M, v));
    if (v->in_group && !(group1 && v->nranks == 1)) return fail(HPCCG_HIP_EINVAL, "batch: the matrix is a member of an in-process group (one rank only)");
    if (v->nranks > 1) return fail(HPCCG_HIP_EINVAL, "batch: the matrix belongs to a communicator of %d ranks (one rank only)", v->nranks);
    if (v->ghost_lo || v->ghost_hi) return fail(HPCCG_HIP_EINVAL, "batch: the matrix has halo rows (one rank only)");
    if (!v->has_a && !v->has_sell) return fail(HPCCG_HIP_EINVAL, "batch: the matrix holds no device image");
    return 0;
}

BatchArgs make_args(const Workspace* w, int nrhs, int max_iter, double tol)
{
    const MatrixView& v = w->v;
    BatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = v.n;
    a.nslices = v.nslices;
    a.grid = v.grid;
    a.nrhs = nrhs;
    a.cap = w->cap;
    a.ng = (v.nslices + kGroup - 1) / kGroup;
    a.max_iter = max_iter;
    a.tol = tol;
    a.nt = v.nt;
    a.a_width = v.a_width;
    a.tri = std::getenv("HPCCG_BATCH_NO_TRIPLES") ? 0 : 1;  // diagnostics: A/B of the x-triple plan
    a.p = w->pbuf + w->p0;
    a.r = w->rbuf + w->p0;
    a.xsell = v.sell_col_base;
    a.tot = w->tot;
    a.Ap = w->Ap;
    a.x = w->x;
    a.b = w->b;
    a.pcs = w->pcs;
    a.vcs = w->vcs;
    a.partial = w->partial;
    a.gsum = w->gsum;
    a.st = w->st;
    a.hist = w->hist;
    a.hstride = w->hstride;
    a.ended = w->ended;
    a.aval = v.aval;
    a.aoff = v.aoff;
    a.abase = v.abase;
    a.slice_base = v.slice_base;
    a.cols = v.cols;
    a.vals = v.vals;
    return a;
}

// Columns [c0, c0 + kR) per launch: fours, a remainder of three as a four with
// one idle column (one pass over the matrix, not two), of one or two as a two.
template <class F>
void for_chunks(int nrhs, F f)
{
    int c0 = 0;
    while (nrhs - c0 >= 3) {
        f(c0, 4);
        c0 += 4;
    }
    if (c0 < nrhs) f(c0, 2);
}

void launch_spmm(const Workspace* w, BatchArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a) {
            if (R == 4)
                hipLaunchKernelGGL(k_batch_spmm_sell<4>, g, b, 0, s, a, prologue);
            else
                hipLaunchKernelGGL(k_batch_spmm_sell<2>, g, b, 0, s, a, prologue);
            return;
        }
#define HPCCG_BATCH_A(W)                                                               \
    do {                                                                               \
        if (R == 4)                                                                    \
            hipLaunchKernelGGL((k_batch_spmm_a<W, 4>), g, b, 0, s, a, prologue);       \
        else                                                                           \
            hipLaunchKernelGGL((k_batch_spmm_a<W, 2>), g, b, 0, s, a, prologue);       \
    } while (0)
        if (a.a_width == 27 && R == 4 && a.nt)
            hipLaunchKernelGGL((k_batch_spmm_a<27, 4, 5>), g, b, 0, s, a, prologue);
        else if (a.a_width == 27)
            HPCCG_BATCH_A(27);
        else if (a.a_width == 7)
            HPCCG_BATCH_A(7);
        else
            HPCCG_BATCH_A(0);
#undef HPCCG_BATCH_A
    });
}

void launch_p(const Workspace* w, BatchArgs a, bool prologue)
{
    for_chunks(a.nrhs, [&](int c0, int R) {
        a.c0 = c0;
        if (R == 4)
            hipLaunchKernelGGL(k_batch_p<4>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
        else
            hipLaunchKernelGGL(k_batch_p<2>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
    });
}

void launch_update(const Workspace* w, BatchArgs a, bool prologue)
{
    for_chunks(a.nrhs, [&](int c0, int R) {
        a.c0 = c0;
        if (R == 4)
            hipLaunchKernelGGL(k_batch_update<4>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
        else
            hipLaunchKernelGGL(k_batch_update<2>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
    });
}

void launch_finalize(const Workspace* w, const BatchArgs& a, int which, int local = 0)
{
    hipLaunchKernelGGL(k_batch_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, local);
}

// Columns between the caller's column-major array and the workspace (kind:
// host or device on the caller's side), stream-ordered.
int copy_cols(const Workspace* w, double* dst, long long ldd, const double* src, long long lds, int nrhs,
              hipMemcpyKind kind)
{
    for (int c = 0; c < nrhs; c++)
        HIP_TRY(hipMemcpyAsync(dst + (size_t)c * (size_t)ldd, src + (size_t)c * (size_t)lds,
                               sizeof(double) * (size_t)w->v.n, kind, w->v.stream));
    return 0;
}

int read_results(Workspace* w, int nrhs, int* niters, double* normr, double* wall);

// The batch CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    hipStream_t s = w->v.stream;
    const BatchArgs a = make_args(w, nrhs, max_iter, tol);
    HIP_TRY(hipEventRecord(w->ev0, s));
    hipLaunchKernelGGL(k_batch_init, dim3((nrhs + 63) / 64), dim3(64), 0, s, a);
    launch_p(w, a, true);
    launch_spmm(w, a, true);
    launch_update(w, a, true);
    launch_finalize(w, a, kDotRR);
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < max_iter; k++) {
        launch_p(w, a, false);
        launch_spmm(w, a, false);
        launch_finalize(w, a, kDotPAP);
        launch_update(w, a, false);
        launch_finalize(w, a, kDotRR);
        if (k % kCheckEvery == 0 && k + 1 < max_iter) {
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(w->h_ended, w->ended, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (*w->h_ended >= nrhs) break;  // later launches would be no-ops for every column
        }
    }
    HIP_TRY(hipGetLastError());
    return read_results(w, nrhs, niters, normr, wall);
}

// The end of a batch CG on w's stream (a group: member 0's, whose last launch
// followed every member's): its wall time, the columns' states and traces.
int read_results(Workspace* w, int nrhs, int* niters, double* normr, double* wall)
{
    hipStream_t s = w->v.stream;
    HIP_TRY(hipEventRecord(w->ev1, s));
    std::vector<ColState> st(nrhs);
    std::vector<double> hist((size_t)nrhs * (size_t)w->hstride);
    HIP_TRY(hipMemcpyAsync(st.data(), w->st, sizeof(ColState) * nrhs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(hist.data(), w->hist, sizeof(double) * hist.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, w->ev0, w->ev1));
    if (wall) *wall = 1e-3 * ms;
    w->trace.assign(nrhs, {});
    for (int c = 0; c < nrhs; c++) {
        // a column still running when the launches ran out did max_iter - 1 iterations
        const int it = st[c].run ? st[c].k - 1 : st[c].niters;
        const double* h = hist.data() + (size_t)c * (size_t)w->hstride;
        // normr after iteration k is sqrt(r_{k-1}.r_{k-1}) (HPCCG.cpp:371): the single solve's trace
        std::vector<double>& tr = w->trace[c];
        tr.assign(it + 1, 0.0);
        tr[0] = std::sqrt(h[0]);
        for (int k = 1; k <= it; k++) tr[k] = std::sqrt(h[k - 1]);
        niters[c] = it;
        normr[c] = tr[it];
    }
    return 0;
}

int check_solve_args(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                     int max_iter, int* niters, double* normr)
{
    if (!M || !B || !X || !niters || !normr) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "batch: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "batch: max_iter %d is negative", max_iter);
    (void)ldb;
    (void)ldx;
    return 0;
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx, int max_iter,
                 double tol, int* niters, double* normr, double* times, bool host, bool group1 = false)
{
    TRY(check_solve_args(M, nrhs, B, ldb, X, ldx, max_iter, niters, normr));
    MatrixView v;
    TRY(check_matrix(M, &v, group1));
    if (ldb < v.n || ldx < v.n)
        return fail(HPCCG_HIP_EINVAL, "batch: leading dimensions %lld, %lld below the %d rows", ldb, ldx, v.n);
    if (times) std::fill(times, times + 7, 0.0);
    Workspace* w = nullptr;
    if (nrhs == 1 || v.n == 0) {  // the single solve itself
        TRY(get_workspace(M, v, 0, 0, &w));
        w->trace.assign(nrhs, {});
        for (int c = 0; c < nrhs; c++) {
            double t1[7] = {0, 0, 0, 0, 0, 0, 0};
            if (host)
                TRY(hpccg_hip_solve(M, B + c * ldb, X + c * ldx, max_iter, tol, niters + c, normr + c, t1, 0));
            else
                TRY(hpccg_hip_solve_device(M, B + c * ldb, X + c * ldx, max_iter, tol, niters + c, normr + c, t1, 0));
            if (times) {
                times[0] += t1[0];
                times[6] += t1[6];
            }
            std::vector<double>& tr = w->trace[c];
            tr.assign((size_t)niters[c] + 1, 0.0);
            const int got = hpccg_hip_last_trace(M, tr.data(), (int)tr.size());
            tr.resize((size_t)std::max(got, 0));
        }
        return 0;
    }
    if (max_iter < 1) max_iter = 1;
    TRY(get_workspace(M, v, nrhs, max_iter, &w));
    const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const hipMemcpyKind out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const auto t0 = std::chrono::steady_clock::now();
    TRY(copy_cols(w, w->b, w->vcs, B, ldb, nrhs, in));
    TRY(copy_cols(w, w->x, w->vcs, X, ldx, nrhs, in));
    if (host) HIP_TRY(hipStreamSynchronize(v.stream));
    const auto t1 = std::chrono::steady_clock::now();
    double wall = 0.0;
    TRY(run_cg(w, nrhs, max_iter, tol, niters, normr, &wall));
    const auto t2 = std::chrono::steady_clock::now();
    TRY(copy_cols(w, X, ldx, w->x, w->vcs, nrhs, out));
    HIP_TRY(hipStreamSynchronize(v.stream));
    const auto t3 = std::chrono::steady_clock::now();
    if (times) {
        times[0] = wall;
        if (host) times[6] = std::chrono::duration<double>((t1 - t0) + (t3 - t2)).count();
    }
    return 0;
}

// Y(:,c) = A X(:,c) on one rank.
int sparsemv_one(hpccg_hip_matrix* M, int nrhs, const double* X_dev, long long ldx, double* Y_dev, long long ldy,
                 bool group1)
{
    if (!M || !X_dev || !Y_dev) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "batch: nrhs %d (at least 1)", nrhs);
    MatrixView v;
    TRY(check_matrix(M, &v, group1));
    if (ldx < v.n || ldy < v.n)
        return fail(HPCCG_HIP_EINVAL, "batch: leading dimensions %lld, %lld below the %d rows", ldx, ldy, v.n);
    if (v.n == 0) return 0;
    if (nrhs == 1) return hpccg_hip_sparsemv(M, X_dev, Y_dev);
    Workspace* w = nullptr;
    TRY(get_workspace(M, v, nrhs, 1, &w));
    // x into the guarded p columns, Ap = A p, Ap out
    BatchArgs a = make_args(w, nrhs, 1, 0.0);
    a.force = 1;
    TRY(copy_cols(w, a.p, w->pcs, X_dev, ldx, nrhs, hipMemcpyDeviceToDevice));
    launch_spmm(w, a, true);
    HIP_TRY(hipGetLastError());
    TRY(copy_cols(w, Y_dev, ldy, w->Ap, w->vcs, nrhs, hipMemcpyDeviceToDevice));
    HIP_TRY(hipStreamSynchronize(v.stream));
    return 0;
}

// ---------------------------------------------------------------------------
// In-process rank group (include/hpccg_hip_batch_group.h): member r is rank r
// of a z-slab job; every member runs the batch kernels on its own stream with
// its own workspace, the ghost planes of every column's p move by copies
// between the members, and the two dots are summed over the members in rank
// order by k_batch_group_sum on member 0's stream.
// ---------------------------------------------------------------------------
struct Group {
    int P = 0;
    std::vector<MatrixView> v;
    std::vector<Workspace*> w;
    std::vector<BatchArgs> a;
};

// The whole group in rank order, z-slab plan, a device image on every member.
// Reads the matrices' records only: no device work.
int check_group(hpccg_hip_matrix* const* Ms, int nranks, Group* G)
{
    G->P = nranks;
    G->v.resize(nranks);
    for (int r = 0; r < nranks; r++) {
        if (!Ms[r]) return fail(HPCCG_HIP_EINVAL, "group batch: Ms[%d] is NULL", r);
        TRY(hpccg_hip_internal_view(Ms[r], &G->v[r]));
        const MatrixView& v = G->v[r];
        if (v.nranks != nranks || v.rank != r || (nranks > 1 && !v.in_group))
            return fail(HPCCG_HIP_EINVAL, "group batch: Ms[%d] is not rank %d of a %d-rank in-process group", r, r,
                        nranks);
        if (nranks > 1 && v.group_id != G->v[0].group_id)
            return fail(HPCCG_HIP_EINVAL, "group batch: Ms[%d] is a member of another group than Ms[0]", r);
    }
    if (nranks == 1) return 0;  // (the single-rank batch checks its matrix itself)
    for (int r = 0; r < nranks; r++) {
        const MatrixView& v = G->v[r];
        if (v.general)
            return fail(HPCCG_HIP_EPLAN, "group batch: member %d uses the gather plan (z-slab plan members only)", r);
        // the halo copies below rely on these (hpccg_slab_plan made them so)
        const int lo_max = r > 0 ? G->v[r - 1].n : 0, hi_max = r < nranks - 1 ? G->v[r + 1].n : 0;
        if (v.ghost_lo < 0 || v.ghost_hi < 0 || v.ghost_lo > lo_max || v.ghost_hi > hi_max)
            return fail(HPCCG_HIP_EPLAN, "group batch: member %d's ghost rows (%d, %d) are not its neighbours' rows", r,
                        v.ghost_lo, v.ghost_hi);
        if (v.n <= 0) return fail(HPCCG_HIP_EINVAL, "group batch: member %d has no rows", r);
        if (!v.has_a && !v.has_sell) return fail(HPCCG_HIP_EINVAL, "group batch: member %d holds no device image", r);
    }
    return 0;
}

int check_group_lds(const Group& G, const long long* l0, const long long* l1, const char* what)
{
    for (int r = 0; r < G.P; r++)
        if (l0[r] < G.v[r].n || l1[r] < G.v[r].n)
            return fail(HPCCG_HIP_EINVAL, "group batch: member %d's leading dimensions (%s) %lld, %lld below its %d rows",
                        r, what, l0[r], l1[r], G.v[r].n);
    return 0;
}

int use(const Group& G, int r)
{
    HIP_TRY(hipSetDevice(G.v[r].device));
    return 0;
}

int group_workspaces(hpccg_hip_matrix* const* Ms, Group* G, int nrhs, int max_iter, double tol)
{
    G->w.assign(G->P, nullptr);
    G->a.resize(G->P);
    for (int r = 0; r < G->P; r++) {
        TRY(get_workspace(Ms[r], G->v[r], nrhs, max_iter, &G->w[r]));
        G->a[r] = make_args(G->w[r], nrhs, max_iter, tol);
    }
    return 0;
}

// rows of one member's column into another's (one device: a plain copy)
int member_copy(const MatrixView& dv, double* dst, const MatrixView& sv, const double* src, size_t n)
{
    if (dv.device == sv.device)
        HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToDevice, dv.stream));
    else
        HIP_TRY(hipMemcpyPeerAsync(dst, dv.device, src, sv.device, sizeof(double) * n, dv.stream));
    return 0;
}

// The halo of every column's p (group_halo in hpccg_solver.cpp, per column):
// member r's ghost_lo rows are member r - 1's last rows, its ghost_hi rows
// (from local row n) member r + 1's first, copied on r's stream once the
// neighbour's stream has stored them (its event). Frozen columns' planes are
// copied too (their p no longer changes: harmless).
// p is one buffer per column, not a ring. A neighbour cannot overwrite its p
// before these copies have read it: its next k_batch_p follows the group sum of
// p.Ap (in the prologue: of r.r) on its stream, that sum waits for every
// member's SpMM, and each member's SpMM follows its copies on its own stream.
int group_halo(const Group& G, int nrhs)
{
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    for (int r = 0; r < G.P; r++) {
        const MatrixView& v = G.v[r];
        const BatchArgs& a = G.a[r];
        TRY(use(G, r));
        if (r > 0 && v.ghost_lo) {
            const BatchArgs& l = G.a[r - 1];
            HIP_TRY(hipStreamWaitEvent(v.stream, G.w[r - 1]->evr, 0));
            for (int c = 0; c < nrhs; c++)
                TRY(member_copy(v, a.p + (long long)c * a.pcs - v.ghost_lo, G.v[r - 1],
                                l.p + (long long)c * l.pcs + (l.n - v.ghost_lo), (size_t)v.ghost_lo));
        }
        if (r < G.P - 1 && v.ghost_hi) {
            const BatchArgs& u = G.a[r + 1];
            HIP_TRY(hipStreamWaitEvent(v.stream, G.w[r + 1]->evr, 0));
            for (int c = 0; c < nrhs; c++)
                TRY(member_copy(v, a.p + (long long)c * a.pcs + a.n, G.v[r + 1], u.p + (long long)c * u.pcs,
                                (size_t)v.ghost_hi));
        }
    }
    return 0;
}

// The global dot `which` of every running column and its state on every
// member: member 0's stream waits for every member's local finalize, runs
// k_batch_group_sum, and the other members' streams wait for it.
int group_sum(const Group& G, const GroupTotals& gt, int which, int nrhs)
{
    for (int r = 1; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    TRY(use(G, 0));
    hipStream_t s0 = G.v[0].stream;
    for (int r = 1; r < G.P; r++) HIP_TRY(hipStreamWaitEvent(s0, G.w[r]->evr, 0));
    hipLaunchKernelGGL(k_batch_group_sum, dim3((nrhs + 63) / 64), dim3(64), 0, s0, G.a[0], gt, which);
    HIP_TRY(hipEventRecord(G.w[0]->evs, s0));
    for (int r = 1; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipStreamWaitEvent(G.v[r].stream, G.w[0]->evs, 0));
    }
    return 0;
}

// The batch CG over the group on the columns staged in the members' b and x.
int group_run_cg(const Group& G, int nrhs, int max_iter, int* niters, double* normr, double* wall)
{
    GroupTotals gt;
    std::memset(&gt, 0, sizeof gt);
    gt.nranks = G.P;
    for (int r = 0; r < G.P; r++) {
        gt.cap[r] = G.w[r]->cap;
        gt.tot[r] = G.w[r]->tot;
        gt.st[r] = G.w[r]->st;
    }
    Workspace* w0 = G.w[0];
    TRY(use(G, 0));
    HIP_TRY(hipEventRecord(w0->ev0, G.v[0].stream));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        hipLaunchKernelGGL(k_batch_init, dim3((nrhs + 63) / 64), dim3(64), 0, G.v[r].stream, G.a[r]);
        launch_p(G.w[r], G.a[r], true);
    }
    TRY(group_halo(G, nrhs));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm(G.w[r], G.a[r], true);
        launch_update(G.w[r], G.a[r], true);
        launch_finalize(G.w[r], G.a[r], kDotRR, 1);
    }
    TRY(group_sum(G, gt, kDotRR, nrhs));
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < max_iter; k++) {
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_p(G.w[r], G.a[r], false);
        }
        TRY(group_halo(G, nrhs));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_spmm(G.w[r], G.a[r], false);
            launch_finalize(G.w[r], G.a[r], kDotPAP, 1);
        }
        TRY(group_sum(G, gt, kDotPAP, nrhs));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_update(G.w[r], G.a[r], false);
            launch_finalize(G.w[r], G.a[r], kDotRR, 1);
        }
        TRY(group_sum(G, gt, kDotRR, nrhs));
        if (k % kCheckEvery == 0 && k + 1 < max_iter) {
            HIP_TRY(hipGetLastError());
            TRY(use(G, 0));
            HIP_TRY(hipMemcpyAsync(w0->h_ended, w0->ended, sizeof(int), hipMemcpyDeviceToHost, G.v[0].stream));
            HIP_TRY(hipStreamSynchronize(G.v[0].stream));
            if (*w0->h_ended >= nrhs) break;  // every column is frozen on every member
        }
    }
    HIP_TRY(hipGetLastError());
    TRY(use(G, 0));
    TRY(read_results(w0, nrhs, niters, normr, wall));
    for (int r = 1; r < G.P; r++) {  // (the last sum's event was their streams' last wait)
        TRY(use(G, r));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    return 0;
}

int group_solve(hpccg_hip_matrix* const* Ms, const Group& G0, int nrhs, const double* const* B, const long long* ldb,
                double* const* X, const long long* ldx, int max_iter, double tol, int* niters, double* normr,
                double* times)
{
    Group G = G0;
    if (times) std::fill(times, times + 7, 0.0);
    if (nrhs == 1) {  // the group solve itself; its trace kept with member 0's record
        double t1[7] = {0, 0, 0, 0, 0, 0, 0};
        TRY(hpccg_hip_group_solve(Ms, G.P, B, X, max_iter, tol, niters, normr, t1));
        if (times) times[0] = t1[0];
        Workspace* w = nullptr;
        TRY(get_workspace(Ms[0], G.v[0], 0, 0, &w));
        w->trace.assign(1, {});
        std::vector<double>& tr = w->trace[0];
        tr.assign((size_t)niters[0] + 1, 0.0);
        const int got = hpccg_hip_last_trace(Ms[0], tr.data(), (int)tr.size());
        tr.resize((size_t)std::max(got, 0));
        return 0;
    }
    if (max_iter < 1) max_iter = 1;
    TRY(group_workspaces(Ms, &G, nrhs, max_iter, tol));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        TRY(copy_cols(G.w[r], G.w[r]->b, G.w[r]->vcs, B[r], ldb[r], nrhs, hipMemcpyDeviceToDevice));
        TRY(copy_cols(G.w[r], G.w[r]->x, G.w[r]->vcs, X[r], ldx[r], nrhs, hipMemcpyDeviceToDevice));
    }
    double wall = 0.0;
    TRY(group_run_cg(G, nrhs, max_iter, niters, normr, &wall));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        TRY(copy_cols(G.w[r], X[r], ldx[r], G.w[r]->x, G.w[r]->vcs, nrhs, hipMemcpyDeviceToDevice));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    if (times) times[0] = wall;
    return 0;
}

int group_sparsemv(hpccg_hip_matrix* const* Ms, const Group& G0, int nrhs, const double* const* X,
                   const long long* ldx, double* const* Y, const long long* ldy)
{
    Group G = G0;
    TRY(group_workspaces(Ms, &G, nrhs, 1, 0.0));
    // x into the local rows of the p columns, their halo, Ap = A p, Ap out
    for (int r = 0; r < G.P; r++) {
        G.a[r].force = 1;
        TRY(use(G, r));
        TRY(copy_cols(G.w[r], G.a[r].p, G.w[r]->pcs, X[r], ldx[r], nrhs, hipMemcpyDeviceToDevice));
    }
    TRY(group_halo(G, nrhs));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm(G.w[r], G.a[r], true);
        HIP_TRY(hipGetLastError());
        TRY(copy_cols(G.w[r], Y[r], ldy[r], G.w[r]->Ap, G.w[r]->vcs, nrhs, hipMemcpyDeviceToDevice));
    }
    // (every member's copies of its neighbours' rows are done before any
    // member's buffers may be reused by the next call)
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    return 0;
}

// f() with the caller's current device put back afterwards
template <class F>
int keep_device(F f)
{
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    const int rc = f();
    (void)hipSetDevice(cur);
    return rc;
}

int check_group_args(hpccg_hip_matrix* const* Ms, int nranks, int nrhs)
{
    if (!Ms) return fail(HPCCG_HIP_EINVAL, "group batch: Ms is NULL");
    if (nranks < 1 || nranks > kMaxMembers)
        return fail(HPCCG_HIP_EINVAL, "group batch: nranks %d (1 to %d members)", nranks, kMaxMembers);
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "group batch: nrhs %d (at least 1)", nrhs);
    return 0;
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_batch_abi_version(void) { return 1; }

int hpccg_hip_batch_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                 long long ldx, int max_iter, double tolerance, int* niters, double* normr,
                                 double* times)
{
    return solve_common(M, nrhs, B_dev, ldb, X_dev, ldx, max_iter, tolerance, niters, normr, times, false);
}

int hpccg_hip_batch_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                          int max_iter, double tolerance, int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B, ldb, X, ldx, max_iter, tolerance, niters, normr, times, true);
}

int hpccg_hip_batch_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    if (!M || !out) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    const Workspace* w = find_workspace(M);
    if (!w || col < 0 || col >= (int)w->trace.size())
        return fail(HPCCG_HIP_EINVAL, "batch: no trace of column %d (the last batch solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    const std::vector<double>& tr = w->trace[col];
    const int n = std::min<int>(std::max(cap, 0), (int)tr.size());
    for (int i = 0; i < n; i++) out[i] = tr[i];
    return n;
}

int hpccg_hip_batch_sparsemv(hpccg_hip_matrix* M, int nrhs, const double* X_dev, long long ldx, double* Y_dev,
                             long long ldy)
{
    return sparsemv_one(M, nrhs, X_dev, ldx, Y_dev, ldy, false);
}

int hpccg_hip_batch_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    drop_workspace(M);
    return 0;
}

int hpccg_hip_batch_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    const Workspace* w = find_workspace(M);
    *bytes = w ? w->bytes : 0;
    return 0;
}

int hpccg_hip_batch_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    std::lock_guard<std::mutex> lk(g_mu);
    *count = (int)g_ws.size();
    return 0;
}

// ---- include/hpccg_hip_batch_group.h ---------------------------------------
int hpccg_hip_group_batch_abi_version(void) { return 1; }

int hpccg_hip_group_batch_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                       const long long* ldb, double* const* X_dev, const long long* ldx, int max_iter,
                                       double tolerance, int* niters, double* normr, double* times)
{
    TRY(check_group_args(Ms, nranks, nrhs));
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "group batch: max_iter %d is negative", max_iter);
    if (!B_dev || !ldb || !X_dev || !ldx || !niters || !normr)
        return fail(HPCCG_HIP_EINVAL, "group batch: NULL argument (B_dev, ldb, X_dev, ldx, niters or normr)");
    for (int r = 0; r < nranks; r++)
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "group batch: B_dev[%d] or X_dev[%d] is NULL", r, r);
    Group G;
    TRY(check_group(Ms, nranks, &G));
    TRY(check_group_lds(G, ldb, ldx, "ldb, ldx"));
    return keep_device([&] {
        if (nranks == 1)
            return solve_common(Ms[0], nrhs, B_dev[0], ldb[0], X_dev[0], ldx[0], max_iter, tolerance, niters, normr,
                                times, false, true);
        return group_solve(Ms, G, nrhs, B_dev, ldb, X_dev, ldx, max_iter, tolerance, niters, normr, times);
    });
}

int hpccg_hip_group_batch_sparsemv(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* X_dev,
                                   const long long* ldx, double* const* Y_dev, const long long* ldy)
{
    TRY(check_group_args(Ms, nranks, nrhs));
    if (!X_dev || !ldx || !Y_dev || !ldy)
        return fail(HPCCG_HIP_EINVAL, "group batch: NULL argument (X_dev, ldx, Y_dev or ldy)");
    for (int r = 0; r < nranks; r++)
        if (!X_dev[r] || !Y_dev[r]) return fail(HPCCG_HIP_EINVAL, "group batch: X_dev[%d] or Y_dev[%d] is NULL", r, r);
    Group G;
    TRY(check_group(Ms, nranks, &G));
    TRY(check_group_lds(G, ldx, ldy, "ldx, ldy"));
    return keep_device([&] {
        if (nranks == 1) return sparsemv_one(Ms[0], nrhs, X_dev[0], ldx[0], Y_dev[0], ldy[0], true);
        return group_sparsemv(Ms, G, nrhs, X_dev, ldx, Y_dev, ldy);
    });
}

int hpccg_hip_group_batch_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    if (!Ms) return fail(HPCCG_HIP_EINVAL, "group batch: Ms is NULL");
    if (nranks < 1 || nranks > kMaxMembers)
        return fail(HPCCG_HIP_EINVAL, "group batch: nranks %d (1 to %d members)", nranks, kMaxMembers);
    if (!out) return fail(HPCCG_HIP_EINVAL, "group batch: out is NULL");
    Group G;
    TRY(check_group(Ms, nranks, &G));
    // one set of all-reduced scalars: kept with member 0's record
    return hpccg_hip_batch_last_trace(Ms[0], col, out, cap);
}

}  // extern "C"
