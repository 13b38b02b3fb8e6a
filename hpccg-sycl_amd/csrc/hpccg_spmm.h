// hpccg_spmm.h -- the fp64 SpMM loops shared by the units that stream the
// matrix's own fp64 image for several columns (hpccg_batch.hip,
// hpccg_pcg.hip, hpccg_pcg_group.hip, hpccg_poly.hip, hpccg_poly_group.hip,
// and hpccg_poly32.hip for the outer SpMM of an inexact image): the slot loop
// and the x-triple plan over SELL-512-A, the int32-column loop over SELL-512,
// and the two kernel bodies around them. hpccg_spmm32.h builds the same loops
// over an fp32 image on the ends policy defined here. A
// unit's __global__ entry points are thin wrappers over the bodies (their
// launch bounds and occupancy are the wrapper's); the bodies are templates on
// the unit's argument struct A, a ColArgs with
//   int tri;             width 27: slices whose offsets come in runs of three use the x-triple plan
//   const double* aval;  the SELL-512-A values
//   const double* vals;  the SELL-512 values
// and on an ends policy E (SpmmToAp by default): where column 0's x lives and
// what becomes of the row sums (hpccg_poly.hip's steps read z and apply the
// Chebyshev step in registers).
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include "hpccg_columns.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// ---------------------------------------------------------------------------
// SpMM over SELL-512-A: k_spmv_a's slot loop with kR running sums per row. A
// value slot pair is loaded once; column c's x is p_c at the slice's offsets
// (holes: 0.0 times a finite word of p_c's zeroed guard zone or a real
// neighbour). Per row and column the products are added in slot order with no
// contraction: the single kernel's row sum.
// ---------------------------------------------------------------------------
template <int kW, int kR, bool kNT, bool kAll, class A>
__device__ __forceinline__ void spmm_a_slots(const A& a, const double* __restrict__ vp, const int* __restrict__ off,
                                             int wdt, const double* __restrict__ xr, const bool (&act)[kR],
                                             double (&sum)[kR][kRpt])
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

template <int kR, bool kNT, class A>
__device__ __forceinline__ void spmm_a_triples(const A& a, const double* __restrict__ vp, const int* __restrict__ off,
                                               const double* __restrict__ xr, double (&sum)[kR][kRpt])
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

// The first and the last statement of each arm of a branch on a.nt. The two
// arms differ in the value loads' non-temporal hint alone, which is metadata:
// the optimiser takes their instructions for the same, hoists them from the
// top or sinks them from the bottom into one copy, and the hint is gone
// (without these statements the one- and two-column forms of widths 27 and 7
// have no non-temporal load left in the code object; 200^3 two columns: 5 %
// slower). An empty statement that differs between the arms, at
// both ends, keeps them two. tests/test_pcg_cpu.py counts the non-temporal
// loads in the code objects.
template <int kArm>
__device__ __forceinline__ void arm()
{
    asm volatile("; value loads, arm %0" ::"n"(kArm));
}

// The default ends of a body: x is p, the row sums go to Ap with the p.Ap
// slice partial (spmm_rows_out).
struct SpmmToAp {
    template <class A>
    static __device__ __forceinline__ const double* x(const A& a)
    {
        return a.p;
    }
    template <int kR, class A>
    static __device__ __forceinline__ void out(const A& a, bool prologue, int s, int row, const bool (&act)[kR],
                                               const double (&sum)[kR][kRpt])
    {
        spmm_rows_out<kR>(a, prologue, s, row, act, sum);
    }
};

// The body of a unit's SELL-512-A SpMM kernel<kW, kR> (one block per slice).
template <int kW, int kR, class A, class E = SpmmToAp>
__device__ __forceinline__ void spmm_a_body(const A& a, bool prologue)
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
    const double* __restrict__ xr = E::x(a) + (size_t)a.c0 * a.pcs + row;  // column c0 + c: x of column row + off at xr[c * pcs + off]
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
            if (a.nt) {
                arm<1>();
                spmm_a_triples<kR, true>(a, vp, off, xr, sum);
                arm<1>();
            } else {
                arm<0>();
                spmm_a_triples<kR, false>(a, vp, off, xr, sum);
                arm<0>();
            }
        }
    } else if (all) {
        if (a.nt) {
            arm<1>();
            spmm_a_slots<kW, kR, true, true>(a, vp, off, wdt, xr, act, sum);
            arm<1>();
        } else {
            arm<0>();
            spmm_a_slots<kW, kR, false, true>(a, vp, off, wdt, xr, act, sum);
            arm<0>();
        }
    } else {
        spmm_a_slots<kW, kR, false, false>(a, vp, off, wdt, xr, act, sum);
    }
    E::template out<kR>(a, prologue, s, row, act, sum);
}

// ---------------------------------------------------------------------------
// SpMM over SELL-512 (int32 columns; matrices without an A image): k_spmv_sell's
// loop, x gathered from p_c. Padding slots (column -1, value 0) add +0. The
// body of a unit's SELL-512 SpMM kernel<kR>.
// ---------------------------------------------------------------------------
template <int kR, class A, class E = SpmmToAp>
__device__ __forceinline__ void spmm_sell_body(const A& a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    bool act[kR], all;
    if (!active_cols<kR>(a, act, all)) return;
    const size_t base = (size_t)sld(a.slice_base + s) * kSliceRows + (size_t)threadIdx.x * kRpt;
    const int w = (int)(sld(a.slice_base + s + 1) - sld(a.slice_base + s));
    const double* __restrict__ vp = a.vals + base;
    const int* __restrict__ cp = a.cols + base;
    const double* __restrict__ x0 = E::x(a) + ((long long)a.c0 * a.pcs + a.xsell);
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
    E::template out<kR>(a, prologue, s, row, act, sum);
}

}  // namespace

}  // namespace hpccg
