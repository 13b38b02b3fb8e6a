// hpccg_spmm32.h -- the fp32 image of the matrix values and the fp64 SpMM loops
// over it, for the units that stream such an image for several columns
// (hpccg_mixed.hip, hpccg_poly32.hip, hpccg_poly32_group.hip).
//   device  the body of a unit's convert kernel; the slot loops over the image
//           (spmm32_a_slots, slot32_sell) and the two SpMM kernel bodies around
//           them (spmm32_a_body with the x-triple plan, spmm32_sell_body). A
//           unit's __global__ entry points are thin wrappers over the bodies;
//           the mixed unit keeps the frames of its two SpMM kernels (it has no
//           x-triple arm) and runs the slot loops from here.
//   host    Image32, the image's record in a unit's workspace, and
//           ensure_image32, its one builder.
// The image follows the image the matrix holds (SELL-512-A where it exists,
// else SELL-512), slice by slice with the same slot-row bases, so the offset
// tables / int32 columns are shared; inside a slice the slots are interleaved
// in pairs, slot pair (2q, 2q + 1) laid out so that thread t (rows 2t, 2t + 1)
// reads one float4
//   { v[2q][2t], v[2q][2t + 1], v[2q + 1][2t], v[2q + 1][2t + 1] }
// at (base + 2q) * 512 + 4t; an odd width's last slot is a plain [512 rows]
// run read 8 B per lane. Exactly 4 B per slot. A value is widened in the
// register; every product and sum is fp64, added in slot order with no
// contraction: the fp64 loops' row sum of the widened values.
// The bodies are templates on the unit's argument struct A, a ColArgs with
//   const float* img;  the fp32 values
// on kNT (the value loads are non-temporal: a template parameter of the
// kernel, chosen on the host -- as a branch inside the kernel the two arms
// differ in the hint alone, the optimiser merges them and the hint is lost) and
// on an ends policy E as hpccg_spmm.h's bodies are (SpmmToAp by default).
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include <cfloat>

#include "hpccg_columns.h"
#include "hpccg_spmm.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

template <bool kNT>
__device__ __forceinline__ f4v ld_f4(const float* __restrict__ p)
{
    if constexpr (kNT)
        return __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
    else
        return *reinterpret_cast<const f4v*>(p);
}

template <bool kNT>
__device__ __forceinline__ f2v ld_f2(const float* __restrict__ p)
{
    if constexpr (kNT)
        return __builtin_nontemporal_load(reinterpret_cast<const f2v*>(p));
    else
        return *reinterpret_cast<const f2v*>(p);
}

// ---------------------------------------------------------------------------
// fp64 image -> fp32 image, one block per slice (the body of a unit's convert
// kernel). width > 0: every slice has that many slots (base s * width); else
// slice s holds base_tab[s] .. base_tab[s + 1]. flags[0] counts the values with
// (double)(float)v != v, flags[1] those outside fp32 range (image not finite,
// or nonzero below FLT_MIN). Zero holes and padding slots are exact.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void convert32_body(const double* __restrict__ vals,
                                               const unsigned int* __restrict__ base_tab, int width,
                                               float* __restrict__ img, unsigned long long* flags)
{
    const int s = blockIdx.x;
    const int w = width > 0 ? width : (int)(base_tab[s + 1] - base_tab[s]);
    const size_t vb = (width > 0 ? (size_t)s * width : (size_t)base_tab[s]) * kSliceRows;
    const double* __restrict__ src = vals + vb + (size_t)threadIdx.x * kRpt;
    float* __restrict__ dst = img + vb;
    const int wp = w & ~1;  // slots in pairs
    unsigned int inexact = 0, range = 0;
    for (int j = 0; j < w; j++) {
        const Rows v = ld(src + (size_t)j * kSliceRows);
        f2v f;
        f.x = (float)v.v[0];
        f.y = (float)v.v[1];
#pragma unroll
        for (int i = 0; i < kRpt; i++) {
            const float fi = i ? f.y : f.x;
            if (!((double)fi == v.v[i])) inexact++;
            if (!isfinite(fi) || (v.v[i] != 0.0 && fabs(v.v[i]) < (double)FLT_MIN)) range++;
        }
        float* q = j < wp ? dst + (size_t)(j & ~1) * kSliceRows + (size_t)threadIdx.x * 4 + (j & 1) * 2
                          : dst + (size_t)j * kSliceRows + (size_t)threadIdx.x * 2;
        *reinterpret_cast<f2v*>(q) = f;
    }
    if (inexact) atomicAdd(flags, (unsigned long long)inexact);
    if (range) atomicAdd(flags + 1, (unsigned long long)range);
}

// One slot of the A image for every column: sum[c][i] = sum[c][i] +
// (double)v[i] * x_c[row + off + i], the fp64 loops' row-sum step.
template <int kR, bool kAll, class A>
__device__ __forceinline__ void slot32_a(const A& a, float v0, float v1, int oj, const double* __restrict__ xr,
                                         const bool (&act)[kR], double (&sum)[kR][kRpt])
{
    const double w0 = (double)v0, w1 = (double)v1;
#pragma unroll
    for (int c = 0; c < kR; c++) {
        if (kAll || act[c]) {
            const Rows xv = ld_u(xr + ((long long)c * a.pcs + oj));
            sum[c][0] = sum[c][0] + w0 * xv.v[0];
            sum[c][1] = sum[c][1] + w1 * xv.v[1];
        }
    }
}

// The slot loop over a slice of the fp32 SELL-512-A image: two slots per 16-B
// value load. Column c's x at the slice's offsets (holes: 0.0 times a finite
// word of the column's zeroed guard zone or a real neighbour).
template <int kW, int kR, bool kNT, bool kAll, class A>
__device__ __forceinline__ void spmm32_a_slots(const A& a, const float* __restrict__ base,
                                               const int* __restrict__ off, int wdt, const double* __restrict__ xr,
                                               const bool (&act)[kR], double (&sum)[kR][kRpt])
{
    const float* __restrict__ vp = base + (size_t)threadIdx.x * 4;
    const int np = wdt >> 1;
#pragma unroll kW > 0 ? kW / 2 : 2
    for (int q = 0; q < np; q++) {
        const f4v v = ld_f4<kNT>(vp + (size_t)(2 * q) * kSliceRows);
        const int o0 = sld(off + 2 * q), o1 = sld(off + 2 * q + 1);
        slot32_a<kR, kAll>(a, v.x, v.y, o0, xr, act, sum);
        slot32_a<kR, kAll>(a, v.z, v.w, o1, xr, act, sum);
    }
    if (wdt & 1) {  // (block-uniform) the odd width's last slot
        const f2v v = ld_f2<kNT>(base + (size_t)(wdt - 1) * kSliceRows + (size_t)threadIdx.x * 2);
        slot32_a<kR, kAll>(a, v.x, v.y, sld(off + wdt - 1), xr, act, sum);
    }
}

// One run of three slots o - 1, o, o + 1 for every column: hpccg_spmm.h's
// x-triple plan. One 16-B load of the centre pair serves the run; row 2t's left
// neighbour and row 2t + 1's right neighbour come from the adjacent lanes, lanes
// 0 and 63 load their one outside value. The same x values in the same products
// in slot order: the slot loop's bits.
template <int kR, class A>
__device__ __forceinline__ void triple32(const A& a, float a0, float a1, float b0, float b1, float c0, float c1, int o,
                                         const double* __restrict__ xr, double (&sum)[kR][kRpt])
{
    const int lane = threadIdx.x & (kWave - 1);
    const double v00 = (double)a0, v01 = (double)a1, v10 = (double)b0, v11 = (double)b1, v20 = (double)c0,
                 v21 = (double)c1;
#pragma unroll
    for (int c = 0; c < kR; c++) {
        const double* __restrict__ xc = xr + ((long long)c * a.pcs + o);
        const Rows ctr = ld_u(xc);
        double left = wave_shr1(ctr.v[1]);
        double right = wave_shl1(ctr.v[0]);
        if (lane == 0) left = xc[-1];
        if (lane == kWave - 1) right = xc[2];
        sum[c][0] = sum[c][0] + v00 * left;
        sum[c][1] = sum[c][1] + v01 * ctr.v[0];
        sum[c][0] = sum[c][0] + v10 * ctr.v[0];
        sum[c][1] = sum[c][1] + v11 * ctr.v[1];
        sum[c][0] = sum[c][0] + v20 * ctr.v[1];
        sum[c][1] = sum[c][1] + v21 * right;
    }
}

// The x-triple plan over the 27 slots of the fp32 image: nine runs of three
// slots against slot pairs of two, so three 16-B value loads serve two runs
// (four times), and the last run takes the thirteenth pair and the odd slot.
template <int kR, bool kNT, class A>
__device__ __forceinline__ void spmm32_a_triples(const A& a, const float* __restrict__ base,
                                                 const int* __restrict__ off, const double* __restrict__ xr,
                                                 double (&sum)[kR][kRpt])
{
    static_assert(kTriples == 9, "27 slots");
    const float* __restrict__ vp = base + (size_t)threadIdx.x * 4;
    // (not unrolled, as the fp64 plan: one pass's loads in flight per thread)
#pragma unroll 1
    for (int h = 0; h < 4; h++) {
        const f4v p0 = ld_f4<kNT>(vp + (size_t)(6 * h) * kSliceRows);
        const f4v p1 = ld_f4<kNT>(vp + (size_t)(6 * h + 2) * kSliceRows);
        const f4v p2 = ld_f4<kNT>(vp + (size_t)(6 * h + 4) * kSliceRows);
        triple32<kR>(a, p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, sld(off + 6 * h + 1), xr, sum);
        triple32<kR>(a, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w, sld(off + 6 * h + 4), xr, sum);
    }
    const f4v p = ld_f4<kNT>(vp + (size_t)24 * kSliceRows);
    const f2v q = ld_f2<kNT>(base + (size_t)26 * kSliceRows + (size_t)threadIdx.x * 2);
    triple32<kR>(a, p.x, p.y, p.z, p.w, q.x, q.y, sld(off + 25), xr, sum);
}

// The body of a unit's SpMM kernel<kW, kR, kNT> over the fp32 SELL-512-A image
// (one block per slice). Width 27 with four columns: slices whose offsets come
// in runs of three use the x-triple plan where a.tri allows it (an A with
// hpccg_spmm.h's `int tri`), as the fp64 body does.
template <int kW, int kR, bool kNT, class A, class E = SpmmToAp>
__device__ __forceinline__ void spmm32_a_body(const A& a, bool prologue)
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
    const double* __restrict__ xr = E::x(a) + (size_t)a.c0 * a.pcs + row;  // column c0 + c: x of column row + off at xr[c * pcs + off]
    double sum[kR][kRpt];
#pragma unroll
    for (int c = 0; c < kR; c++)
#pragma unroll
        for (int i = 0; i < kRpt; i++) sum[c][i] = 0.0;
    bool tri = false;
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
        if constexpr (kTri) spmm32_a_triples<kR, kNT>(a, base, off, xr, sum);
    } else if (all) {
        spmm32_a_slots<kW, kR, kNT, true>(a, base, off, wdt, xr, act, sum);
    } else {
        spmm32_a_slots<kW, kR, kNT, false>(a, base, off, wdt, xr, act, sum);
    }
    E::template out<kR>(a, prologue, s, row, act, sum);
}

// One slot of the SELL-512 image for every column.
template <int kR, class A>
__device__ __forceinline__ void slot32_sell(const A& a, float v0, float v1, int c0, int c1,
                                            const double* __restrict__ x0, const bool (&act)[kR],
                                            double (&sum)[kR][kRpt])
{
    const double w[kRpt] = {(double)v0, (double)v1};
    const int col[kRpt] = {c0, c1};
#pragma unroll
    for (int c = 0; c < kR; c++) {
        if (!act[c]) continue;  // (block-uniform)
        const double* __restrict__ x = x0 + (size_t)c * a.pcs;
#pragma unroll
        for (int i = 0; i < kRpt; i++) {
            const double xv = (col[i] >= 0) ? x[col[i]] : 0.0;
            sum[c][i] = sum[c][i] + w[i] * xv;
        }
    }
}

// The body of a unit's SpMM kernel<kR, kNT> over the fp32 SELL-512 image (the
// shared int32 columns; matrices without an A image). Padding slots (column
// -1, value 0) add +0.
template <int kR, bool kNT, class A, class E = SpmmToAp>
__device__ __forceinline__ void spmm32_sell_body(const A& a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    bool act[kR], all;
    if (!active_cols<kR>(a, act, all)) return;
    const size_t sb = (size_t)sld(a.slice_base + s) * kSliceRows;
    const int w = (int)(sld(a.slice_base + s + 1) - sld(a.slice_base + s));
    const float* __restrict__ base = a.img + sb;
    const int* __restrict__ cp = a.cols + sb + (size_t)threadIdx.x * kRpt;
    const double* __restrict__ x0 = E::x(a) + ((long long)a.c0 * a.pcs + a.xsell);
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
    E::template out<kR>(a, prologue, s, row, act, sum);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// The fp32 image of one matrix (a unit's Workspace derives from it): kept while
// the columns grow, counted in img_bytes; the verdict stays when the image goes.
struct Image32 {
    float* img = nullptr;
    long long img_bytes = 0;
    bool built = false;
    long long inexact = 0, out_of_range = 0;

    void free_image()
    {
        if (img) (void)hipFree(img);
        img = nullptr;
        img_bytes = 0;
    }
};

typedef void (*Convert32Kernel)(const double*, const unsigned int*, int, float*, unsigned long long*);

// The fp32 image, built once per matrix on the device from the image it holds,
// by the unit's convert kernel. who: the name in front of the unit's messages.
int ensure_image32(Image32* im, const MatrixView& v, Convert32Kernel k_convert, const char* who)
{
    auto out_of_range = [&] {
        return fail(HPCCG_HIP_EINVAL,
                    "%s: the matrix is outside fp32 range (%lld stored values with no finite, normal fp32 image)", who,
                    im->out_of_range);
    };
    if (im->built) return im->out_of_range ? out_of_range() : 0;
    hipStream_t s = v.stream;
    HIP_TRY(hipSetDevice(v.device));
    const double* vals = v.has_a ? v.aval : v.vals;
    const unsigned int* tab = v.has_a ? v.abase : v.slice_base;
    const int width = v.has_a ? v.a_width : 0;
    long long slot_rows = (long long)v.nslices * width;
    if (width <= 0) {
        unsigned int last = 0;
        HIP_TRY(hipMemcpyAsync(&last, tab + v.nslices, sizeof last, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        slot_rows = last;
    }
    const size_t bytes = sizeof(float) * (size_t)std::max<long long>(slot_rows, 1) * kSliceRows;
    unsigned long long* flags = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&im->img), bytes));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&flags), 2 * sizeof *flags);
    unsigned long long h[2] = {0, 0};
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, 2 * sizeof *flags, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_convert, dim3(v.nslices), dim3(kBlock), 0, s, vals, tab, width, im->img, flags);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (flags) (void)hipFree(flags);
    if (e != hipSuccess) {
        (void)hipFree(im->img);
        im->img = nullptr;
        return fail(e == hipErrorOutOfMemory ? HPCCG_HIP_ENOMEM : HPCCG_HIP_EHIP, "%s: building the fp32 image: %s",
                    who, hipGetErrorString(e));
    }
    im->built = true;
    im->inexact = (long long)h[0];
    im->out_of_range = (long long)h[1];
    im->img_bytes = (long long)bytes;
    if (im->out_of_range) {  // never solved with: the image goes, the verdict stays
        im->free_image();
        return out_of_range();
    }
    return 0;
}

}  // namespace

}  // namespace hpccg
