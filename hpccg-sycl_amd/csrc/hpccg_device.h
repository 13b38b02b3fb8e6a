// hpccg_device.h -- device pieces shared by the kernel translation units
// (hpccg_kernels.hip, hpccg_batch.hip, hpccg_mixed.hip; the latter two through
// hpccg_columns.h): the row-blocked vector access and the fixed-shape
// reductions. Every rounding shape of a dot product exists once, here, so a
// kernel of any unit that sums the same values gets the same bits. Internal linkage (each unit inlines its own copy); device code only.
#pragma once
#include "hpccg_internal.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

constexpr int kWave = 64;
constexpr int kRpt = 2;                    // rows per thread in every slice kernel
constexpr int kBlock = kSliceRows / kRpt;  // 256 threads per slice

// Block b of a grid dealt round-robin over the 8 XCDs -> logical slice, so
// that every XCD walks one contiguous 1/8 of the rows (x re-reads of the
// stencil's neighbouring planes then hit that XCD's L2). Speed only: no
// result depends on the placement.
__device__ __forceinline__ int xcd_slice(int grid)
{
    const int b = blockIdx.x;
    const int per = grid / kNumXcd;
    return (b % kNumXcd) * per + (b / kNumXcd);
}

// Lane l < off receives lane l + off (gfx950 lane moves, no LDS traffic):
// permlane32/16_swap for the cross-row steps, DPP row_shl inside a row.
template <int kOff>
__device__ __forceinline__ double from_lane_plus(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    int rlo, rhi;
    if constexpr (kOff == 32) {
        rlo = __builtin_amdgcn_permlane32_swap(lo, lo, false, false)[1];
        rhi = __builtin_amdgcn_permlane32_swap(hi, hi, false, false)[1];
    } else if constexpr (kOff == 16) {
        rlo = __builtin_amdgcn_permlane16_swap(lo, lo, false, false)[1];
        rhi = __builtin_amdgcn_permlane16_swap(hi, hi, false, false)[1];
    } else {
        static_assert(kOff >= 1 && kOff <= 8, "row_shl range");
        rlo = __builtin_amdgcn_update_dpp(0, lo, 0x100 + kOff, 0xF, 0xF, false);
        rhi = __builtin_amdgcn_update_dpp(0, hi, 0x100 + kOff, 0xF, 0xF, false);
    }
    return __hiloint2double(rhi, rlo);
}

// Whole-wave lane shifts (DPP wave_shr:1 / wave_shl:1): lane l receives lane
// l - 1 / l + 1; lane 0 / lane 63 receive 0.0 (the caller loads those itself).
__device__ __forceinline__ double wave_shr1(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x138, 0xF, 0xF, false),
                            __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ double wave_shl1(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x130, 0xF, 0xF, false),
                            __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xF, 0xF, false));
}

// Wave sum, result valid in LANE 0 only. Fixed tree: v_l += v_{l+off} for
// off = 32, 16, 8, 4, 2, 1 (lanes >= off are don't-care).
__device__ __forceinline__ double wave_sum(double v)
{
    v += from_lane_plus<32>(v);
    v += from_lane_plus<16>(v);
    v += from_lane_plus<8>(v);
    v += from_lane_plus<4>(v);
    v += from_lane_plus<2>(v);
    v += from_lane_plus<1>(v);
    return v;
}

// Deterministic block reduction (fixed shape): wave sums, then the wave sums
// in wave order by thread 0. Result valid in thread 0.
template <int kThreads>
__device__ __forceinline__ double block_sum(double v)
{
    constexpr int kWaves = kThreads / kWave;
    __shared__ double wsum[kWaves];
    v = wave_sum(v);
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    if (lane == 0) wsum[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kWaves; i++) s += wsum[i];
    }
    return s;
}

// ---------------------------------------------------------------------------
// Row-blocked vector access: thread t owns rows 2t, 2t + 1 of its slice, so
// every vector stream is 16 B per lane.
// ---------------------------------------------------------------------------
struct Rows {
    double v[kRpt];
};

typedef double d2v __attribute__((ext_vector_type(2)));
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

__device__ __forceinline__ Rows ld(const double* __restrict__ p)
{
    const d2v t = *reinterpret_cast<const d2v*>(p);
    return Rows{{t.x, t.y}};
}

// 8-byte aligned pair (SELL-512-A reads x at odd offsets)
__device__ __forceinline__ Rows ld_u(const double* __restrict__ p)
{
    const d2u t = *reinterpret_cast<const d2u*>(p);
    return Rows{{t.x, t.y}};
}

// Matrix streams: non-temporal when the image is far beyond the Infinity
// Cache (read once per SpMV; keeps L2 for the vectors).
template <bool kNT>
__device__ __forceinline__ Rows ld_m(const double* __restrict__ p)
{
    if constexpr (!kNT) {
        return ld(p);
    } else {
        const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
        return Rows{{t.x, t.y}};
    }
}

// Vectors are allocated padded to a multiple of 512 rows, so full-width loads
// are always in bounds; rows >= n are masked on store and in the dots.
__device__ __forceinline__ void st_rows(double* __restrict__ base, int row, int n, const Rows& o)
{
    if (row + kRpt <= n) {
        *reinterpret_cast<d2v*>(base + row) = d2v{o.v[0], o.v[1]};
    } else {
        for (int i = 0; i < kRpt; i++)
            if (row + i < n) base[row + i] = o.v[i];
    }
}

// The two upper levels of every dot product (see "Dot-product completion" in
// hpccg_kernels.hip): groups of kGroup slice partials, then kTopThreads
// virtual threads over the group sums.
constexpr int kGroup = 64;
constexpr int kTopThreads = 256;

// The fixed top-level shape computed by one wave (virtual waves in order);
// valid in lane 0. ld(i) reads group sum i. All loads are issued before the sums.
template <class Ld>
__device__ __forceinline__ double top_sum_wave(Ld ld, int ng, int lane)
{
    constexpr int kVWaves = kTopThreads / kWave;
    double v[kVWaves];
#pragma unroll
    for (int vw = 0; vw < kVWaves; vw++) v[vw] = 0.0;
    for (int i0 = 0; i0 < ng; i0 += kTopThreads) {
        double t[kVWaves];
#pragma unroll
        for (int vw = 0; vw < kVWaves; vw++) {
            const int i = i0 + vw * kWave + lane;
            t[vw] = i < ng ? ld(i) : 0.0;
        }
#pragma unroll
        for (int vw = 0; vw < kVWaves; vw++)
            if (i0 + vw * kWave < ng) v[vw] += t[vw];
    }
    double s = 0.0;
#pragma unroll
    for (int vw = 0; vw < kVWaves; vw++) s += wave_sum(v[vw]);
    return s;
}

}  // namespace

}  // namespace hpccg
