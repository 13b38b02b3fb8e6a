// hpccg_poly_bodies.h -- the device code of the Chebyshev polynomial
// preconditioner (include/hpccg_hip_poly.h), shared by the one-rank unit
// (hpccg_poly.hip) and the unit over an in-process rank group
// (hpccg_poly_group.hip): one definition of every rounding-relevant expression,
// so a member's rows are computed as the one-rank solve computes them.
//   device  PolyArgs; the update with step 0 in r's pass (poly_update0); the
//           ends of a step's SpMM body (PolyStep, for hpccg_spmm.h's loops);
//           the bodies of the bound's kernels (q = sqrt(m), the slice maxima of
//           the symmetric Gershgorin rows, their maximum) with max_nan and
//           block_max. A unit's __global__ entry points are thin wrappers.
// The vectors the bodies read at neighbour offsets (a step's z, the bound's q)
// are columns in p's layout: a zeroed guard zone around each and, for a group
// member, its ghost planes (hpccg_group.h: guarded_p_column).
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include "hpccg_columns.h"
#include "hpccg_jacobi.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct PolyArgs : ColArgs {
    // (ColArgs' p: a guard zone around each column; minv: the call's m)
    int tri;  // width 27: slices whose offsets come in runs of three use the x-triple plan
    const double* aval;
    const double* vals;
    // the Chebyshev application (z buffers: local row 0 of column 0, p's column layout)
    const double* zin;  // a step's input z
    double* zout;       // a step's output z; the update kernel: step 0's
    double* dd;         // column c at dd + c * vcs
    double cheb0;       // step 0's scalar
    double aj, bj;      // step j's scalars
    int last;           // 1: the last step (it forms the r.z slice partial)
};

// ---------------------------------------------------------------------------
// prologue: r = b + (-1)*Ap | loop: x = x + alpha*p; r = r + (-alpha)*Ap
// (col_update's statements), then step 0 on the new r in the same pass:
//   t = m*r;  dd = c0*t;  z = dd
// and the r.r slice partial. The r.z slice partial is the last step's.
// ---------------------------------------------------------------------------
template <int kR>
__device__ __forceinline__ void poly_update0(const PolyArgs& a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    const Rows mv = ld(a.minv + row);
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        if (c >= a.nrhs) break;
        if (!a.st[c].run) continue;  // (block-uniform)
        double* __restrict__ rc = a.r + (size_t)c * a.rcs;
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
        Rows dn;
#pragma unroll
        for (int i = 0; i < kRpt; i++) {
            const double t = mv.v[i] * rn.v[i];
            dn.v[i] = a.cheb0 * t;
        }
        st_rows(a.dd + (size_t)c * a.vcs, row, a.n, dn);
        st_rows(a.zout + (size_t)c * a.pcs, row, a.n, dn);
        rr_slice_partial(a, s, row, c, rn);
    }
}

// ---------------------------------------------------------------------------
// The ends of a step's SpMM body: x is the step's input z; the row sums
// w = (A z)_i stay in registers and step j is applied to them:
//   t = m_i*(r_i - w_i);  dd_i = a_j*dd_i + b_j*t;  z_i = z_i + dd_i
// dd in place (a row is its own thread's), z into the other buffer (its
// neighbours are still being read by the launch's other blocks). m is loaded
// once for the launch's columns. The last step adds the r.z slice partial in
// rw_slice_partial's order.
// ---------------------------------------------------------------------------
struct PolyStep {
    static __device__ __forceinline__ const double* x(const PolyArgs& a) { return a.zin; }

    template <int kR>
    static __device__ __forceinline__ void out(const PolyArgs& a, bool, int s, int row, const bool (&act)[kR],
                                               const double (&sum)[kR][kRpt])
    {
        const Rows mv = ld(a.minv + row);
#pragma unroll
        for (int j = 0; j < kR; j++) {
            if (!act[j]) continue;  // (block-uniform)
            const int c = a.c0 + j;
            const Rows rv = ld(a.r + (size_t)c * a.rcs + row);
            double* __restrict__ dc = a.dd + (size_t)c * a.vcs;
            const Rows dv = ld(dc + row);
            const Rows zv = ld(a.zin + (size_t)c * a.pcs + row);
            Rows dn, zn;
#pragma unroll
            for (int i = 0; i < kRpt; i++) {
                const double t = mv.v[i] * (rv.v[i] - sum[j][i]);
                dn.v[i] = a.aj * dv.v[i] + a.bj * t;
                zn.v[i] = zv.v[i] + dn.v[i];
            }
            st_rows(dc, row, a.n, dn);
            st_rows(a.zout + (size_t)c * a.pcs, row, a.n, zn);
            if (a.last) rw_slice_partial(a, kDotRZ, s, row, c, rv, zn);  // (block-uniform)
        }
    }
};

// ---------------------------------------------------------------------------
// The symmetric Gershgorin bound on the spectrum of M^-1 A (that of
// M^-1/2 A M^-1/2): with q_i = sqrt(m_i),
//   g_i = q_i * sum_j |a_ij|*q_j  (slot order; holes and padding slots add 0),
//   lmax = max_i g_i.
// One pass over the image: an SpMV with |a| on q (a guarded copy, p's column
// layout), a max per slice, then one block over the slice maxima. A NaN stays.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double max_nan(double a, double b)
{
    return (b > a || b != b) ? b : a;
}

// valid in thread 0
__device__ __forceinline__ double block_max(double v)
{
    constexpr int kWaves = kBlock / kWave;
    __shared__ double wmax[kWaves];
    v = max_nan(v, from_lane_plus<32>(v));
    v = max_nan(v, from_lane_plus<16>(v));
    v = max_nan(v, from_lane_plus<8>(v));
    v = max_nan(v, from_lane_plus<4>(v));
    v = max_nan(v, from_lane_plus<2>(v));
    v = max_nan(v, from_lane_plus<1>(v));
    if ((threadIdx.x & (kWave - 1)) == 0) wmax[threadIdx.x / kWave] = v;
    __syncthreads();
    double m = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kWaves; i++) m = max_nan(m, wmax[i]);
    }
    return m;
}

// (The pointer parameters of the three bodies carry no __restrict__: the
// wrappers' kernel parameters do, as the kernels did before the bodies moved
// here, and the code objects stay what they were.)
// q_i = sqrt(m_i) for the n rows (q: local row 0 of the guarded copy; one thread per row)
__device__ __forceinline__ void poly_q_body(const double* m, int n, double* q)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) q[i] = sqrt(m[i]);
}

// One block per slice, a thread its two rows: smax[s] = max of g over the slice's rows < n.
__device__ __forceinline__ void poly_bound_body(const DiagArgs& a, const double* q, double* smax)
{
    const int s = blockIdx.x;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    double g[kRpt] = {0.0, 0.0};
    if (a.has_a) {
        const int wdt = a.a_width > 0 ? a.a_width : (int)(sld(a.abase + s + 1) - sld(a.abase + s));
        const size_t vb = a.a_width > 0 ? (size_t)s * a.a_width : (size_t)sld(a.abase + s);
        const double* __restrict__ vp = a.aval + vb * kSliceRows + (size_t)threadIdx.x * kRpt;
        const int* __restrict__ off = a.aoff + (size_t)s * kAMax;
        const double* __restrict__ xr = q + row;
#pragma unroll 4
        for (int j = 0; j < wdt; j++) {
            const Rows v = ld(vp + (size_t)j * kSliceRows);
            const Rows xv = ld_u(xr + sld(off + j));
#pragma unroll
            for (int i = 0; i < kRpt; i++) g[i] = g[i] + fabs(v.v[i]) * xv.v[i];
        }
    } else {
        const size_t base = (size_t)sld(a.slice_base + s) * kSliceRows + (size_t)threadIdx.x * kRpt;
        const int w = (int)(sld(a.slice_base + s + 1) - sld(a.slice_base + s));
        const double* __restrict__ x0 = q + a.xsell;
        for (int j = 0; j < w; j++) {
#pragma unroll
            for (int i = 0; i < kRpt; i++) {
                const int col = a.cols[base + (size_t)j * kSliceRows + i];
                const double xv = (col >= 0) ? x0[col] : 0.0;
                g[i] = g[i] + fabs(a.vals[base + (size_t)j * kSliceRows + i]) * xv;
            }
        }
    }
    const Rows qv = ld(q + row);
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < kRpt; i++)
        if (row + i < a.n) m = max_nan(m, qv.v[i] * g[i]);
    m = block_max(m);
    if (threadIdx.x == 0) smax[s] = m;
}

// One block: *out = max of the nslices slice maxima.
__device__ __forceinline__ void poly_bound_top_body(const double* smax, int nslices, double* out)
{
    double m = 0.0;
    for (int i = threadIdx.x; i < nslices; i += kBlock) m = max_nan(m, smax[i]);
    m = block_max(m);
    if (threadIdx.x == 0) *out = m;
}

}  // namespace

}  // namespace hpccg
