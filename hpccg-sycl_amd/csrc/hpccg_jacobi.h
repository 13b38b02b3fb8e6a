// hpccg_jacobi.h -- the diagonal preconditioner's vector, shared by the
// preconditioned units (through hpccg_onerank_host.h hpccg_pcg.hip,
// hpccg_srcg.hip, hpccg_pcg_group.hip and the four polynomial units): reading
// a_ii from the matrix image, checking a caller's m, and the part of a
// workspace that holds them while its columns grow.
//   device  the bodies of the diagonal kernel and of the check kernel; a unit's
//           __global__ entry points are thin wrappers over them
//   host    DiagArgs from a matrix view; JacobiCache (a unit's Workspace derives
//           from it beside ColWorkspace): the cached 1 / a_ii with its verdict,
//           the slot for a call's own m, the "first bad row" word
// A matrix with ghost rows (a member of an in-process group) is read like any
// other: SELL-512-A offsets are local column - local row, so the offset-0 slot
// is a_ii; SELL-512 columns count the ghost_lo rows, and the view's
// sell_col_base (-ghost_lo) puts them back on local rows.
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include <climits>

#include "hpccg_columns.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct DiagArgs {
    int n, has_a, a_width;
    long long xsell;
    const double* aval;
    const int* aoff;
    const unsigned int* abase;
    const unsigned int* slice_base;
    const int* cols;
    const double* vals;
};

// ---------------------------------------------------------------------------
// The diagonal, one block per slice, a thread its two rows: the offset-0 slot
// of the slice (SELL-512-A; a hole there is 0.0) or the first slot whose column
// is the row (SELL-512). d_out (may be null; any alignment): a_ii, 0.0 where
// none is stored. minv_out (may be null; a padded vector): 1.0 / a_ii, and
// *bad becomes the first row whose a_ii or 1.0 / a_ii is not finite and > 0.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void diag_body(const DiagArgs& a, double* d_out, double* minv_out, int* bad)
{
    const int s = blockIdx.x;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    Rows d{{0.0, 0.0}};
    if (a.has_a) {
        const int wdt = a.a_width > 0 ? a.a_width : (int)(a.abase[s + 1] - a.abase[s]);
        const size_t vb = a.a_width > 0 ? (size_t)s * a.a_width : (size_t)a.abase[s];
        const int* __restrict__ off = a.aoff + (size_t)s * kAMax;
        for (int j = 0; j < wdt; j++)
            if (off[j] == 0) {  // (block-uniform)
                d = ld(a.aval + (vb + j) * kSliceRows + (size_t)threadIdx.x * kRpt);
                break;
            }
    } else {
        const size_t base = (size_t)a.slice_base[s] * kSliceRows + (size_t)threadIdx.x * kRpt;
        const int w = (int)(a.slice_base[s + 1] - a.slice_base[s]);
        bool found[kRpt] = {false, false};
        for (int j = 0; j < w; j++) {
#pragma unroll
            for (int i = 0; i < kRpt; i++) {
                const int col = a.cols[base + (size_t)j * kSliceRows + i];
                if (!found[i] && col >= 0 && col + a.xsell == (long long)(row + i)) {
                    d.v[i] = a.vals[base + (size_t)j * kSliceRows + i];
                    found[i] = true;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kRpt; i++) {
        if (row + i >= a.n) continue;
        if (d_out) d_out[row + i] = d.v[i];
        if (minv_out) {
            const double m = 1.0 / d.v[i];
            minv_out[row + i] = m;
            if (!(d.v[i] > 0.0 && isfinite(d.v[i]) && isfinite(m))) atomicMin(bad, row + i);
        }
    }
}

// *bad becomes the first row of m that is not finite and > 0 (one thread per row).
__device__ __forceinline__ void check_body(const double* __restrict__ m, int n, int* bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = m[i];
    if (!(v > 0.0 && isfinite(v))) atomicMin(bad, i);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
typedef void (*DiagKernel)(DiagArgs, double*, double*, int*);
typedef void (*CheckKernel)(const double*, int, int*);

// (inline: hpccg_onerank_host.h brings this header to units without a preconditioner)
inline DiagArgs diag_args(const MatrixView& v)
{
    DiagArgs d{};
    d.n = v.n;
    d.has_a = v.has_a;
    d.a_width = v.a_width;
    d.xsell = v.sell_col_base;
    d.aval = v.aval;
    d.aoff = v.aoff;
    d.abase = v.abase;
    d.slice_base = v.slice_base;
    d.cols = v.cols;
    d.vals = v.vals;
    return d;
}

// What stays while the columns grow: the cached 1 / a_ii (matrices are
// immutable) with its verdict, a call's own m, the "first bad row" word.
struct JacobiCache {
    double *jac = nullptr, *muser = nullptr;
    int* bad = nullptr;
    long long rest_bytes = 0;
    bool jac_built = false;
    int jac_bad_row = -1;

    void free_cache()
    {
        for (void* q : {(void*)jac, (void*)muser, (void*)bad})
            if (q) (void)hipFree(q);
        jac = muser = nullptr;
        bad = nullptr;
        rest_bytes = 0;
    }
};

// The cache's vectors (zeroed: the rows past n of jac and muser are loaded and
// never stored). W: a ColWorkspace and a JacobiCache.
template <class W>
int ensure_cache(W* w)
{
    if (w->jac) return 0;
    HIP_TRY(hipSetDevice(w->v.device));
    const size_t npad = (size_t)w->v.npad;
    const long long before = w->bytes;  // (alloc_zero counts into bytes: the columns')
    int rc = alloc_zero(w, &w->bad, 1);
    if (!rc) rc = alloc_zero(w, &w->muser, npad);
    if (!rc) rc = alloc_zero(w, &w->jac, npad);
    w->rest_bytes += w->bytes - before;
    w->bytes = before;
    if (rc) w->free_cache();
    return rc;
}

// The first bad row a check kernel found (-1: none), once the stream has run dry.
template <class W>
int read_bad(W* w, int* row)
{
    int h = INT_MAX;
    HIP_TRY(hipMemcpyAsync(&h, w->bad, sizeof h, hipMemcpyDeviceToHost, w->v.stream));
    HIP_TRY(hipStreamSynchronize(w->v.stream));
    *row = h == INT_MAX ? -1 : h;
    return 0;
}

template <class W>
int arm_bad(W* w)
{
    static const int kNoRow = INT_MAX;  // above every row index
    HIP_TRY(hipMemcpyAsync(w->bad, &kNoRow, sizeof(int), hipMemcpyHostToDevice, w->v.stream));
    return 0;
}

// Jacobi: 1.0 / a_ii into w->jac, built once per matrix on the device by the
// unit's diagonal kernel; the verdict on a matrix it does not exist for is kept
// too. *row: the first row whose diagonal is missing, not finite or <= 0 (-1: none).
template <class W>
int build_jacobi(W* w, DiagKernel k_diag, int* row)
{
    if (!w->jac_built) {
        TRY(arm_bad(w));
        hipLaunchKernelGGL(k_diag, dim3(w->v.nslices), dim3(kBlock), 0, w->v.stream, diag_args(w->v), (double*)nullptr,
                           w->jac, w->bad);
        HIP_TRY(hipGetLastError());
        TRY(read_bad(w, &w->jac_bad_row));
        w->jac_built = true;
    }
    *row = w->jac_bad_row;
    return 0;
}

// A call's own m into the padded w->muser (kind: where minv lives), checked by
// the unit's check kernel. *row: the first entry not finite and > 0 (-1: none).
template <class W>
int load_minv(W* w, const double* minv, hipMemcpyKind kind, CheckKernel k_check, int* row)
{
    hipStream_t s = w->v.stream;
    const int n = w->v.n;
    HIP_TRY(hipMemcpyAsync(w->muser, minv, sizeof(double) * (size_t)n, kind, s));
    TRY(arm_bad(w));
    hipLaunchKernelGGL(k_check, dim3((n + 255) / 256), dim3(256), 0, s, (const double*)w->muser, n, w->bad);
    HIP_TRY(hipGetLastError());
    return read_bad(w, row);
}

}  // namespace

}  // namespace hpccg
