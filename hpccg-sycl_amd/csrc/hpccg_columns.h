// hpccg_columns.h -- the column-recurrence engine shared by the multi-column
// units (hpccg_batch.hip, hpccg_mixed.hip, hpccg_pcg.hip, hpccg_pcg_group.hip, hpccg_poly.hip,
// hpccg_poly_group.hip): one CG recurrence
// per column of a call, each with the single solve's expressions and the
// single solve's dot shape (hpccg_device.h). Every rounding-relevant expression
// at column level and the loop test exist once, here, so column c of the batch
// or the mixed library is bitwise the single solve of it. The bodies' kPre
// forms are the diagonally preconditioned recurrence (hpccg_pcg.hip): the same
// statements with z = m r in r's place where the recurrence asks for z, and a
// second dot, r.z, beside r.r; with m = 1 they are the plain ones bit for bit.
//   device  ColState, ColArgs; the bodies of the init kernel, the p update, the
//           SpMM epilogue, the update with its r.r slice partial and the
//           finalize. A unit's __global__ entry points are thin wrappers over
//           them; its SpMM loops (value type, load shape: the tuned part) are
//           its own or hpccg_spmm.h's.
//   host    error helpers, the workspace registry, the shared vector set with
//           its grow-or-keep logic, the eager launch loop of one recurrence,
//           its end (wall time, the history -> trace read-back) and the trace's
//           copy-out.
// The same recurrence over an in-process rank group is hpccg_group.h, on top of
// this header.
// Internal linkage (each unit compiles its own copy), like hpccg_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/hpccg_hip.h"
#include "hpccg_device.h"
#include "hpccg_internal.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// Per-column scalar state of the running recurrence: set before it starts (a
// kernel or an upload of the unit's), advanced by the finalize only (a group
// member's: by the group's sum only).
//   Preconditioned (kPre; m the unit's positive vector, z = m r never stored):
// rtrans and oldrtrans hold r.z, which alpha and beta are made of, and rr holds
// r.r, which the history and the loop test are made of. Unpreconditioned the
// two are one number, stored twice.
struct ColState {
    double rtrans;     // r_{k-1}.z_{k-1} of the iteration k about to run (HPCCG.cpp: rtrans)
    double oldrtrans;  // r_{k-2}.z_{k-2}
    double rr;         // r_{k-1}.r_{k-1}
    double pap;        // p_k.Ap_k
    double alpha;      // rtrans / pap
    double beta;       // rtrans / oldrtrans (0.0 for k = 1)
    double tol;        // the loop test's tolerance of this column's recurrence
    int k;             // the iteration about to run (0: the prologue)
    int run;           // 1: iteration k runs; 0: the column is frozen
    int niters;        // iterations done once the recurrence has ended
    int max_iter;      // the loop test's iteration limit of this column's recurrence
};

// (kDotRZ: the preconditioned recurrence's r.z partials, completed by the r.r finalize)
enum Dot : int { kDotRR = 0, kDotPAP = 1, kDotRZ = 2 };

// What every kernel of a unit takes (the unit's own struct adds its matrix values).
struct ColArgs {
    int n, nslices, grid;
    int nrhs;      // columns of the call
    int c0;        // first column of this launch (it covers c0 .. c0 + kR - 1, those < nrhs)
    int cap;       // columns the workspace holds (stride of the partials)
    int ng;        // ceil(nslices / kGroup)
    int force;     // 1: every column runs whatever its state (the plain SpMM)
    int nt, a_width;
    double* p;     // local row 0 of column 0; column c at p + c * pcs (a zeroed guard zone around each)
    long long xsell;  // SELL-512 column 0 relative to local row 0
    double* r;     // column c at r + c * rcs
    double* Ap;    // column c at Ap + c * vcs, as x, b
    double* x;     // the recurrence's unknown
    double* b;     // the recurrence's right-hand side
    long long pcs, vcs, rcs;
    const double* minv;  // preconditioned: m, one entry per row, shared by the columns (else unused)
    double* partial;  // [ndots][cap][nslices] slice partials (r.r, then p.Ap; preconditioned: then r.z)
    double* gsum;     // [ndots][cap][ng] group sums (beyond the finalize block's LDS only)
    double* tot;      // [which][cap] dot totals the finalize stores instead of advancing the state
    ColState* st;     // [cap]
    double* hist;     // [cap][hstride]: hist[c][k] = r_k.r_k
    long long hstride;
    int* ended;       // columns whose loop has ended
    const int* aoff;
    const unsigned int* abase;
    const unsigned int* slice_base;
    const int* cols;
};

// Wave-uniform table loads through the scalar cache (tables no kernel writes).
template <class T>
__device__ __forceinline__ T sld(const T* p)
{
    return *(const __attribute__((address_space(4))) T*)(p);
}

template <int kR>
__device__ __forceinline__ bool active_cols(const ColArgs& a, bool (&act)[kR], bool& all)
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

__device__ __forceinline__ double* slice_partials(const ColArgs& a, int which, int c)
{
    return a.partial + ((size_t)which * a.cap + c) * (size_t)a.nslices;
}

// Every column of the call runs, with the call's tolerance and limit (one
// thread per column).
__device__ __forceinline__ void col_init(const ColArgs& a, int max_iter, double tol)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) *a.ended = 0;
    if (c >= a.nrhs) return;
    ColState s;
    s.rtrans = s.oldrtrans = s.rr = s.pap = s.alpha = s.beta = 0.0;
    s.tol = tol;
    s.k = 0;
    s.run = 1;
    s.niters = 0;
    s.max_iter = max_iter;
    a.st[c] = s;
}

// ---------------------------------------------------------------------------
// p = x + 0.0*x (prologue, HPCCG.cpp:347) | p = r + beta*p (k_p_update's
// expression: k == 1 reads r for p, beta 0.0), per running column.
// kPre: p = z + beta*p with z = m*r formed in the register (k == 1: z for p);
// m is loaded once for the launch's columns.
// ---------------------------------------------------------------------------
template <int kR, bool kPre = false>
__device__ __forceinline__ void col_p(const ColArgs& a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    Rows mv{};
    if constexpr (kPre)
        if (!prologue) mv = ld(a.minv + row);
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        if (c >= a.nrhs) break;
        if (!a.st[c].run) continue;  // (block-uniform)
        double* __restrict__ pc = a.p + (size_t)c * a.pcs;
        Rows o;
        if (prologue) {
            const Rows xv = ld(a.x + (size_t)c * a.vcs + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) o.v[i] = xv.v[i] + 0.0 * xv.v[i];
        } else {
            const int k = a.st[c].k;
            const double beta = a.st[c].beta;
            Rows rv = ld(a.r + (size_t)c * a.rcs + row);
            if constexpr (kPre) {
#pragma unroll
                for (int i = 0; i < kRpt; i++) rv.v[i] = mv.v[i] * rv.v[i];  // z
            }
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
__device__ __forceinline__ void spmm_rows_out(const ColArgs& a, bool prologue, int s, int row, const bool (&act)[kR],
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

// The slice partial `which` of column c from this thread's two rows of r and
// of w: sum of r_i * w_i (r.r: w = r; r.z: w = z).
__device__ __forceinline__ void rw_slice_partial(const ColArgs& a, int which, int s, int row, int c, const Rows& rn,
                                                 const Rows& wn)
{
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < kRpt; i++)
        if (row + i < a.n) d += rn.v[i] * wn.v[i];
    const double bs = block_sum<kBlock>(d);
    if (threadIdx.x == 0) slice_partials(a, which, c)[s] = bs;
    __syncthreads();  // block_sum's LDS words are free for the next column
}

// The r.r slice partial of column c from this thread's two rows of r.
__device__ __forceinline__ void rr_slice_partial(const ColArgs& a, int s, int row, int c, const Rows& rn)
{
    rw_slice_partial(a, kDotRR, s, row, c, rn, rn);
}

// ---------------------------------------------------------------------------
// prologue: r = b + (-1)*Ap                         (HPCCG.cpp:352)
// loop:     x = x + alpha*p; r = r + (-alpha)*Ap    (HPCCG.cpp:382-384)
// then the r.r slice partial (k_update's expressions), per running column.
// kPre: also the r.z slice partial, sum of r_i * (m_i * r_i), in the same pass;
// m is loaded once for the launch's columns.
// ---------------------------------------------------------------------------
template <int kR, bool kPre = false>
__device__ __forceinline__ void col_update(const ColArgs& a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    Rows mv{};
    if constexpr (kPre) mv = ld(a.minv + row);
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
        if constexpr (kPre) {
            Rows zn;
#pragma unroll
            for (int i = 0; i < kRpt; i++) zn.v[i] = mv.v[i] * rn.v[i];
            rw_slice_partial(a, kDotRZ, s, row, c, rn, zn);
        }
        rr_slice_partial(a, s, row, c, rn);
    }
}

// The column's scalars once a dot's total is known (one lane).
//   p.Ap: alpha = rtrans / p.Ap                       (HPCCG.cpp:381-382)
//   r.r of iteration k: hist[k]; oldrtrans, rtrans, beta for iteration k + 1
//         and its loop test k + 1 < max_iter && normr > tol, normr being the
//         value iteration k computed, sqrt(r_{k-1}.r_{k-1}) (HPCCG.cpp:358,
//         as cg_run restates it; sqrt(r_0.r_0) for k + 1 = 1).
//   rr: the r.r total beside the r.z total tot of a preconditioned recurrence
//         (hist and the loop test are r.r's, alpha and beta r.z's); else tot
//         itself. Unused for p.Ap.
__device__ __forceinline__ void advance_column(const ColArgs& a, ColState* st, int c, int which, double tot, double rr)
{
    if (which == kDotPAP) {
        st->pap = tot;
        st->alpha = st->rtrans / tot;
        return;
    }
    const int k = st->k;
    const double old = st->rtrans;  // r_{k-1}.z_{k-1} (k >= 1)
    const double oldrr = st->rr;    // r_{k-1}.r_{k-1} (k >= 1)
    a.hist[(size_t)c * a.hstride + k] = rr;
    st->oldrtrans = old;
    st->rtrans = tot;
    st->rr = rr;
    st->beta = (k == 0) ? 0.0 : tot / old;
    st->k = k + 1;
    const bool run = k + 1 < st->max_iter && sqrt(k == 0 ? rr : oldrr) > st->tol;
    if (!run) {
        st->run = 0;
        st->niters = k;
        atomicAdd(a.ended, 1);
    }
}

// ---------------------------------------------------------------------------
// One block per column: the dot's two upper levels (finalize_groups' and
// k_finalize's shapes: a 64-lane butterfly per group of 64 slice partials,
// top_sum_wave over the group sums), then the column's scalars
// (advance_column). store_total: the total goes to tot[which][c] instead and
// the state is left alone (a group member's part of the dot; the r.r of a
// residual step).
// ---------------------------------------------------------------------------
constexpr int kFinThreads = 1024;
constexpr int kFinLds = 2048;  // group sums kept in LDS up to 128 K slices

// The total of column c's dot `which` from its slice partials, by the whole
// block (gs: its kFinLds LDS words); valid in thread 0.
__device__ __forceinline__ double col_dot_total(const ColArgs& a, int which, int c, double* gs)
{
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
    if (threadIdx.x >= kWave) return 0.0;
    return in_lds ? top_sum_wave([&](int i) { return gs[i]; }, ng, lane)
                  : top_sum_wave([gp](int i) { return gp[i]; }, ng, lane);
}

// kPre: the r.r finalize completes the r.z total too (the update kernel's two
// slice partials), and the column advances once on both; with store_total it
// stores both, r.z to tot[kDotRZ][c] (hpccg_pcg_group.hip: ntot = 3).
template <bool kPre = false>
__device__ __forceinline__ void col_finalize(const ColArgs& a, int which, int store_total)
{
    __shared__ double gs[kFinLds];
    const int c = blockIdx.x;
    ColState* const st = a.st + c;
    if (!st->run) return;  // (block-uniform) a frozen column keeps its state
    const double tot = col_dot_total(a, which, c, gs);
    double rz = tot;
    if constexpr (kPre) {
        if (which == kDotRR) {  // (block-uniform)
            __syncthreads();    // the r.r group sums in gs have been read
            rz = col_dot_total(a, kDotRZ, c, gs);
            // (a group member: its part of r.z beside its part of r.r below)
            if (store_total && threadIdx.x == 0) a.tot[(size_t)kDotRZ * a.cap + c] = rz;
        }
    }
    if (threadIdx.x != 0) return;
    if (store_total) {
        a.tot[(size_t)which * a.cap + c] = tot;
        return;
    }
    advance_column(a, st, c, which, rz, tot);
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

// The vectors and scalars of the recurrences on one matrix. A unit's Workspace
// derives from it and adds its own vectors, with
//   void free_own_vectors()  its device vectors (what ensure_columns' `own` allocates)
//   void free_own_rest()     what else it holds, as the record goes
struct ColWorkspace {
    MatrixView v;
    int cap = 0;  // columns
    int ndots = 2;  // dots with slice partials per column (a preconditioned unit: 3, r.z)
    long long pcs = 0, vcs = 0;
    double *pbuf = nullptr, *Ap = nullptr;
    double *partial = nullptr, *gsum = nullptr, *tot = nullptr;
    ColState* st = nullptr;
    int* ended = nullptr;
    double* hist = nullptr;
    long long hstride = 0;
    int* h_ended = nullptr;  // pinned
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    long long bytes = 0;  // of the vectors
};

// A workspace whose recurrences' normr traces are kept for the unit's
// last_trace call (the mixed unit keeps its own records).
struct TraceWorkspace : ColWorkspace {
    std::vector<std::vector<double>> trace;  // per column of the last solve
};

template <class T>
int alloc_zero(ColWorkspace* w, T** p, size_t count)
{
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), bytes));
    HIP_TRY(hipMemsetAsync(*p, 0, bytes, w->v.stream));
    w->bytes += (long long)bytes;
    return 0;
}

template <class W>
void free_vectors(W* w)
{
    if (w->v.stream) (void)hipStreamSynchronize(w->v.stream);
    w->free_own_vectors();
    for (void* q : {(void*)w->pbuf, (void*)w->Ap, (void*)w->partial, (void*)w->gsum, (void*)w->tot, (void*)w->st,
                    (void*)w->ended, (void*)w->hist})
        if (q) (void)hipFree(q);
    w->pbuf = w->Ap = w->partial = w->gsum = w->tot = w->hist = nullptr;
    w->st = nullptr;
    w->ended = nullptr;
    w->cap = 0;
    w->hstride = 0;
    w->bytes = 0;
}

// The workspaces of one unit, keyed by matrix; a record goes with its matrix
// (the destroy hook) or by the unit's release call.
template <class W>
struct Registry {
    std::mutex mu;
    std::map<const hpccg_hip_matrix*, W*> ws;

    W* find(const hpccg_hip_matrix* M)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = ws.find(M);
        return it == ws.end() ? nullptr : it->second;
    }

    int live()
    {
        std::lock_guard<std::mutex> lk(mu);
        return (int)ws.size();
    }

    void drop(const hpccg_hip_matrix* M)
    {
        W* w = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = ws.find(M);
            if (it == ws.end()) return;
            w = it->second;
            ws.erase(it);
        }
        (void)hipSetDevice(w->v.device);
        free_vectors(w);
        w->free_own_rest();
        if (w->h_ended) (void)hipHostFree(w->h_ended);
        if (w->ev0) (void)hipEventDestroy(w->ev0);
        if (w->ev1) (void)hipEventDestroy(w->ev1);
        delete w;
    }

    // The matrix's record (made on first use, with the destroy hook).
    int record(hpccg_hip_matrix* M, const MatrixView& v, W** out);
};

template <class W>
Registry<W> g_ws;

// the destroy hook (ctx: the matrix, the workspace's key; a no-op once released)
template <class W>
void on_matrix_destroy(void* ctx)
{
    g_ws<W>.drop(static_cast<const hpccg_hip_matrix*>(ctx));
}

template <class W>
int Registry<W>::record(hpccg_hip_matrix* M, const MatrixView& v, W** out)
{
    W* w = find(M);
    if (!w) {
        w = new W;
        {
            std::lock_guard<std::mutex> lk(mu);
            ws[M] = w;
        }
        w->v = v;
        const int rc = hpccg_hip_internal_on_destroy(M, on_matrix_destroy<W>, M);
        if (rc) {
            drop(M);
            return rc;
        }
    }
    w->v = v;
    *out = w;
    return 0;
}

// Room for ncols columns and a history of max_iter + 1 entries per column:
// kept where what is there suffices (and keep, the unit's own condition,
// holds), else everything is freed and allocated anew at the larger of the old
// and the new sizes. pcs: the unit's p column; ntot: totals per column (0:
// none); own(cap): allocates the unit's vectors, last.
template <class W, class Own>
int ensure_columns(W* w, int ncols, int max_iter, bool keep, long long pcs, int ntot, Own own)
{
    const MatrixView& v = w->v;
    HIP_TRY(hipSetDevice(v.device));
    if (!w->h_ended) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&w->h_ended), sizeof(int), hipHostMallocDefault));
    if (!w->ev0) HIP_TRY(hipEventCreate(&w->ev0));
    if (!w->ev1) HIP_TRY(hipEventCreate(&w->ev1));
    const long long hneed = (long long)max_iter + 1;
    if (ncols <= w->cap && hneed <= w->hstride && keep) return 0;
    const int cap = std::max(ncols, w->cap);
    const long long hstride = std::max(hneed, w->hstride);
    free_vectors(w);
    const size_t npad = (size_t)v.npad;
    const size_t ng = (size_t)(v.nslices + kGroup - 1) / kGroup;
    w->pcs = pcs;
    w->vcs = (long long)npad;
    // zeroed: p's guard zones and the rows past n are read (holes, full-width
    // loads) and never stored by a kernel
    int rc = alloc_zero(w, &w->pbuf, (size_t)pcs * cap);
    if (!rc) rc = alloc_zero(w, &w->Ap, npad * cap);
    if (!rc) rc = alloc_zero(w, &w->partial, (size_t)w->ndots * cap * std::max(v.nslices, 1));
    if (!rc) rc = alloc_zero(w, &w->gsum, (size_t)w->ndots * cap * std::max<size_t>(ng, 1));
    if (!rc && ntot) rc = alloc_zero(w, &w->tot, (size_t)ntot * cap);
    if (!rc) rc = alloc_zero(w, &w->st, (size_t)cap);
    if (!rc) rc = alloc_zero(w, &w->ended, 1);
    if (!rc) rc = alloc_zero(w, &w->hist, (size_t)cap * (size_t)hstride);
    if (!rc) rc = own(cap);
    if (rc) {
        free_vectors(w);
        return rc;
    }
    w->cap = cap;
    w->hstride = hstride;
    return 0;
}

// The shared fields of a unit's kernel arguments (p, r, x, b and their strides
// beyond pcs and vcs are the unit's).
void fill_args(ColArgs* a, const ColWorkspace* w, int nrhs)
{
    const MatrixView& v = w->v;
    a->n = v.n;
    a->nslices = v.nslices;
    a->grid = v.grid;
    a->nrhs = nrhs;
    a->cap = w->cap;
    a->ng = (v.nslices + kGroup - 1) / kGroup;
    a->nt = v.nt;
    a->a_width = v.a_width;
    a->xsell = v.sell_col_base;
    a->Ap = w->Ap;
    a->pcs = w->pcs;
    a->vcs = w->vcs;
    a->partial = w->partial;
    a->gsum = w->gsum;
    a->tot = w->tot;
    a->st = w->st;
    a->hist = w->hist;
    a->hstride = w->hstride;
    a->ended = w->ended;
    a->aoff = v.aoff;
    a->abase = v.abase;
    a->slice_base = v.slice_base;
    a->cols = v.cols;
}

// Columns [c0, c0 + kR) per launch: fours, a remainder of three as a four with
// one idle column (one pass over the matrix, not two), of two as a two, of one
// as a one where the unit has that instantiation (ones), else as a two.
template <class F>
void for_chunks(int nrhs, bool ones, F f)
{
    int c0 = 0;
    while (nrhs - c0 >= 3) {
        f(c0, 4);
        c0 += 4;
    }
    if (c0 < nrhs) f(c0, ones && nrhs - c0 == 1 ? 1 : 2);
}

// Columns between the caller's column-major array and the workspace (kind:
// host or device on the caller's side), stream-ordered.
int copy_cols(const ColWorkspace* w, double* dst, long long ldd, const double* src, long long lds, int nrhs,
              hipMemcpyKind kind)
{
    for (int c = 0; c < nrhs; c++)
        HIP_TRY(hipMemcpyAsync(dst + (size_t)c * (size_t)ldd, src + (size_t)c * (size_t)lds,
                               sizeof(double) * (size_t)w->v.n, kind, w->v.stream));
    return 0;
}

// One CG recurrence per running column of the states on the device, on (b, x)
// of a: the prologue, then iterations 1 .. kmax - 1, launched eagerly on the
// matrix's stream. Every kCheckEvery iterations the host reads the "columns
// ended" word and stops launching once the nrun columns that ran have ended.
template <class W, class A>
int run_recurrence(W* w, const A& a, int nrun, int kmax, void (*launch_p)(const W*, A, bool),
                   void (*launch_spmm)(const W*, A, bool), void (*launch_update)(const W*, A, bool),
                   void (*launch_finalize)(const W*, const A&, int, int))
{
    hipStream_t s = w->v.stream;
    launch_p(w, a, true);
    launch_spmm(w, a, true);
    launch_update(w, a, true);
    launch_finalize(w, a, kDotRR, 0);
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < kmax; k++) {
        launch_p(w, a, false);
        launch_spmm(w, a, false);
        launch_finalize(w, a, kDotPAP, 0);
        launch_update(w, a, false);
        launch_finalize(w, a, kDotRR, 0);
        if (k % kCheckEvery == 0 && k + 1 < kmax) {
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(w->h_ended, w->ended, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (*w->h_ended >= nrun) break;  // later launches would be no-ops for every column
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The columns' states and histories once the stream has run dry.
int read_columns(const ColWorkspace* w, int nrhs, std::vector<ColState>* st, std::vector<double>* hist)
{
    hipStream_t s = w->v.stream;
    st->resize(nrhs);
    hist->resize((size_t)nrhs * (size_t)w->hstride);
    HIP_TRY(hipMemcpyAsync(st->data(), w->st, sizeof(ColState) * nrhs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(hist->data(), w->hist, sizeof(double) * hist->size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// Iterations done by a column's recurrence, from its state and history h; its
// normr trace is appended to tr.
int column_trace(const ColState& st, const double* h, std::vector<double>* tr)
{
    // a column still running when the launches ran out did max_iter - 1 iterations
    const int it = st.run ? st.k - 1 : st.niters;
    // normr after iteration k is sqrt(r_{k-1}.r_{k-1}) (HPCCG.cpp:371): the single solve's trace
    tr->push_back(std::sqrt(h[0]));
    for (int k = 1; k <= it; k++) tr->push_back(std::sqrt(h[k - 1]));
    return it;
}

// The end of the recurrences on w's stream, after the last launch: their wall
// time since ev0, then every column's iterations, final normr and trace.
// (inline, as copy_trace: a unit with records of its own uses neither)
inline int finish_recurrence(TraceWorkspace* w, int nrhs, int* niters, double* normr, double* wall)
{
    HIP_TRY(hipEventRecord(w->ev1, w->v.stream));
    std::vector<ColState> st;
    std::vector<double> hist;
    TRY(read_columns(w, nrhs, &st, &hist));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, w->ev0, w->ev1));
    if (wall) *wall = 1e-3 * ms;
    w->trace.assign(nrhs, {});
    for (int c = 0; c < nrhs; c++) {
        niters[c] = column_trace(st[c], hist.data() + (size_t)c * (size_t)w->hstride, &w->trace[c]);
        normr[c] = w->trace[c][niters[c]];
    }
    return 0;
}

// The first cap entries of column col's trace into out: their number, or -1
// where the last solve kept no such column (w: the matrix's record, if any).
inline int copy_trace(const TraceWorkspace* w, int col, double* out, int cap)
{
    if (!w || col < 0 || col >= (int)w->trace.size()) return -1;
    const std::vector<double>& tr = w->trace[col];
    const int n = std::min<int>(std::max(cap, 0), (int)tr.size());
    for (int i = 0; i < n; i++) out[i] = tr[i];
    return n;
}

}  // namespace

}  // namespace hpccg
