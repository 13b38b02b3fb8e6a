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
// The recurrence itself -- the column's state, the bodies of the p update, the
// SpMM epilogue, the update and the finalize, the workspace registry and the
// launch loop -- is hpccg_columns.h, the fp64 SpMM loops are hpccg_spmm.h; this
// unit adds the guarded p / r layout and the group.
//
// Over an in-process rank group (include/hpccg_hip_batch_group.h; the last part
// of the host code): every member runs these kernels on its rows, the ghost
// planes of every column's p are copied between the members' p columns after
// k_batch_p, k_batch_finalize stores each member's local total only
// (store_total), and k_batch_group_sum adds the totals in rank order and
// advances the column's state on every member. Column c is bitwise
// hpccg_hip_group_solve of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <vector>

#include "../../include/hpccg_hip_batch.h"
#include "../../include/hpccg_hip_batch_group.h"
#include "hpccg_columns.h"
#include "hpccg_spmm.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct BatchArgs : ColArgs {
    // (ColArgs' p and r: guard zones around each column; a group member:
    // ghost_lo rows below row 0, ghost_hi rows from row n; xsell: -ghost_lo;
    // tot: a group member's local dot totals)
    int tri;  // width 27: slices whose offsets come in runs of three use the x-triple plan
    const double* aval;
    const double* vals;
};

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_batch_init(BatchArgs a, int max_iter, double tol)
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

template <int kR>
__global__ __launch_bounds__(kBlock) void k_batch_p(BatchArgs a, bool prologue)
{
    col_p<kR>(a, prologue);
}

// The SpMM loops are hpccg_spmm.h's (shared with hpccg_pcg.hip); the entry
// points set the launch shape.
// kWaves: the occupancy the kernel is compiled for (waves per SIMD). The
// 27-wide four-column form exists twice: at 5 (92 VGPRs) for images streamed
// from HBM and at 4 (102) for images the Infinity Cache holds -- same box,
// against the sequential solves: 200^3 1.59x at 5 and 1.52x at 4, 100^3 1.30x
// at 5 and 1.38x at 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_batch_spmm_a(BatchArgs a,
                                                                                                     bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_batch_spmm_sell(BatchArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_batch_update(BatchArgs a, bool prologue)
{
    col_update<kR>(a, prologue);
}

// store_total (a member of an in-process group): the total is this member's
// part of the dot and the state is left to k_batch_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_batch_finalize(BatchArgs a, int which, int store_total)
{
    col_finalize(a, which, store_total);
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
    advance_column(a, &s, c, which, v, v);
    for (int r = 0; r < g.nranks; r++) g.st[r][c] = s;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct Workspace : ColWorkspace {
    double *rbuf = nullptr, *x = nullptr, *b = nullptr;  // (r is guarded like p: stride pcs)
    long long p0 = 0;  // local row 0 inside a p / r column (guard zone + the padded ghost_lo rows)
    hipEvent_t evr = nullptr, evs = nullptr;  // group: this member's stream is ready | member 0: the sum is done
    std::vector<std::vector<double>> trace;   // per column of the last batch solve

    void free_own_vectors()
    {
        for (double* q : {rbuf, x, b})
            if (q) (void)hipFree(q);
        rbuf = x = b = nullptr;
    }
    void free_own_rest()
    {
        if (evr) (void)hipEventDestroy(evr);
        if (evs) (void)hipEventDestroy(evs);
    }
};

// The matrix's workspace record with room for nrhs columns (ncols 0: the record
// only) and a history of max_iter + 1 entries per column.
int get_workspace(hpccg_hip_matrix* M, const MatrixView& v, int ncols, int max_iter, Workspace** out)
{
    TRY(g_ws<Workspace>.record(M, v, out));
    if (ncols <= 0) return 0;
    Workspace* w = *out;
    const size_t npad = (size_t)v.npad;
    // a p column: [guard | ghost_lo (padded) | local rows (padded) | ghost_hi's spill (padded) | guard].
    // The ghost_hi rows start at local row n (where the single solve's p has
    // them): inside the last slice's padding rows and, past npad, in ghi_pad.
    // glo_pad is whole slices, so local row 0 keeps the buffer's alignment.
    const size_t glo_pad = ((size_t)v.ghost_lo + kSliceRows - 1) / kSliceRows * kSliceRows;
    const size_t ghi_pad = v.ghost_hi ? ((size_t)v.ghost_hi + 2 + kSliceRows - 1) / kSliceRows * kSliceRows : 0;
    const long long pcs = (long long)(npad + glo_pad + ghi_pad + 2 * (size_t)v.guard_rows);
    // (r's guard zones and rows past n are read and never stored, as p's; p's
    // ghost rows are stored by the group's halo copies only)
    TRY(ensure_columns(w, ncols, max_iter, true, pcs, v.in_group ? 2 : 0, [&](int cap) {
        w->p0 = (long long)((size_t)v.guard_rows + glo_pad);
        TRY(alloc_zero(w, &w->rbuf, (size_t)pcs * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        return 0;
    }));
    if (v.in_group && !w->evr) HIP_TRY(hipEventCreateWithFlags(&w->evr, hipEventDisableTiming));
    if (v.in_group && !w->evs) HIP_TRY(hipEventCreateWithFlags(&w->evs, hipEventDisableTiming));
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

BatchArgs make_args(const Workspace* w, int nrhs)
{
    const MatrixView& v = w->v;
    BatchArgs a{};
    fill_args(&a, w, nrhs);
    a.tri = std::getenv("HPCCG_BATCH_NO_TRIPLES") ? 0 : 1;  // diagnostics: A/B of the x-triple plan
    a.p = w->pbuf + w->p0;
    a.r = w->rbuf + w->p0;
    a.rcs = w->pcs;
    a.x = w->x;
    a.b = w->b;
    a.aval = v.aval;
    a.vals = v.vals;
    return a;
}

void launch_spmm(const Workspace* w, BatchArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, false, [&](int c0, int R) {
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
    for_chunks(a.nrhs, false, [&](int c0, int R) {
        a.c0 = c0;
        if (R == 4)
            hipLaunchKernelGGL(k_batch_p<4>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
        else
            hipLaunchKernelGGL(k_batch_p<2>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
    });
}

void launch_update(const Workspace* w, BatchArgs a, bool prologue)
{
    for_chunks(a.nrhs, false, [&](int c0, int R) {
        a.c0 = c0;
        if (R == 4)
            hipLaunchKernelGGL(k_batch_update<4>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
        else
            hipLaunchKernelGGL(k_batch_update<2>, dim3(a.grid), dim3(kBlock), 0, w->v.stream, a, prologue);
    });
}

void launch_finalize(const Workspace* w, const BatchArgs& a, int which, int store_total = 0)
{
    hipLaunchKernelGGL(k_batch_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, store_total);
}

int read_results(Workspace* w, int nrhs, int* niters, double* normr, double* wall);

// The batch CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    hipStream_t s = w->v.stream;
    const BatchArgs a = make_args(w, nrhs);
    HIP_TRY(hipEventRecord(w->ev0, s));
    hipLaunchKernelGGL(k_batch_init, dim3((nrhs + 63) / 64), dim3(64), 0, s, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p, launch_spmm, launch_update, launch_finalize));
    return read_results(w, nrhs, niters, normr, wall);
}

// The end of a batch CG on w's stream (a group: member 0's, whose last launch
// followed every member's): its wall time, the columns' states and traces.
int read_results(Workspace* w, int nrhs, int* niters, double* normr, double* wall)
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
    BatchArgs a = make_args(w, nrhs);
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

int group_workspaces(hpccg_hip_matrix* const* Ms, Group* G, int nrhs, int max_iter)
{
    G->w.assign(G->P, nullptr);
    G->a.resize(G->P);
    for (int r = 0; r < G->P; r++) {
        TRY(get_workspace(Ms[r], G->v[r], nrhs, max_iter, &G->w[r]));
        G->a[r] = make_args(G->w[r], nrhs);
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
int group_run_cg(const Group& G, int nrhs, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    GroupTotals gt{};
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
        hipLaunchKernelGGL(k_batch_init, dim3((nrhs + 63) / 64), dim3(64), 0, G.v[r].stream, G.a[r], max_iter, tol);
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
    TRY(group_workspaces(Ms, &G, nrhs, max_iter));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        TRY(copy_cols(G.w[r], G.w[r]->b, G.w[r]->vcs, B[r], ldb[r], nrhs, hipMemcpyDeviceToDevice));
        TRY(copy_cols(G.w[r], G.w[r]->x, G.w[r]->vcs, X[r], ldx[r], nrhs, hipMemcpyDeviceToDevice));
    }
    double wall = 0.0;
    TRY(group_run_cg(G, nrhs, max_iter, tol, niters, normr, &wall));
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
    TRY(group_workspaces(Ms, &G, nrhs, 1));
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
    const Workspace* w = g_ws<Workspace>.find(M);
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
    g_ws<Workspace>.drop(M);
    return 0;
}

int hpccg_hip_batch_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    *bytes = w ? w->bytes : 0;
    return 0;
}

int hpccg_hip_batch_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "batch: NULL argument");
    *count = g_ws<Workspace>.live();
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
