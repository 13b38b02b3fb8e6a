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
// SpMM epilogue, the update and the finalize, the workspace registry, the
// launch loop and its read-back -- is hpccg_columns.h, the fp64 SpMM loops are
// hpccg_spmm.h; the matrix check and the bodies of the bookkeeping exports are
// hpccg_onerank_host.h; this unit adds its args, its launch dispatch (two and
// four columns only: one is forwarded to the main library) and a guarded r.
//
// Over an in-process rank group (include/hpccg_hip_batch_group.h; the last part
// of the host code): every member runs these kernels on its rows, the ghost
// planes of every column's p are copied between the members' p columns after
// k_batch_p, k_batch_finalize stores each member's local total only
// (store_total), and k_batch_group_sum adds the totals in rank order and
// advances the column's state on every member. Column c is bitwise
// hpccg_hip_group_solve of it. That engine -- the group, its checks, the guarded
// p column, the halo, the sum and the launch loop -- is hpccg_group.h, shared
// with hpccg_pcg_group.hip; here are the batch's launchers for it, what the
// batch forwards (one column, one member) and the group's SpMM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <vector>

#include "../../include/hpccg_hip_batch.h"
#include "../../include/hpccg_hip_batch_group.h"
#include "hpccg_group.h"
#include "hpccg_onerank_host.h"

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
    col_init(a, max_iter, tol);
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

// In-process group: the global dot and the column's state on every member
// (hpccg_group.h), on member 0's stream after every member's local finalize.
__global__ void k_batch_group_sum(BatchArgs a, GroupTotals g, int which)
{
    col_group_sum<false>(a, g, which);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct Workspace : TraceWorkspace, GroupMember {
    double *rbuf = nullptr, *x = nullptr, *b = nullptr;  // (r is guarded like p: stride pcs, local row 0 at p0)

    void free_own_vectors()
    {
        for (double* q : {rbuf, x, b})
            if (q) (void)hipFree(q);
        rbuf = x = b = nullptr;
    }
    void free_own_rest() { destroy_events(); }
    long long total_bytes() const { return bytes; }
};

// The matrix's workspace record with room for nrhs columns (ncols 0: the record
// only) and a history of max_iter + 1 entries per column.
int get_workspace(hpccg_hip_matrix* M, const MatrixView& v, int ncols, int max_iter, Workspace** out)
{
    TRY(g_ws<Workspace>.record(M, v, out));
    if (ncols <= 0) return 0;
    Workspace* w = *out;
    const size_t npad = (size_t)v.npad;
    const PColumn pc = guarded_p_column(v);
    // (r's guard zones and rows past n are read and never stored, as p's; p's
    // ghost rows are stored by the group's halo copies only)
    TRY(ensure_columns(w, ncols, max_iter, true, pc.pcs, v.in_group ? 2 : 0, [&](int cap) {
        w->p0 = pc.p0;
        TRY(alloc_zero(w, &w->rbuf, (size_t)pc.pcs * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        return 0;
    }));
    if (v.in_group) TRY(w->create_events());
    return 0;
}

// What hpccg_onerank_host.h's matrix check and bookkeeping bodies go by.
struct Batch {
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "batch";
    static constexpr const char* solve_name = "batch";
};

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

void launch_init(const Workspace* w, const BatchArgs& a, int max_iter, double tol)
{
    hipLaunchKernelGGL(k_batch_init, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, max_iter, tol);
}

// The batch CG on the columns staged in the workspace's b and x.
int run_cg(Workspace* w, int nrhs, int max_iter, double tol, int* niters, double* normr, double* wall)
{
    const BatchArgs a = make_args(w, nrhs);
    HIP_TRY(hipEventRecord(w->ev0, w->v.stream));
    launch_init(w, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p, launch_spmm, launch_update, launch_finalize));
    return finish_recurrence(w, nrhs, niters, normr, wall);
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
    TRY(check_matrix(Batch::who, M, &v, group1));
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
    TRY(check_matrix(Batch::who, M, &v, group1));
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
// order by k_batch_group_sum on member 0's stream. The engine is hpccg_group.h;
// here are the batch's launchers for it, its workspaces and what it forwards.
// ---------------------------------------------------------------------------
using BatchGroup = Group<Workspace, BatchArgs>;
constexpr const char* kGroupWho = "group batch";
// a group of one is the one-rank batch (solve_common, sparsemv_one), which checks its matrix itself
constexpr bool kOneForwarded = true;

void launch_group_sum(const Workspace* w, const BatchArgs& a, const GroupTotals& gt, int which)
{
    hipLaunchKernelGGL(k_batch_group_sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt, which);
}

// (halo null: the ghost planes move by copies, one per column and side)
constexpr GroupLaunch<Workspace, BatchArgs> kGroupLaunch = {launch_init,     launch_p,         launch_spmm, launch_update,
                                                            launch_finalize, launch_group_sum, nullptr};

int group_workspaces(hpccg_hip_matrix* const* Ms, BatchGroup* G, int nrhs, int max_iter)
{
    G->w.assign(G->P, nullptr);
    G->a.resize(G->P);
    for (int r = 0; r < G->P; r++) {
        TRY(get_workspace(Ms[r], G->v[r], nrhs, max_iter, &G->w[r]));
        G->a[r] = make_args(G->w[r], nrhs);
    }
    return 0;
}

int group_solve(hpccg_hip_matrix* const* Ms, const BatchGroup& G0, int nrhs, const double* const* B, const long long* ldb,
                double* const* X, const long long* ldx, int max_iter, double tol, int* niters, double* normr,
                double* times)
{
    BatchGroup G = G0;
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
    TRY(group_stage_in(G, nrhs, B, ldb, X, ldx));
    double wall = 0.0;
    TRY(group_run_cg(G, nrhs, max_iter, tol, kGroupLaunch, niters, normr, &wall));
    TRY(group_stage_out(G, nrhs, X, ldx));
    if (times) times[0] = wall;
    return 0;
}

int group_sparsemv(hpccg_hip_matrix* const* Ms, const BatchGroup& G0, int nrhs, const double* const* X,
                   const long long* ldx, double* const* Y, const long long* ldy)
{
    BatchGroup G = G0;
    TRY(group_workspaces(Ms, &G, nrhs, 1));
    // x into the local rows of the p columns, their halo, Ap = A p, Ap out
    for (int r = 0; r < G.P; r++) {
        G.a[r].force = 1;
        TRY(use(G, r));
        TRY(copy_cols(G.w[r], G.a[r].p, G.w[r]->pcs, X[r], ldx[r], nrhs, hipMemcpyDeviceToDevice));
    }
    TRY(group_halo(G, nrhs, nullptr));
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
    return unit_last_trace<Batch>(M, col, out, cap);
}

int hpccg_hip_batch_sparsemv(hpccg_hip_matrix* M, int nrhs, const double* X_dev, long long ldx, double* Y_dev,
                             long long ldy)
{
    return sparsemv_one(M, nrhs, X_dev, ldx, Y_dev, ldy, false);
}

int hpccg_hip_batch_release(hpccg_hip_matrix* M) { return unit_release<Batch>(M); }

int hpccg_hip_batch_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Batch>(M, bytes);
}

int hpccg_hip_batch_live_workspaces(int* count) { return unit_live_workspaces<Batch>(count); }

// ---- include/hpccg_hip_batch_group.h ---------------------------------------
int hpccg_hip_group_batch_abi_version(void) { return 1; }

int hpccg_hip_group_batch_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                       const long long* ldb, double* const* X_dev, const long long* ldx, int max_iter,
                                       double tolerance, int* niters, double* normr, double* times)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    TRY(check_group_columns(kGroupWho, nrhs, max_iter, B_dev, ldb, X_dev, ldx, niters, normr));
    for (int r = 0; r < nranks; r++)
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "group batch: B_dev[%d] or X_dev[%d] is NULL", r, r);
    BatchGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    TRY(check_group_lds(kGroupWho, G, ldb, ldx, "ldb, ldx"));
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
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "group batch: nrhs %d (at least 1)", nrhs);
    if (!X_dev || !ldx || !Y_dev || !ldy)
        return fail(HPCCG_HIP_EINVAL, "group batch: NULL argument (X_dev, ldx, Y_dev or ldy)");
    for (int r = 0; r < nranks; r++)
        if (!X_dev[r] || !Y_dev[r]) return fail(HPCCG_HIP_EINVAL, "group batch: X_dev[%d] or Y_dev[%d] is NULL", r, r);
    BatchGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    TRY(check_group_lds(kGroupWho, G, ldx, ldy, "ldx, ldy"));
    return keep_device([&] {
        if (nranks == 1) return sparsemv_one(Ms[0], nrhs, X_dev[0], ldx[0], Y_dev[0], ldy[0], true);
        return group_sparsemv(Ms, G, nrhs, X_dev, ldx, Y_dev, ldy);
    });
}

int hpccg_hip_group_batch_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "group batch: out is NULL");
    BatchGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    // one set of all-reduced scalars: kept with member 0's record
    return hpccg_hip_batch_last_trace(Ms[0], col, out, cap);
}

}  // extern "C"
