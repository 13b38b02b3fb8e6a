// hpccg_srcg_group.hip -- single-reduction preconditioned CG over an in-process
// rank group (include/hpccg_hip_srcg_group.h, lib/libhpccg_hip_srcg_group.so):
// kernels and host code of the eleventh library.
//
// Member r is rank r of a z-slab job. Every member runs the Chronopoulos-Gear
// recurrence of hpccg_srcg.hip (the step and the finalize of
// hpccg_srcg_bodies.h, the SpMM bodies of hpccg_spmm.h, that library's launch
// bounds and plan choices) on its own rows, on its own stream, in a workspace
// of its own. An iteration carries one sum over the members where the group
// pcg's carries two:
//   step      k_srcg_group_step<kR>: p, s, x, r, u = m r and the r.u and r.r
//             slice partials (prologue: r = b - A t, u = m r), then the halo of
//             every column's u
//   SpMM      k_srcg_group_spmm_a<kW, kR, kWaves> | k_srcg_group_spmm_sell<kR>:
//             w = A u and the u.w slice partial
//   finalize  k_srcg_group_finalize with store_total: the member's local totals
//             of r.r, r.u and u.w
//   sum       k_srcg_group_sum on member 0's stream: each of the three totals
//             added in rank order from 0.0, one srcg_advance, the state stored
//             to every member
//   halo      k_srcg_group_halo: one launch per member moves the ghost planes
//             of all columns; the copy form is kept as the fallback and the
//             baseline
//   prologue  k_srcg_group_t<kR>: t = x + 0 x into u's buffer, then the halo of t
//   diagonal  k_srcg_group_diag | k_srcg_group_check: hpccg_jacobi.h's bodies,
//             per member, with no communication
// The group and its checks, the guarded u column, the bodies of the halo
// kernel, the halo, the ordering of the sum and the staging of B and X are
// hpccg_group.h; the dispatch of a launch on a chunk's columns and SpMM form
// and the bookkeeping exports are hpccg_onerank_host.h; this unit adds the sum
// kernel, the members' preconditioner and the launch loop. Ordering between the
// members is by stream events. No kernel here waits on another block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/hpccg_hip_srcg_group.h"
#include "hpccg_group.h"
#include "hpccg_onerank_host.h"
#include "hpccg_srcg_bodies.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// (SrcgArgs' p: u, a guard zone around each column, ghost_lo rows below row 0,
// ghost_hi rows from row n; xsell: -ghost_lo; minv: the member's m; tot: the
// member's local dot totals, [3][cap])

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_srcg_group_init(SrcgArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

// The prologue's t = x + 0.0*x, into u's buffer (col_p's prologue form; launched with no other).
template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_group_t(SrcgArgs a, bool prologue)
{
    col_p<kR, true>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_group_step(SrcgArgs a, bool prologue)
{
    srcg_step<kR>(a, prologue);
}

// The pcg library's plan choices (hpccg_pcg.hip): kWaves 5 for the 27-wide
// four-column form over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_srcg_group_spmm_a(
    SrcgArgs a, bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_srcg_group_spmm_sell(SrcgArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

// store_total: the three totals are this member's parts of the dots and the
// state is left to k_srcg_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_srcg_group_finalize(SrcgArgs a, int store_total)
{
    srcg_finalize(a, store_total);
}

// The group's three dots and the column's state on every member: one thread
// per column on member 0's stream, after every member's local finalize. Each
// dot is the members' local totals added in rank order from 0.0 (col_group_sum's
// sum); the column advances once, as in the one-rank finalize, and its state is
// stored into every member's state array, so all members freeze a column
// together. hist and the "columns ended" word are member 0's (a: its args).
__global__ void k_srcg_group_sum(SrcgArgs a, GroupTotals g)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nrhs) return;
    ColState s = a.st[c];
    if (!s.run) return;  // frozen on every member
    double rr = 0.0, gamma = 0.0, delta = 0.0;
    for (int r = 0; r < g.nranks; r++) rr += g.tot[r][(size_t)kDotRR * g.cap[r] + c];
    for (int r = 0; r < g.nranks; r++) gamma += g.tot[r][(size_t)kDotRZ * g.cap[r] + c];
    for (int r = 0; r < g.nranks; r++) delta += g.tot[r][(size_t)kDotPAP * g.cap[r] + c];
    srcg_advance(a, &s, c, rr, gamma, delta);
    for (int r = 0; r < g.nranks; r++) g.st[r][c] = s;
}

// The halo of every column's u (in the prologue: t) in one launch per member (hpccg_group.h).
__global__ __launch_bounds__(kHaloThreads) void k_srcg_group_halo(HaloArgs h)
{
    halo_body(h);
}

// The diagonal of a member's rows and the check of a caller's m: hpccg_jacobi.h's
// bodies (the view of a member with ghost rows is read like any other).
__global__ __launch_bounds__(kBlock) void k_srcg_group_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_srcg_group_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// One member's workspace: the columns (u's guarded, with the member's ghost
// planes), p and s, the cached 1 / a_ii with its verdict and a slot for a
// caller's m. The member's other workspaces are other records.
struct Workspace : TraceWorkspace, GroupMember, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;
    double *pd = nullptr, *sd = nullptr;  // p and s = A p (never zeroed again: k == 1 reads u and w)

    Workspace() { ndots = 3; }

    void free_own_vectors()
    {
        for (double* q : {r, x, b, pd, sd})
            if (q) (void)hipFree(q);
        r = x = b = pd = sd = nullptr;
    }
    void free_own_rest()
    {
        free_cache();
        destroy_events();
    }
    long long total_bytes() const { return bytes + rest_bytes; }
};

// The member's cache (hpccg_jacobi.h) and its two events.
int ensure_rest(Workspace* w)
{
    HIP_TRY(hipSetDevice(w->v.device));
    TRY(w->create_events());
    return ensure_cache(w);
}

// Jacobi on member r: the cached 1.0 / a_ii of its rows, from its own image, or
// the refusal of a member it does not exist for.
int ensure_jacobi(Workspace* w, int r)
{
    int row = -1;
    TRY(build_jacobi(w, k_srcg_group_diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "group srcg: Jacobi needs a finite diagonal > 0 in every row; on member %d row %d (local) is the "
                    "first whose diagonal is missing, not finite or <= 0",
                    r, row);
    return 0;
}

// A call's own m of member r: into the padded muser, every entry finite and > 0.
int stage_minv(Workspace* w, int r, const double* minv)
{
    int row = -1;
    TRY(load_minv(w, minv, hipMemcpyDeviceToDevice, k_srcg_group_check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "group srcg: member %d's minv[%d] is not finite and > 0 (the first such entry)", r,
                    row);
    return 0;
}

// Room for ncols columns (u's are guarded, with the ghost planes) and a
// history of max_iter + 1 entries per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter)
{
    const MatrixView& v = w->v;
    const size_t npad = (size_t)v.npad;
    const PColumn pc = guarded_p_column(v);
    return ensure_columns(w, ncols, max_iter, true, pc.pcs, 3, [&](int cap) {
        w->p0 = pc.p0;
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        TRY(alloc_zero(w, &w->pd, npad * cap));
        TRY(alloc_zero(w, &w->sd, npad * cap));
        return 0;
    });
}

SrcgArgs make_args(const Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    SrcgArgs a{};
    fill_args(&a, w, nrhs);  // (Ap: w = A u)
    a.tri = 1;
    a.p = w->pbuf + w->p0;  // u
    a.r = w->r;
    a.rcs = w->vcs;
    a.x = w->x;
    a.b = w->b;
    a.minv = m;
    a.aval = v.aval;
    a.vals = v.vals;
    a.pd = w->pd;
    a.sd = w->sd;
    return a;
}

// hpccg_onerank_host.h's launchers over this unit's kernels
struct SrcgGroupUnit {
    using Args = SrcgArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "group srcg";

    static constexpr auto init = k_srcg_group_init;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_srcg_group_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_srcg_group_spmm_sell<kR>;
};
constexpr const char* kGroupWho = SrcgGroupUnit::who;

void launch_t(const Workspace* w, const SrcgArgs& a)
{
    // (prologue: col_p's form)
    launch_chunks(w, a, true, [](auto r) { return k_srcg_group_t<decltype(r)::value>; });
}

void launch_step(const Workspace* w, const SrcgArgs& a, bool prologue)
{
    launch_chunks(w, a, prologue, [](auto r) { return k_srcg_group_step<decltype(r)::value>; });
}

// (store_total: always 1 here, a member's part; the state is the group sum's)
void launch_finalize(const Workspace* w, const SrcgArgs& a)
{
    hipLaunchKernelGGL(k_srcg_group_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, 1);
}

// (which: group_sum's; the one launch sums all three dots)
void launch_group_sum(const Workspace* w, const SrcgArgs& a, const GroupTotals& gt, int)
{
    hipLaunchKernelGGL(k_srcg_group_sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt);
}

void launch_halo(hipStream_t s, dim3 grid, const HaloArgs& h)
{
    hipLaunchKernelGGL(k_srcg_group_halo, grid, dim3(kHaloThreads), 0, s, h);
}

using SrcgGroup = Group<Workspace, SrcgArgs>;
// a group of one is checked and run like any other: nothing forwards it
constexpr bool kOneForwarded = false;

// Every member's stream waits for what its neighbours' streams hold so far.
// The prologue needs it once: a member's step overwrites the t rows its
// neighbours' halos read, with no group sum between the two (in the loop the
// sum is that fence: hpccg_group.h's argument for p, here for u).
int neighbour_fence(const SrcgGroup& G)
{
    if (G.P == 1) return 0;
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        if (r > 0) HIP_TRY(hipStreamWaitEvent(G.v[r].stream, G.w[r - 1]->evr, 0));
        if (r < G.P - 1) HIP_TRY(hipStreamWaitEvent(G.v[r].stream, G.w[r + 1]->evr, 0));
    }
    return 0;
}

// step, the halo of u, SpMM and finalize on every member, then the group's one sum.
int group_iteration(const SrcgGroup& G, int nrhs, bool prologue, HaloLaunch halo, const GroupTotals& gt,
                    const GroupLaunch<Workspace, SrcgArgs>& L)
{
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_step(G.w[r], G.a[r], prologue);
    }
    TRY(group_halo(G, nrhs, halo));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm64<SrcgGroupUnit>(G.w[r], G.a[r], false);
        launch_finalize(G.w[r], G.a[r]);
    }
    return group_sum(G, gt, kDotRR, L);
}

// The single-reduction CG over the group on the columns staged in the members'
// b and x: hpccg_srcg.hip's launch sequence on every member's stream, the halo
// after t and after every step, one sum after every finalize. Every
// kCheckEvery iterations the host reads member 0's "columns ended" word, as
// group_run_cg does.
int group_run_srcg(const SrcgGroup& G, int nrhs, int max_iter, double tol, HaloLaunch halo, int* niters,
                   double* normr, double* wall)
{
    GroupTotals gt{};
    gt.nranks = G.P;
    for (int r = 0; r < G.P; r++) {
        gt.cap[r] = G.w[r]->cap;
        gt.tot[r] = G.w[r]->tot;
        gt.st[r] = G.w[r]->st;
    }
    GroupLaunch<Workspace, SrcgArgs> L{};  // (group_sum takes the sum's launcher from it)
    L.sum = launch_group_sum;
    Workspace* w0 = G.w[0];
    TRY(use(G, 0));
    HIP_TRY(hipEventRecord(w0->ev0, G.v[0].stream));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_init<SrcgGroupUnit>(G.w[r], G.a[r], max_iter, tol);
        launch_t(G.w[r], G.a[r]);
    }
    TRY(group_halo(G, nrhs, halo));
    TRY(neighbour_fence(G));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm64<SrcgGroupUnit>(G.w[r], G.a[r], true);
    }
    TRY(group_iteration(G, nrhs, true, halo, gt, L));
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < max_iter; k++) {
        TRY(group_iteration(G, nrhs, false, halo, gt, L));
        if (k % kCheckEvery == 0 && k + 1 < max_iter) {
            HIP_TRY(hipGetLastError());
            TRY(use(G, 0));
            HIP_TRY(hipMemcpyAsync(w0->h_ended, w0->ended, sizeof(int), hipMemcpyDeviceToHost, G.v[0].stream));
            HIP_TRY(hipStreamSynchronize(G.v[0].stream));
            if (*w0->h_ended >= nrhs) break;  // every column is frozen on every member
        }
    }
    HIP_TRY(hipGetLastError());
    // the end on member 0's stream, whose last launch followed every member's
    TRY(use(G, 0));
    TRY(finish_recurrence(w0, nrhs, niters, normr, wall));
    for (int r = 1; r < G.P; r++) {  // (the last sum's event was their streams' last wait)
        TRY(use(G, r));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    return 0;
}

// copies: the halo by copies (the fallback and the baseline), else by k_srcg_group_halo.
int group_solve(hpccg_hip_matrix* const* Ms, const SrcgGroup& G0, int nrhs, const double* const* B,
                const long long* ldb, double* const* X, const long long* ldx, const double* const* minv, int max_iter,
                double tol, bool copies, int* niters, double* normr, double* times)
{
    SrcgGroup G = G0;
    if (times) std::fill(times, times + 7, 0.0);
    if (max_iter < 1) max_iter = 1;
    G.w.assign(G.P, nullptr);
    G.a.resize(G.P);
    // the preconditioner first, on every member: a refused one leaves every X as it is
    for (int r = 0; r < G.P; r++) {
        TRY(g_ws<Workspace>.record(Ms[r], G.v[r], &G.w[r]));
        TRY(ensure_rest(G.w[r]));
        if (minv)
            TRY(stage_minv(G.w[r], r, minv[r]));
        else
            TRY(ensure_jacobi(G.w[r], r));
    }
    for (int r = 0; r < G.P; r++) {
        Workspace* w = G.w[r];
        TRY(ensure_vectors(w, nrhs, max_iter));
        G.a[r] = make_args(w, nrhs, minv ? w->muser : w->jac);
    }
    TRY(group_stage_in(G, nrhs, B, ldb, X, ldx));
    double wall = 0.0;
    TRY(group_run_srcg(G, nrhs, max_iter, tol, copies ? nullptr : launch_halo, niters, normr, &wall));
    TRY(group_stage_out(G, nrhs, X, ldx));
    if (times) times[0] = wall;
    return 0;
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_group_srcg_abi_version(void) { return 1; }

int hpccg_hip_group_srcg_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                      const long long* ldb, double* const* X_dev, const long long* ldx,
                                      const double* const* minv_dev, int max_iter, double tolerance, int* niters,
                                      double* normr, double* times)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "group srcg: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "group srcg: max_iter %d is negative", max_iter);
    if (!B_dev || !ldb || !X_dev || !ldx || !niters || !normr)
        return fail(HPCCG_HIP_EINVAL, "group srcg: NULL argument (B_dev, ldb, X_dev, ldx, niters or normr)");
    for (int r = 0; r < nranks; r++) {
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "group srcg: B_dev[%d] or X_dev[%d] is NULL", r, r);
        if (minv_dev && !minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "group srcg: minv_dev[%d] is NULL", r);
    }
    SrcgGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    TRY(check_group_lds(kGroupWho, G, ldb, ldx, "ldb, ldx"));
    // diagnostics: the halo by copies, the A/B of k_srcg_group_halo (tools/group_srcg_bench.py)
    const bool copies = std::getenv("HPCCG_GROUP_SRCG_HALO_COPIES") != nullptr;
    return keep_device([&] {
        return group_solve(Ms, G, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, tolerance, copies, niters, normr,
                           times);
    });
}

int hpccg_hip_group_srcg_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "group srcg: out is NULL");
    SrcgGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    // one set of all-reduced scalars: kept with member 0's record
    const Workspace* w = g_ws<Workspace>.find(Ms[0]);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "group srcg: no trace of column %d (the last group solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

int hpccg_hip_group_srcg_release(hpccg_hip_matrix* M) { return unit_release<SrcgGroupUnit>(M); }

int hpccg_hip_group_srcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<SrcgGroupUnit>(M, bytes);
}

int hpccg_hip_group_srcg_live_workspaces(int* count) { return unit_live_workspaces<SrcgGroupUnit>(count); }

}  // extern "C"
