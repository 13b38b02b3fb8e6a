// hpccg_pcg_group.hip -- diagonally preconditioned CG over an in-process rank
// group (include/hpccg_hip_pcg_group.h, lib/libhpccg_hip_pcg_group.so): kernels
// and host code of the fifth library.
//
// Member r is rank r of a z-slab job. Every member runs the preconditioned
// recurrence of hpccg_pcg.hip (the kPre bodies of hpccg_columns.h, the SpMM
// bodies of hpccg_spmm.h, that library's launch bounds and plan choices) on its
// own rows, on its own stream, in a workspace of its own:
//   p update  k_pcg_group_p<kR>, then the halo of every column's p
//   SpMM      k_pcg_group_spmm_a<kW, kR, kWaves> | k_pcg_group_spmm_sell<kR>
//   update    k_pcg_group_update<kR>: + the r.z and r.r slice partials
//   finalize  k_pcg_group_finalize with store_total: the member's local totals
//             (the r.r launch stores r.z's too)
//   sum       k_pcg_group_sum on member 0's stream: the totals added in rank
//             order from 0.0 (r.r and r.z in one launch), one advance_column,
//             the state stored to every member
//   halo      k_pcg_group_halo: one launch per member moves the ghost planes of
//             all columns (the group batch: one copy per column and side); the
//             copy form is kept as the fallback and the baseline
//   diagonal  k_pcg_group_diag | k_pcg_group_check: hpccg_jacobi.h's bodies,
//             per member. Jacobi needs no communication: a member's image
//             holds a_ii of each of its rows
// The group engine -- the group and its checks, the guarded p column, the
// bodies of the sum and halo kernels, the halo, the sum, the launch loop and
// the staging of B and X -- is hpccg_group.h, shared with hpccg_batch.hip; the
// dispatch of a launch on a chunk's columns and SpMM form and the bookkeeping
// exports are hpccg_onerank_host.h, shared with hpccg_pcg.hip; this unit adds
// its args, its sum and halo launchers and the members' preconditioner.
// Ordering between the members is by stream events (group_halo and group_sum
// there). No kernel here waits on another block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/hpccg_hip_pcg_group.h"
#include "hpccg_group.h"
#include "hpccg_onerank_host.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct PcgArgs : ColArgs {
    // (ColArgs' p: a guard zone around each column, ghost_lo rows below row 0,
    // ghost_hi rows from row n; xsell: -ghost_lo; minv: the member's m; tot:
    // the member's local dot totals, [3][cap])
    int tri;  // width 27: slices whose offsets come in runs of three use the x-triple plan
    const double* aval;
    const double* vals;
};

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_pcg_group_init(PcgArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_pcg_group_p(PcgArgs a, bool prologue)
{
    col_p<kR, true>(a, prologue);
}

// The pcg library's plan choices (hpccg_pcg.hip): kWaves 5 for the 27-wide
// four-column form over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_pcg_group_spmm_a(
    PcgArgs a, bool prologue)
{
    spmm_a_body<kW, kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_pcg_group_spmm_sell(PcgArgs a, bool prologue)
{
    spmm_sell_body<kR>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_pcg_group_update(PcgArgs a, bool prologue)
{
    col_update<kR, true>(a, prologue);
}

// store_total: the totals are this member's parts of the dots (the r.r launch:
// of r.r and of r.z) and the state is left to k_pcg_group_sum.
__global__ __launch_bounds__(kFinThreads) void k_pcg_group_finalize(PcgArgs a, int which, int store_total)
{
    col_finalize<true>(a, which, store_total);
}

// The group's dots and the column's state on every member (hpccg_group.h), on
// member 0's stream after every member's local finalize; the r.r launch sums
// r.r and r.z.
__global__ void k_pcg_group_sum(PcgArgs a, GroupTotals g, int which)
{
    col_group_sum<true>(a, g, which);
}

// The halo of every column's p in one launch per member (hpccg_group.h).
__global__ __launch_bounds__(kHaloThreads) void k_pcg_group_halo(HaloArgs h)
{
    halo_body(h);
}

// The diagonal of a member's rows and the check of a caller's m: hpccg_jacobi.h's
// bodies (the view of a member with ghost rows is read like any other).
__global__ __launch_bounds__(kBlock) void k_pcg_group_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_pcg_group_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// One member's workspace: the columns, the cached 1 / a_ii with its verdict and
// a slot for a caller's m. The member's own solve vectors and its batch and pcg
// workspaces are other records.
struct Workspace : TraceWorkspace, GroupMember, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;

    Workspace() { ndots = 3; }

    void free_own_vectors()
    {
        for (double* q : {r, x, b})
            if (q) (void)hipFree(q);
        r = x = b = nullptr;
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
    TRY(build_jacobi(w, k_pcg_group_diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "group pcg: Jacobi needs a finite diagonal > 0 in every row; on member %d row %d (local) is the "
                    "first whose diagonal is missing, not finite or <= 0",
                    r, row);
    return 0;
}

// A call's own m of member r: into the padded muser, every entry finite and > 0.
int stage_minv(Workspace* w, int r, const double* minv)
{
    int row = -1;
    TRY(load_minv(w, minv, hipMemcpyDeviceToDevice, k_pcg_group_check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "group pcg: member %d's minv[%d] is not finite and > 0 (the first such entry)", r,
                    row);
    return 0;
}

// Room for ncols columns and a history of max_iter + 1 entries per column.
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
        return 0;
    });
}

PcgArgs make_args(const Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    PcgArgs a{};
    fill_args(&a, w, nrhs);
    a.tri = 1;
    a.p = w->pbuf + w->p0;
    a.r = w->r;
    a.rcs = w->vcs;
    a.x = w->x;
    a.b = w->b;
    a.minv = m;
    a.aval = v.aval;
    a.vals = v.vals;
    return a;
}

// hpccg_onerank_host.h's launchers over this unit's kernels
struct PcgGroupUnit {
    using Args = PcgArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "group pcg";

    static constexpr auto init = k_pcg_group_init;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_pcg_group_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_pcg_group_spmm_sell<kR>;
    // (store_total: always 1 here, a member's part; the state is the group sum's)
    static constexpr auto finalize = k_pcg_group_finalize;
};
constexpr const char* kGroupWho = PcgGroupUnit::who;

void launch_p(const Workspace* w, PcgArgs a, bool prologue)
{
    launch_chunks(w, a, prologue, [](auto r) { return k_pcg_group_p<decltype(r)::value>; });
}

void launch_update(const Workspace* w, PcgArgs a, bool prologue)
{
    launch_chunks(w, a, prologue, [](auto r) { return k_pcg_group_update<decltype(r)::value>; });
}

void launch_group_sum(const Workspace* w, const PcgArgs& a, const GroupTotals& gt, int which)
{
    hipLaunchKernelGGL(k_pcg_group_sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt, which);
}

void launch_halo(hipStream_t s, dim3 grid, const HaloArgs& h)
{
    hipLaunchKernelGGL(k_pcg_group_halo, grid, dim3(kHaloThreads), 0, s, h);
}

using PcgGroup = Group<Workspace, PcgArgs>;
// a group of one is checked and run like any other: nothing forwards it
constexpr bool kOneForwarded = false;

// copies: the halo by copies (the fallback and the baseline), else by k_pcg_group_halo.
int group_solve(hpccg_hip_matrix* const* Ms, const PcgGroup& G0, int nrhs, const double* const* B, const long long* ldb,
                double* const* X, const long long* ldx, const double* const* minv, int max_iter, double tol,
                bool copies, int* niters, double* normr, double* times)
{
    PcgGroup G = G0;
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
    const GroupLaunch<Workspace, PcgArgs> launch = {launch_init<PcgGroupUnit>,
                                                    launch_p,
                                                    launch_spmm64<PcgGroupUnit>,
                                                    launch_update,
                                                    launch_finalize<PcgGroupUnit>,
                                                    launch_group_sum,
                                                    copies ? nullptr : launch_halo};
    double wall = 0.0;
    TRY(group_run_cg(G, nrhs, max_iter, tol, launch, niters, normr, &wall));
    TRY(group_stage_out(G, nrhs, X, ldx));
    if (times) times[0] = wall;
    return 0;
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_group_pcg_abi_version(void) { return 1; }

int hpccg_hip_group_pcg_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                                     const long long* ldb, double* const* X_dev, const long long* ldx,
                                     const double* const* minv_dev, int max_iter, double tolerance, int* niters,
                                     double* normr, double* times)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "group pcg: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "group pcg: max_iter %d is negative", max_iter);
    if (!B_dev || !ldb || !X_dev || !ldx || !niters || !normr)
        return fail(HPCCG_HIP_EINVAL, "group pcg: NULL argument (B_dev, ldb, X_dev, ldx, niters or normr)");
    for (int r = 0; r < nranks; r++) {
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "group pcg: B_dev[%d] or X_dev[%d] is NULL", r, r);
        if (minv_dev && !minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "group pcg: minv_dev[%d] is NULL", r);
    }
    PcgGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    TRY(check_group_lds(kGroupWho, G, ldb, ldx, "ldb, ldx"));
    // diagnostics: the halo by copies, the A/B of k_pcg_group_halo (tools/group_pcg_bench.py)
    const bool copies = std::getenv("HPCCG_GROUP_PCG_HALO_COPIES") != nullptr;
    return keep_device([&] {
        return group_solve(Ms, G, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, tolerance, copies, niters, normr,
                           times);
    });
}

int hpccg_hip_group_pcg_diagonal(hpccg_hip_matrix* const* Ms, int nranks, double* const* d_dev)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (!d_dev) return fail(HPCCG_HIP_EINVAL, "group pcg: d_dev is NULL");
    for (int r = 0; r < nranks; r++)
        if (!d_dev[r]) return fail(HPCCG_HIP_EINVAL, "group pcg: d_dev[%d] is NULL", r);
    PcgGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    return keep_device([&]() -> int {
        for (int r = 0; r < nranks; r++) {
            const MatrixView& v = G.v[r];
            TRY(use(G, r));
            hipLaunchKernelGGL(k_pcg_group_diag, dim3(v.nslices), dim3(kBlock), 0, v.stream, diag_args(v), d_dev[r],
                               (double*)nullptr, (int*)nullptr);
            HIP_TRY(hipGetLastError());
        }
        for (int r = 0; r < nranks; r++) {
            TRY(use(G, r));
            HIP_TRY(hipStreamSynchronize(G.v[r].stream));
        }
        return 0;
    });
}

int hpccg_hip_group_pcg_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    TRY(check_group_args(kGroupWho, Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "group pcg: out is NULL");
    PcgGroup G;
    TRY(check_group(kGroupWho, Ms, nranks, kOneForwarded, &G));
    // one set of all-reduced scalars: kept with member 0's record
    const Workspace* w = g_ws<Workspace>.find(Ms[0]);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "group pcg: no trace of column %d (the last group solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

int hpccg_hip_group_pcg_release(hpccg_hip_matrix* M) { return unit_release<PcgGroupUnit>(M); }

int hpccg_hip_group_pcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<PcgGroupUnit>(M, bytes);
}

int hpccg_hip_group_pcg_live_workspaces(int* count) { return unit_live_workspaces<PcgGroupUnit>(count); }

}  // extern "C"
