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
// exports are hpccg_onerank_host.h, shared with hpccg_pcg.hip; the member's
// workspace and preconditioner, the argument checks and the solve are
// hpccg_group_host.h, shared with hpccg_srcg_group.hip and the polynomial group
// units; this unit adds its args, its launch list and the diagonal's export.
// Ordering between the members is by stream events (group_halo and group_sum
// there). No kernel here waits on another block.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_pcg_group.h"
#include "hpccg_group_host.h"

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
// hpccg_group_host.h's and hpccg_onerank_host.h's host code over this unit's
// kernels; a member's workspace is GroupWorkspace as it stands
using Workspace = GroupWorkspace;

struct PcgGroupUnit {
    using Args = PcgArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "group pcg";
    // diagnostics: the halo by copies, the A/B of k_pcg_group_halo (tools/group_pcg_bench.py)
    static constexpr const char* halo_env = "HPCCG_GROUP_PCG_HALO_COPIES";
    static int own_vectors(Workspace*, size_t) { return 0; }
    static PcgArgs make_args(const Workspace* w, int nrhs, const double* m)
    {
        PcgArgs a{};
        fill_member_args(&a, w, nrhs, m);
        return a;
    }

    static constexpr auto init = k_pcg_group_init;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_pcg_group_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_pcg_group_spmm_sell<kR>;
    // (store_total: always 1 here, a member's part; the state is the group sum's)
    static constexpr auto finalize = k_pcg_group_finalize;
    static constexpr auto sum = k_pcg_group_sum;
    static constexpr auto halo = k_pcg_group_halo;
    static constexpr auto diag = k_pcg_group_diag;
    static constexpr auto check = k_pcg_group_check;
};
constexpr const char* kGroupWho = PcgGroupUnit::who;
using PcgGroup = GroupOf<PcgGroupUnit>;

void launch_p(const Workspace* w, PcgArgs a, bool prologue)
{
    launch_chunks(w, a, prologue, [](auto r) { return k_pcg_group_p<decltype(r)::value>; });
}

void launch_update(const Workspace* w, PcgArgs a, bool prologue)
{
    launch_chunks(w, a, prologue, [](auto r) { return k_pcg_group_update<decltype(r)::value>; });
}

// The group engine's loop over this unit's launchers (halo null: by copies).
int group_run_pcg(const PcgGroup& G, int nrhs, int max_iter, double tol, HaloLaunch halo, int* niters, double* normr,
                  double* wall)
{
    const GroupLaunch<Workspace, PcgArgs> launch = {launch_init<PcgGroupUnit>,
                                                    launch_p,
                                                    launch_spmm64<PcgGroupUnit>,
                                                    launch_update,
                                                    launch_finalize<PcgGroupUnit>,
                                                    launch_group_sum<PcgGroupUnit>,
                                                    halo};
    return group_run_cg(G, nrhs, max_iter, tol, launch, niters, normr, wall);
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
    return group_diag_solve_device<PcgGroupUnit>(Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter,
                                                 tolerance, niters, normr, times, group_run_pcg);
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
    return group_last_trace<PcgGroupUnit>(Ms, nranks, col, out, cap);
}

int hpccg_hip_group_pcg_release(hpccg_hip_matrix* M) { return unit_release<PcgGroupUnit>(M); }

int hpccg_hip_group_pcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<PcgGroupUnit>(M, bytes);
}

int hpccg_hip_group_pcg_live_workspaces(int* count) { return unit_live_workspaces<PcgGroupUnit>(count); }

}  // extern "C"
