// hpccg_group_host.h -- the host code shared by the group units whose members
// carry a diagonal preconditioner (hpccg_pcg_group.hip, hpccg_srcg_group.hip
// and, under hpccg_poly_group_host.h, hpccg_poly_group.hip and
// hpccg_poly32_group.hip): the members' records, events, caches and
// preconditioner with its refusals, the argument checks of solve_device, the
// staging around a unit's launch loop and the body of last_trace; for the two
// units without a polynomial (pcg, srcg) also the member's workspace, its
// vectors, the shared kernel arguments and the whole solve. The launch loop
// of the single-reduction group units is hpccg_srcg_group_host.h. It stands on
// hpccg_group.h (the group engine) and hpccg_onerank_host.h (the launch
// dispatch, the bookkeeping bodies).
// A unit hands over one traits struct U: Args, Workspace (a TraceWorkspace, a
// GroupMember and a JacobiCache with the staged columns b and x), init,
// spmm_a, spmm_sell (hpccg_onerank_host.h's) and
//   who                   the name in front of its messages ("group pcg")
//   halo_env              the environment variable of the halo by copies
//   halo, diag, check     its halo kernel and the preconditioner's kernels
//   sum                   its group sum kernel, where that takes `which`
// and pcg and srcg further
//   own_vectors(w, count)     allocates what its Workspace adds to r, x, b
//   make_args(w, nrhs, m)     its kernel arguments (fill_member_args and its own)
// The __global__ entry points, the Args types and the extern "C" definitions
// stay in the units. Internal linkage, like hpccg_columns.h.
#pragma once
#include <cstdlib>
#include <vector>

#include "hpccg_group.h"
#include "hpccg_onerank_host.h"

namespace hpccg {

namespace {

template <class U>
using GroupOf = Group<typename U::Workspace, typename U::Args>;

// a group of one is checked and run like any other: nothing forwards it
constexpr bool kOneForwarded = false;

// One member's workspace: the columns, the cached 1 / a_ii with its verdict and
// a slot for a caller's m. The member's own solve vectors and its workspaces
// in other units are other records.
struct GroupWorkspace : TraceWorkspace, GroupMember, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;

    GroupWorkspace() { ndots = 3; }

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

// Room for ncols columns (p's guarded, with the member's ghost planes) and a
// history of max_iter + 1 entries per column; own(w, count): the unit's vectors
// beside r, x and b, of count entries each.
template <class W>
int ensure_member_vectors(W* w, int ncols, int max_iter, int (*own)(W*, size_t))
{
    const PColumn pc = guarded_p_column(w->v);
    return ensure_columns(w, ncols, max_iter, true, pc.pcs, 3, [&](int cap) {
        const size_t count = (size_t)w->v.npad * cap;
        w->p0 = pc.p0;
        TRY(alloc_zero(w, &w->r, count));
        TRY(alloc_zero(w, &w->x, count));
        TRY(alloc_zero(w, &w->b, count));
        return own(w, count);
    });
}

// What the kernel arguments of pcg and srcg share (srcg: p is u, Ap is w = A u).
template <class A, class W>
void fill_member_args(A* a, const W* w, int nrhs, const double* m)
{
    fill_args(a, w, nrhs);
    a->tri = 1;
    a->p = w->pbuf + w->p0;
    a->r = w->r;
    a->rcs = w->vcs;
    a->x = w->x;
    a->b = w->b;
    a->minv = m;
    a->aval = w->v.aval;
    a->vals = w->v.vals;
}

// Jacobi on member r: the cached 1.0 / a_ii of its rows, from its own image, or
// the refusal of a member it does not exist for.
template <class U>
int ensure_member_jacobi(typename U::Workspace* w, int r)
{
    int row = -1;
    TRY(build_jacobi(w, U::diag, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL,
                    "%s: Jacobi needs a finite diagonal > 0 in every row; on member %d row %d (local) is the "
                    "first whose diagonal is missing, not finite or <= 0",
                    U::who, r, row);
    return 0;
}

// A call's own m of member r: into the padded muser, every entry finite and > 0.
template <class U>
int stage_member_minv(typename U::Workspace* w, int r, const double* minv)
{
    int row = -1;
    TRY(load_minv(w, minv, hipMemcpyDeviceToDevice, U::check, &row));
    if (row >= 0)
        return fail(HPCCG_HIP_EINVAL, "%s: member %d's minv[%d] is not finite and > 0 (the first such entry)", U::who, r,
                    row);
    return 0;
}

template <class U>
void launch_halo(hipStream_t s, dim3 grid, const HaloArgs& h)
{
    hipLaunchKernelGGL(U::halo, grid, dim3(kHaloThreads), 0, s, h);
}

template <class U>
void launch_group_sum(const typename U::Workspace* w, const typename U::Args& a, const GroupTotals& gt, int which)
{
    hipLaunchKernelGGL(U::sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt, which);
}

// diagnostics: the halos by copies, the A/B of the unit's halo kernel (the group benchmark tools)
template <class U>
HaloLaunch halo_launcher()
{
    return std::getenv(U::halo_env) ? nullptr : launch_halo<U>;
}

// The members' preparation, per member in this order: its record, what the
// unit builds before the preconditioner (prepare(w, r), may be null: the fp32
// unit's image, whose verdict comes first), its device, events and cache, what
// the unit keeps beside them (extra(w), may be null: the bound's vectors), then
// a caller's m or Jacobi. All of it before any X is touched: a refused
// preconditioner leaves every X as it is. m[r]: member r's padded device m
// (its muser, or its cached 1 / a_ii).
template <class U>
int group_members(hpccg_hip_matrix* const* Ms, GroupOf<U>* G, const double* const* minv,
                  std::vector<const double*>* m, int (*prepare)(typename U::Workspace*, int) = nullptr,
                  int (*extra)(typename U::Workspace*) = nullptr)
{
    G->w.assign(G->P, nullptr);
    m->assign(G->P, nullptr);
    for (int r = 0; r < G->P; r++) {
        TRY(g_ws<typename U::Workspace>.record(Ms[r], G->v[r], &G->w[r]));
        typename U::Workspace* w = G->w[r];
        if (prepare) TRY(prepare(w, r));
        HIP_TRY(hipSetDevice(w->v.device));
        TRY(w->create_events());
        TRY(ensure_cache(w));
        if (extra) TRY(extra(w));
        if (minv)
            TRY(stage_member_minv<U>(w, r, minv[r]));
        else
            TRY(ensure_member_jacobi<U>(w, r));
        (*m)[r] = minv ? w->muser : w->jac;
    }
    return 0;
}

// B and X in, the unit's launch loop run(&wall) on the staged columns, X out.
template <class W, class A, class Run>
int group_run_staged(const Group<W, A>& G, int nrhs, const double* const* B, const long long* ldb, double* const* X,
                     const long long* ldx, double* times, Run run)
{
    TRY(group_stage_in(G, nrhs, B, ldb, X, ldx));
    double wall = 0.0;
    TRY(run(&wall));
    TRY(group_stage_out(G, nrhs, X, ldx));
    if (times) times[0] = wall;
    return 0;
}

// ---------------------------------------------------------------------------
// The bodies of a unit's extern "C" functions
// ---------------------------------------------------------------------------
// solve_device: the argument checks, then solve(G, max_iter) with the caller's
// device kept, `times` zeroed and max_iter at least 1. handles_early: a NULL
// Ms[r] is refused beside member r's arrays (the polynomial units), else by
// check_group, after every array (pcg, srcg). own_checks(): the unit's own,
// after the arrays' and before the group's. Which of two faults a call reports
// is behaviour (tests/test_group_refusals_cpu.py).
template <class U, class Checks, class Solve>
int group_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                       const long long* ldb, double* const* X_dev, const long long* ldx,
                       const double* const* minv_dev, int max_iter, int* niters, double* normr, double* times,
                       bool handles_early, Checks own_checks, Solve solve)
{
    const char* who = U::who;
    TRY(check_group_args(who, Ms, nranks));
    TRY(check_group_columns(who, nrhs, max_iter, B_dev, ldb, X_dev, ldx, niters, normr));
    for (int r = 0; r < nranks; r++) {
        if (handles_early && !Ms[r]) return fail(HPCCG_HIP_EINVAL, "%s: Ms[%d] is NULL", who, r);
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "%s: B_dev[%d] or X_dev[%d] is NULL", who, r, r);
        if (minv_dev && !minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "%s: minv_dev[%d] is NULL", who, r);
    }
    TRY(own_checks());
    GroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    TRY(check_group_lds(who, G, ldb, ldx, "ldb, ldx"));
    return keep_device([&] {
        if (times) std::fill(times, times + 7, 0.0);
        G.a.resize(G.P);
        return solve(G, std::max(max_iter, 1));
    });
}

// pcg's and srcg's solve: the preconditioner on every member, then every
// member's vectors and arguments, then run, the unit's launch loop (halo null:
// the halo by copies, the fallback and the baseline).
template <class U>
int group_diag_solve_device(hpccg_hip_matrix* const* Ms, int nranks, int nrhs, const double* const* B_dev,
                            const long long* ldb, double* const* X_dev, const long long* ldx,
                            const double* const* minv_dev, int max_iter, double tolerance, int* niters, double* normr,
                            double* times,
                            int (*run)(const GroupOf<U>&, int nrhs, int max_iter, double tol, HaloLaunch halo,
                                       int* niters, double* normr, double* wall))
{
    return group_solve_device<U>(
        Ms, nranks, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, niters, normr, times, false, [] { return 0; },
        [&](GroupOf<U>& G, int kmax) -> int {
            const HaloLaunch halo = halo_launcher<U>();
            std::vector<const double*> m;
            TRY(group_members<U>(Ms, &G, minv_dev, &m));
            for (int r = 0; r < G.P; r++) {
                TRY(ensure_member_vectors(G.w[r], nrhs, kmax, U::own_vectors));
                G.a[r] = U::make_args(G.w[r], nrhs, m[r]);
            }
            return group_run_staged(G, nrhs, B_dev, ldb, X_dev, ldx, times, [&](double* wall) {
                return run(G, nrhs, kmax, tolerance, halo, niters, normr, wall);
            });
        });
}

template <class U>
int group_last_trace(hpccg_hip_matrix* const* Ms, int nranks, int col, double* out, int cap)
{
    const char* who = U::who;
    TRY(check_group_args(who, Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "%s: out is NULL", who);
    GroupOf<U> G;
    TRY(check_group(who, Ms, nranks, kOneForwarded, &G));
    // one set of all-reduced scalars: kept with member 0's record
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(Ms[0]);
    const int n = copy_trace(w, col, out, cap);
    if (n < 0)
        return fail(HPCCG_HIP_EINVAL, "%s: no trace of column %d (the last group solve had %d)", who, col,
                    w ? (int)w->trace.size() : 0);
    return n;
}

}  // namespace

}  // namespace hpccg
