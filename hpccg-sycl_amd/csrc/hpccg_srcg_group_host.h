// hpccg_srcg_group_host.h -- the host code that the single-reduction group
// units share (hpccg_srcg_group.hip, hpccg_srpoly_group.hip): the body of their
// sum kernel, its launcher, the fence between neighbours and the launch loop
// of the Chronopoulos-Gear recurrence over an in-process rank group
// (group_iteration: the ordering argument is written there). It stands on
// hpccg_group_host.h (through it hpccg_group.h, the group engine: the halo, the
// ordering of the sum, the loop's frame) and hpccg_srcg_host.h (p and s, the
// launchers of t, the fused step and the finalize).
// A unit hands over one traits struct U: what those headers ask for and
//   sum                   its group sum kernel (srcg_group_sum below)
// and, as a SrcgGroupLaunch, what differs between the units.
// The __global__ entry points and the extern "C" definitions stay in the units.
// Internal linkage, like hpccg_columns.h.
#pragma once
#include "hpccg_group_host.h"
#include "hpccg_srcg_host.h"

namespace hpccg {

namespace {

// The group's three dots and the column's state on every member: one thread
// per column on member 0's stream, after every member's local finalize. Each
// dot is the members' local totals added in rank order from 0.0 (col_group_sum's
// sum); the column advances once, as in the one-rank finalize, and its state is
// stored into every member's state array, so all members freeze a column
// together. hist and the "columns ended" word are member 0's (a: its args).
__device__ __forceinline__ void srcg_group_sum(const ColArgs& a, const GroupTotals& g)
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

// (which: group_sum's; the one launch sums all three dots)
template <class U>
void launch_srcg_group_sum(const typename U::Workspace* w, const typename U::Args& a, const GroupTotals& gt, int)
{
    hipLaunchKernelGGL(U::sum, dim3((a.nrhs + 63) / 64), dim3(64), 0, w->v.stream, a, gt);
}

// Member r's p buffer: what the halo of u moves where u lives there.
template <class W, class A>
HaloBuf p_buf(const Group<W, A>& G, int r)
{
    return HaloBuf{G.a[r].p, G.a[r].pcs};
}

// Where the two units' launch loops differ.
//   spmm_u       a member's w = A u (the polynomial unit: u in p's place)
//   u_buf        member r's buffer of u, whose halo precedes that SpMM
//   fence        whether the prologue needs neighbour_fence
//   steps_group  (may be null: none) what the whole group runs between the
//                members' fused steps and the halo of u: the polynomial unit's
//                steps 1 .. d, each after the halo of the buffer it reads
template <class W, class A>
struct SrcgGroupLaunch {
    void (*spmm_u)(const W*, A, bool prologue);
    HaloBuf (*u_buf)(const Group<W, A>&, int r);
    bool fence;
    int (*steps_group)(const Group<W, A>&, int nrhs, HaloLaunch halo) = nullptr;
};

// Every member's stream waits for what its neighbours' streams hold so far.
// The prologue needs it once: a member's step overwrites the t rows its
// neighbours' halos read, with no group sum between the two (in the loop the
// sum is that fence: hpccg_group.h's argument for p, here for u). That is so
// wherever u shares p's buffer with t (the diagonal unit; the polynomial unit
// at degree 0); with d >= 1 nothing stores p's buffer after t and the fence is
// left out.
template <class W, class A>
int neighbour_fence(const Group<W, A>& G)
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

// ---------------------------------------------------------------------------
// One iteration: every member's fused step (the polynomial unit: step 0 into
// buffer 0), then for j = 1 .. d the halo of z buffer (j - 1) & 1 and every
// member's step j, which stores the member's own rows of buffer j & 1
// (S.steps_group; the diagonal unit has d = 0 and none); then the halo of
// u = z_d (buffer d & 1; degree 0: of p's buffer), every member's SpMM and
// finalize, and the group's one sum. Call the halo that follows step j halo j
// (j = 0 .. d; it moves buffer j & 1): d + 1 halos per iteration.
//
// Two buffers suffice, and no member's rows of a buffer are overwritten before
// every neighbour has pulled them:
//   - Halos 0 .. d - 1 and steps 1 .. d are hpccg_poly_group_host.h's
//     (group_poly_update): member r's halo j waits on the events its neighbours
//     record after their step j; the next store into those rows within the
//     iteration is the neighbour's step j + 2, which follows its halo j + 1,
//     which waits on r's event recorded after r's step j + 1, which follows r's
//     halo j on r's stream.
//   - Halo d moves u after step d. Nothing of this iteration stores buffer
//     d & 1 after step d: the SpMM and the finalize read only.
//   - The next iteration's fused step stores buffer 0 on every member, and its
//     step 1 buffer 1. Both follow the group's sum on every stream; the sum
//     waits for every member's finalize; every member's finalize follows all
//     its halos, halo d included, on its own stream. So every pull of either
//     buffer is over before the next iteration stores into it.
//   - The fused step reads the member's own rows of u = z_d before it stores
//     buffer 0 (for an even d the same rows, by the same thread); it follows
//     the member's SpMM, the last reader of u's ghost planes, on its stream.
//   - A member's ghost planes are stored by its halos and read by its steps and
//     its SpMM only, all on its stream.
// Frozen columns' planes move too; a frozen column's z is no longer stored.
// ---------------------------------------------------------------------------
template <class U>
int group_iteration(const GroupOf<U>& G, int nrhs, bool prologue, HaloLaunch halo, const GroupTotals& gt,
                    const GroupLaunch<typename U::Workspace, typename U::Args>& L,
                    const SrcgGroupLaunch<typename U::Workspace, typename U::Args>& S)
{
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_srcg_step<U>(G.w[r], G.a[r], prologue);
    }
    if (S.steps_group) TRY(S.steps_group(G, nrhs, halo));
    TRY(group_halo_of(G, nrhs, halo, [&](int r) { return S.u_buf(G, r); }));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        S.spmm_u(G.w[r], G.a[r], false);
        launch_srcg_finalize<U>(G.w[r], G.a[r], 1);
    }
    return group_sum(G, gt, kDotRR, L);
}

// The single-reduction CG over the group on the columns staged in the members'
// b and x: the one-rank launch sequence (hpccg_srcg_host.h) on every member's
// stream, the halo after t and after every step, one sum after every finalize.
// Every kCheckEvery iterations the host reads member 0's "columns ended" word,
// as group_run_cg does.
template <class U>
int group_run_srcg(const GroupOf<U>& G, int nrhs, int max_iter, double tol, HaloLaunch halo,
                   const SrcgGroupLaunch<typename U::Workspace, typename U::Args>& S, int* niters, double* normr,
                   double* wall)
{
    const GroupTotals gt = group_totals(G);
    GroupLaunch<typename U::Workspace, typename U::Args> L{};  // (group_sum takes the sum's launcher from it)
    L.sum = launch_srcg_group_sum<U>;
    TRY(use(G, 0));
    HIP_TRY(hipEventRecord(G.w[0]->ev0, G.v[0].stream));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_init<U>(G.w[r], G.a[r], max_iter, tol);
        launch_srcg_t<U>(G.w[r], G.a[r]);
    }
    TRY(group_halo(G, nrhs, halo));
    if (S.fence) TRY(neighbour_fence(G));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm64<U>(G.w[r], G.a[r], true);
    }
    TRY(group_iteration<U>(G, nrhs, true, halo, gt, L, S));
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < max_iter; k++) {
        TRY(group_iteration<U>(G, nrhs, false, halo, gt, L, S));
        if (k % kCheckEvery == 0 && k + 1 < max_iter) {
            bool ended = false;
            TRY(group_ended(G, nrhs, &ended));
            if (ended) break;
        }
    }
    return group_finish(G, nrhs, niters, normr, wall);
}

}  // namespace

}  // namespace hpccg
