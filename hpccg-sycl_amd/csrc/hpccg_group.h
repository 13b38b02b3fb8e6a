// hpccg_group.h -- the column recurrence of hpccg_columns.h over an in-process
// rank group, shared by the group solvers (hpccg_batch.hip, hpccg_pcg_group.hip,
// hpccg_srcg_group.hip, hpccg_poly_group.hip, hpccg_poly32_group.hip).
// Member r is rank r of a z-slab job: it runs its unit's kernels on its own
// rows, on its own stream, in a workspace of its own; the ghost planes of every
// column's p move between the members after the p update, each member's
// finalize stores its local totals only (store_total), and one sum kernel on
// member 0's stream adds them in rank order and advances the column's state on
// every member. Ordering between the members is by stream events; no kernel
// waits on another block.
//   device  GroupTotals and the body of the sum kernel; HaloArgs and the body
//           of the halo kernel. The __global__ entry points are the units'.
//   host    Group, its checks, the guarded p column of a member, the members'
//           events, the halo of any guarded column buffer (by copies or by the
//           unit's kernel), the sum, the launch loop of the group's recurrence
//           with its hook for a unit's own update phase, and the staging of B
//           and X.
// A unit keeps what differs: its args and make_args, its Workspace's vectors,
// its launch dispatch. Internal linkage, like hpccg_columns.h.
#pragma once
#include <cstdint>

#include "hpccg_columns.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

constexpr int kMaxMembers = kMaxGroupRanks;

// ---------------------------------------------------------------------------
// The group's dots: one thread per column on member 0's stream, after every
// member's local finalize. A dot is the members' local totals added in rank
// order from 0.0 (k_group_sum's sum in hpccg_kernels.hip); kPre: the r.r launch
// sums r.r and r.z. The column advances once, as in the unit's finalize, and
// its state is stored into every member's state array (peer pointers across
// devices), so all members freeze a column together. hist and the "columns
// ended" word are member 0's (a: its args).
// ---------------------------------------------------------------------------
struct GroupTotals {
    int nranks;
    int cap[kMaxMembers];            // stride of member r's totals
    const double* tot[kMaxMembers];  // member r's [2][cap] local totals (preconditioned: [3][cap])
    ColState* st[kMaxMembers];       // member r's column states
};

template <bool kPre>
__device__ __forceinline__ void col_group_sum(const ColArgs& a, const GroupTotals& g, int which)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nrhs) return;
    ColState s = a.st[c];
    if (!s.run) return;  // frozen on every member
    double v = 0.0;
    for (int r = 0; r < g.nranks; r++) v += g.tot[r][(size_t)which * g.cap[r] + c];
    double rz = v;
    if constexpr (kPre) {
        if (which == kDotRR) {
            rz = 0.0;
            for (int r = 0; r < g.nranks; r++) rz += g.tot[r][(size_t)kDotRZ * g.cap[r] + c];
        }
    }
    advance_column(a, &s, c, which, rz, v);
    for (int r = 0; r < g.nranks; r++) g.st[r][c] = s;
}

// ---------------------------------------------------------------------------
// The halo of every column's p in one launch per member: blockIdx.y is the
// column, the first blocks_lo blocks of x copy the lower ghost plane (the lower
// neighbour's last rows), the rest the upper one (the upper neighbour's first
// rows, to local row n on). The neighbours' p columns are read through their
// pointers (one device: plain loads; across devices: the peer mapping). vec: a
// thread moves 16 bytes (source and destination of every column 16-byte
// aligned; an odd plane's last row alone), else one double. A pure copy: the
// bits of the copy form.
// ---------------------------------------------------------------------------
constexpr int kHaloThreads = 256;

struct HaloArgs {
    int blocks_lo;
    int cnt_lo, cnt_hi;  // rows of the planes
    int vec_lo, vec_hi;
    double* dst_lo;      // column 0 of this member's ghost rows
    double* dst_hi;
    const double* src_lo;  // column 0 of the neighbour's boundary rows
    const double* src_hi;
    long long dcs;             // this member's p column stride
    long long scs_lo, scs_hi;  // the neighbours'
};

__device__ __forceinline__ void halo_body(const HaloArgs& h)
{
    const bool hi = (int)blockIdx.x >= h.blocks_lo;  // (block-uniform)
    const int blk = hi ? (int)blockIdx.x - h.blocks_lo : (int)blockIdx.x;
    const int cnt = hi ? h.cnt_hi : h.cnt_lo;
    const bool vec = (hi ? h.vec_hi : h.vec_lo) != 0;
    const long long c = blockIdx.y;
    double* __restrict__ d = (hi ? h.dst_hi : h.dst_lo) + c * h.dcs;
    const double* __restrict__ s = hi ? h.src_hi + c * h.scs_hi : h.src_lo + c * h.scs_lo;
    const int i = blk * kHaloThreads + (int)threadIdx.x;
    if (vec) {
        const int e = 2 * i;
        if (e + 1 < cnt)
            *reinterpret_cast<d2v*>(d + e) = *reinterpret_cast<const d2v*>(s + e);
        else if (e < cnt)
            d[e] = s[e];
    } else if (i < cnt) {
        d[i] = s[i];
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// W: the unit's Workspace (a ColWorkspace and a GroupMember with the staged
// columns b and x, stride vcs); A: its kernel arguments (a ColArgs).
template <class W, class A>
struct Group {
    int P = 0;
    std::vector<MatrixView> v;
    std::vector<W*> w;
    std::vector<A> a;
};

// What a member's workspace holds for the group, beside its columns.
struct GroupMember {
    long long p0 = 0;  // local row 0 inside a guarded column (guard zone + the padded ghost_lo rows)
    hipEvent_t evr = nullptr, evs = nullptr;  // this member's stream is ready | member 0: the sum is done

    // (on the member's device; before the first halo or sum)
    int create_events()
    {
        if (!evr) HIP_TRY(hipEventCreateWithFlags(&evr, hipEventDisableTiming));
        if (!evs) HIP_TRY(hipEventCreateWithFlags(&evs, hipEventDisableTiming));
        return 0;
    }
    void destroy_events()
    {
        if (evr) (void)hipEventDestroy(evr);
        if (evs) (void)hipEventDestroy(evs);
    }
};

// A member's p column: [guard | ghost_lo (padded) | local rows (padded) |
// ghost_hi's spill (padded) | guard], pcs rows with local row 0 at p0. The
// ghost_hi rows start at local row n (where the single solve's p has them):
// inside the last slice's padding rows and, past npad, in ghi_pad. glo_pad is
// whole slices, so local row 0 keeps the buffer's alignment. The ghost rows are
// stored by the halo only; a matrix without ghost rows has the guards alone.
struct PColumn {
    long long pcs, p0;
};

PColumn guarded_p_column(const MatrixView& v)
{
    const size_t glo_pad = ((size_t)v.ghost_lo + kSliceRows - 1) / kSliceRows * kSliceRows;
    const size_t ghi_pad = v.ghost_hi ? ((size_t)v.ghost_hi + 2 + kSliceRows - 1) / kSliceRows * kSliceRows : 0;
    return {(long long)((size_t)v.npad + glo_pad + ghi_pad + 2 * (size_t)v.guard_rows),
            (long long)((size_t)v.guard_rows + glo_pad)};
}

// who: the unit's message prefix ("group batch", "group pcg").
int check_group_args(const char* who, hpccg_hip_matrix* const* Ms, int nranks)
{
    if (!Ms) return fail(HPCCG_HIP_EINVAL, "%s: Ms is NULL", who);
    if (nranks < 1 || nranks > kMaxMembers)
        return fail(HPCCG_HIP_EINVAL, "%s: nranks %d (1 to %d members)", who, nranks, kMaxMembers);
    return 0;
}

// What every unit's solve_device checks next: the counts, then the arrays as such.
int check_group_columns(const char* who, int nrhs, int max_iter, const void* B_dev, const void* ldb, const void* X_dev,
                        const void* ldx, const void* niters, const void* normr)
{
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "%s: nrhs %d (at least 1)", who, nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "%s: max_iter %d is negative", who, max_iter);
    if (!B_dev || !ldb || !X_dev || !ldx || !niters || !normr)
        return fail(HPCCG_HIP_EINVAL, "%s: NULL argument (B_dev, ldb, X_dev, ldx, niters or normr)", who);
    return 0;
}

// The whole group in rank order, z-slab plan, a device image on every member.
// one_forwarded: the caller hands a group of one to a one-rank path that checks
// its matrix itself, so the members' own checks are left to it. Reads the
// matrices' records only: no device work.
template <class W, class A>
int check_group(const char* who, hpccg_hip_matrix* const* Ms, int nranks, bool one_forwarded, Group<W, A>* G)
{
    G->P = nranks;
    G->v.resize(nranks);
    for (int r = 0; r < nranks; r++) {
        if (!Ms[r]) return fail(HPCCG_HIP_EINVAL, "%s: Ms[%d] is NULL", who, r);
        TRY(hpccg_hip_internal_view(Ms[r], &G->v[r]));
        const MatrixView& v = G->v[r];
        if (v.nranks != nranks || v.rank != r || (nranks > 1 && !v.in_group))
            return fail(HPCCG_HIP_EINVAL, "%s: Ms[%d] is not rank %d of a %d-rank in-process group", who, r, r, nranks);
        if (nranks > 1 && v.group_id != G->v[0].group_id)
            return fail(HPCCG_HIP_EINVAL, "%s: Ms[%d] is a member of another group than Ms[0]", who, r);
    }
    if (nranks == 1 && one_forwarded) return 0;
    for (int r = 0; r < nranks; r++) {
        const MatrixView& v = G->v[r];
        if (v.general)
            return fail(HPCCG_HIP_EPLAN, "%s: member %d uses the gather plan (z-slab plan members only)", who, r);
        // the halo below relies on these (hpccg_slab_plan made them so)
        const int lo_max = r > 0 ? G->v[r - 1].n : 0, hi_max = r < nranks - 1 ? G->v[r + 1].n : 0;
        if (v.ghost_lo < 0 || v.ghost_hi < 0 || v.ghost_lo > lo_max || v.ghost_hi > hi_max)
            return fail(HPCCG_HIP_EPLAN, "%s: member %d's ghost rows (%d, %d) are not its neighbours' rows", who, r,
                        v.ghost_lo, v.ghost_hi);
        if (v.n <= 0) return fail(HPCCG_HIP_EINVAL, "%s: member %d has no rows", who, r);
        if (!v.has_a && !v.has_sell) return fail(HPCCG_HIP_EINVAL, "%s: member %d holds no device image", who, r);
    }
    return 0;
}

template <class W, class A>
int check_group_lds(const char* who, const Group<W, A>& G, const long long* l0, const long long* l1, const char* what)
{
    for (int r = 0; r < G.P; r++)
        if (l0[r] < G.v[r].n || l1[r] < G.v[r].n)
            return fail(HPCCG_HIP_EINVAL, "%s: member %d's leading dimensions (%s) %lld, %lld below its %d rows", who, r,
                        what, l0[r], l1[r], G.v[r].n);
    return 0;
}

template <class W, class A>
int use(const Group<W, A>& G, int r)
{
    HIP_TRY(hipSetDevice(G.v[r].device));
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

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// A unit's launch of its halo kernel (halo_body) on a member's stream.
using HaloLaunch = void (*)(hipStream_t, dim3 grid, const HaloArgs&);

// Column 0 of a guarded column buffer of a member (guarded_p_column's layout:
// its local row 0) and the buffer's column stride.
struct HaloBuf {
    double* p;
    long long cs;
};

// The halo of every column of one guarded column buffer per member, buf(r)
// being member r's (group_halo in hpccg_solver.cpp, per column): member r's
// ghost_lo rows are member r - 1's last rows, its ghost_hi rows (from local row
// n) member r + 1's first, moved on r's stream once the neighbours' streams
// have stored them (their events): by one launch of the unit's halo kernel, or
// (launch_halo null) by copies, one per column and side. Frozen columns' planes
// move too (their vectors no longer change: harmless). What keeps a neighbour
// from overwriting its rows before they have been read here is the caller's to
// argue (group_halo below: p; hpccg_poly_group_host.h: the two z buffers).
template <class W, class A, class Buf>
int group_halo_of(const Group<W, A>& G, int nrhs, HaloLaunch launch_halo, Buf buf)
{
    if (G.P == 1) return 0;
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    for (int r = 0; r < G.P; r++) {
        const MatrixView& v = G.v[r];
        const HaloBuf a = buf(r);
        const bool lo = r > 0 && v.ghost_lo, hi = r < G.P - 1 && v.ghost_hi;
        if (!lo && !hi) continue;
        TRY(use(G, r));
        HaloArgs h{};
        h.dcs = a.cs;
        if (lo) {
            const HaloBuf l = buf(r - 1);
            HIP_TRY(hipStreamWaitEvent(v.stream, G.w[r - 1]->evr, 0));
            h.cnt_lo = v.ghost_lo;
            h.dst_lo = a.p - v.ghost_lo;
            h.src_lo = l.p + (G.v[r - 1].n - v.ghost_lo);
            h.scs_lo = l.cs;
        }
        if (hi) {
            const HaloBuf u = buf(r + 1);
            HIP_TRY(hipStreamWaitEvent(v.stream, G.w[r + 1]->evr, 0));
            h.cnt_hi = v.ghost_hi;
            h.dst_hi = a.p + v.n;
            h.src_hi = u.p;
            h.scs_hi = u.cs;
        }
        if (!launch_halo) {
            for (int c = 0; lo && c < nrhs; c++)
                TRY(member_copy(v, h.dst_lo + (long long)c * h.dcs, G.v[r - 1], h.src_lo + (long long)c * h.scs_lo,
                                (size_t)h.cnt_lo));
            for (int c = 0; hi && c < nrhs; c++)
                TRY(member_copy(v, h.dst_hi + (long long)c * h.dcs, G.v[r + 1], h.src_hi + (long long)c * h.scs_hi,
                                (size_t)h.cnt_hi));
            continue;
        }
        // (the column strides are whole slices: column 0's alignment is every column's)
        h.vec_lo = lo && aligned16(h.dst_lo) && aligned16(h.src_lo) && h.dcs % 2 == 0 && h.scs_lo % 2 == 0;
        h.vec_hi = hi && aligned16(h.dst_hi) && aligned16(h.src_hi) && h.dcs % 2 == 0 && h.scs_hi % 2 == 0;
        const int items_lo = h.vec_lo ? (h.cnt_lo + 1) / 2 : h.cnt_lo;
        const int items_hi = h.vec_hi ? (h.cnt_hi + 1) / 2 : h.cnt_hi;
        h.blocks_lo = (items_lo + kHaloThreads - 1) / kHaloThreads;
        const int blocks_hi = (items_hi + kHaloThreads - 1) / kHaloThreads;
        launch_halo(v.stream, dim3(h.blocks_lo + blocks_hi, nrhs), h);
    }
    return 0;
}

// The halo of every column's p after the p update.
// p is one buffer per column, not a ring. A neighbour cannot overwrite its p
// before it has been read here: its next p update follows the group sum of p.Ap
// (in the prologue: of r.r) on its stream, that sum waits for every member's
// SpMM, and each member's SpMM follows its halo on its own stream.
template <class W, class A>
int group_halo(const Group<W, A>& G, int nrhs, HaloLaunch launch_halo)
{
    return group_halo_of(G, nrhs, launch_halo, [&](int r) { return HaloBuf{G.a[r].p, G.a[r].pcs}; });
}

// The launchers of a unit's kernels, as run_recurrence takes them, with those
// of the group's own: init and sum (col_init's and col_group_sum's kernels, one
// thread per column) and the halo kernel (null: the halo by copies).
// update_group (may be null: every member launches `update`): the whole group's
// update phase, for a unit whose update exchanges ghost planes of its own
// between the members' launches (hpccg_poly_group.hip: the steps and the halos
// of z); it leaves every member's update launched on its stream.
template <class W, class A>
struct GroupLaunch {
    void (*init)(const W*, const A&, int max_iter, double tol);
    void (*p)(const W*, A, bool);
    void (*spmm)(const W*, A, bool);
    void (*update)(const W*, A, bool);
    void (*finalize)(const W*, const A&, int which, int store_total);
    void (*sum)(const W*, const A&, const GroupTotals&, int which);
    HaloLaunch halo;
    int (*update_group)(const Group<W, A>&, int nrhs, bool prologue, HaloLaunch halo) = nullptr;
};

// The update phase of every member, each on its own stream.
template <class W, class A>
int group_update(const Group<W, A>& G, int nrhs, bool prologue, const GroupLaunch<W, A>& L)
{
    if (L.update_group) return L.update_group(G, nrhs, prologue, L.halo);
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        L.update(G.w[r], G.a[r], prologue);
    }
    return 0;
}

// The global dots `which` of every running column and its state on every
// member: member 0's stream waits for every member's local finalize, runs the
// unit's sum kernel, and the other members' streams wait for it.
template <class W, class A>
int group_sum(const Group<W, A>& G, const GroupTotals& gt, int which, const GroupLaunch<W, A>& L)
{
    for (int r = 1; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    TRY(use(G, 0));
    hipStream_t s0 = G.v[0].stream;
    for (int r = 1; r < G.P; r++) HIP_TRY(hipStreamWaitEvent(s0, G.w[r]->evr, 0));
    L.sum(G.w[0], G.a[0], gt, which);
    if (G.P == 1) return 0;
    HIP_TRY(hipEventRecord(G.w[0]->evs, s0));
    for (int r = 1; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipStreamWaitEvent(G.v[r].stream, G.w[0]->evs, 0));
    }
    return 0;
}

// The frame of a unit's launch loop over the group (group_run_cg below,
// group_run_srcg in hpccg_srcg_group_host.h).
// What the sum kernel reads and stores on the members.
template <class W, class A>
GroupTotals group_totals(const Group<W, A>& G)
{
    GroupTotals gt{};
    gt.nranks = G.P;
    for (int r = 0; r < G.P; r++) {
        gt.cap[r] = G.w[r]->cap;
        gt.tot[r] = G.w[r]->tot;
        gt.st[r] = G.w[r]->st;
    }
    return gt;
}

// Every kCheckEvery iterations the host reads member 0's "columns ended" word
// (the sum kernel keeps it): ended once every column is frozen on every member.
template <class W, class A>
int group_ended(const Group<W, A>& G, int nrhs, bool* ended)
{
    W* w0 = G.w[0];
    HIP_TRY(hipGetLastError());
    TRY(use(G, 0));
    HIP_TRY(hipMemcpyAsync(w0->h_ended, w0->ended, sizeof(int), hipMemcpyDeviceToHost, G.v[0].stream));
    HIP_TRY(hipStreamSynchronize(G.v[0].stream));
    *ended = *w0->h_ended >= nrhs;
    return 0;
}

// The end of the solve on member 0's stream, whose last launch followed every
// member's; then the other members' streams run dry.
template <class W, class A>
int group_finish(const Group<W, A>& G, int nrhs, int* niters, double* normr, double* wall)
{
    HIP_TRY(hipGetLastError());
    TRY(use(G, 0));
    TRY(finish_recurrence(G.w[0], nrhs, niters, normr, wall));
    for (int r = 1; r < G.P; r++) {  // (the last sum's event was their streams' last wait)
        TRY(use(G, r));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    return 0;
}

// The unit's CG over the group on the columns staged in the members' b and x:
// run_recurrence's launch sequence on every member's stream, the halo after
// every p update and the group's sum after every finalize.
template <class W, class A>
int group_run_cg(const Group<W, A>& G, int nrhs, int max_iter, double tol, const GroupLaunch<W, A>& L, int* niters,
                 double* normr, double* wall)
{
    const GroupTotals gt = group_totals(G);
    TRY(use(G, 0));
    HIP_TRY(hipEventRecord(G.w[0]->ev0, G.v[0].stream));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        L.init(G.w[r], G.a[r], max_iter, tol);
        L.p(G.w[r], G.a[r], true);
    }
    TRY(group_halo(G, nrhs, L.halo));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        L.spmm(G.w[r], G.a[r], true);
    }
    TRY(group_update(G, nrhs, true, L));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        L.finalize(G.w[r], G.a[r], kDotRR, 1);
    }
    TRY(group_sum(G, gt, kDotRR, L));
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < max_iter; k++) {
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            L.p(G.w[r], G.a[r], false);
        }
        TRY(group_halo(G, nrhs, L.halo));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            L.spmm(G.w[r], G.a[r], false);
            L.finalize(G.w[r], G.a[r], kDotPAP, 1);
        }
        TRY(group_sum(G, gt, kDotPAP, L));
        TRY(group_update(G, nrhs, false, L));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            L.finalize(G.w[r], G.a[r], kDotRR, 1);
        }
        TRY(group_sum(G, gt, kDotRR, L));
        if (k % kCheckEvery == 0 && k + 1 < max_iter) {
            bool ended = false;
            TRY(group_ended(G, nrhs, &ended));
            if (ended) break;
        }
    }
    return group_finish(G, nrhs, niters, normr, wall);
}

// The callers' B and X (device arrays, one per member) into the members' b and x.
template <class W, class A>
int group_stage_in(const Group<W, A>& G, int nrhs, const double* const* B, const long long* ldb,
                   const double* const* X, const long long* ldx)
{
    for (int r = 0; r < G.P; r++) {
        W* w = G.w[r];
        TRY(use(G, r));
        TRY(copy_cols(w, w->b, w->vcs, B[r], ldb[r], nrhs, hipMemcpyDeviceToDevice));
        TRY(copy_cols(w, w->x, w->vcs, X[r], ldx[r], nrhs, hipMemcpyDeviceToDevice));
    }
    return 0;
}

// The members' x into the callers' X, every member's stream run dry.
template <class W, class A>
int group_stage_out(const Group<W, A>& G, int nrhs, double* const* X, const long long* ldx)
{
    for (int r = 0; r < G.P; r++) {
        W* w = G.w[r];
        TRY(use(G, r));
        TRY(copy_cols(w, X[r], ldx[r], w->x, w->vcs, nrhs, hipMemcpyDeviceToDevice));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    return 0;
}

}  // namespace

}  // namespace hpccg
