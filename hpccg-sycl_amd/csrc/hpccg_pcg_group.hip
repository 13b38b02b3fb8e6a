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
//             order from 0.0 (k_batch_group_sum's sum; r.r and r.z in one
//             launch), one advance_column, the state stored to every member
//   halo      k_pcg_group_halo: one launch per member moves the ghost planes of
//             all columns (the group batch: one copy per column and side); the
//             copy form is kept as the fallback and the baseline
//   diagonal  k_pcg_group_diag | k_pcg_group_check: hpccg_jacobi.h's bodies,
//             per member. Jacobi needs no communication: a member's image
//             holds a_ii of each of its rows
// Ordering between the members is by stream events (group_halo's and
// group_sum's of hpccg_batch.hip). No kernel here waits on another block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/hpccg_hip_pcg_group.h"
#include "hpccg_columns.h"
#include "hpccg_jacobi.h"
#include "hpccg_spmm.h"

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

// ---------------------------------------------------------------------------
// The group's dots: one thread per column on member 0's stream, after every
// member's local finalize. A dot is the members' local totals added in rank
// order from 0.0 (k_batch_group_sum's sum); the r.r launch sums r.r and r.z.
// The column advances once and its state is stored into every member's state
// array (peer pointers across devices), so all members freeze a column
// together. hist and the "columns ended" word are member 0's (a: its args).
// ---------------------------------------------------------------------------
constexpr int kMaxMembers = kMaxGroupRanks;

struct GroupTotals {
    int nranks;
    int cap[kMaxMembers];            // stride of member r's totals
    const double* tot[kMaxMembers];  // member r's [3][cap] local totals
    ColState* st[kMaxMembers];       // member r's column states
};

__global__ void k_pcg_group_sum(PcgArgs a, GroupTotals g, int which)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nrhs) return;
    ColState s = a.st[c];
    if (!s.run) return;  // frozen on every member
    double v = 0.0;
    for (int r = 0; r < g.nranks; r++) v += g.tot[r][(size_t)which * g.cap[r] + c];
    double rz = v;
    if (which == kDotRR) {
        rz = 0.0;
        for (int r = 0; r < g.nranks; r++) rz += g.tot[r][(size_t)kDotRZ * g.cap[r] + c];
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

__global__ __launch_bounds__(kHaloThreads) void k_pcg_group_halo(HaloArgs h)
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
struct Workspace : ColWorkspace, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;
    long long p0 = 0;  // local row 0 inside a p column (guard zone + the padded ghost_lo rows)
    hipEvent_t evr = nullptr, evs = nullptr;  // this member's stream is ready | member 0: the sum is done
    std::vector<std::vector<double>> trace;  // member 0's: per column of the last solve

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
        if (evr) (void)hipEventDestroy(evr);
        if (evs) (void)hipEventDestroy(evs);
    }
};

struct Group {
    int P = 0;
    std::vector<MatrixView> v;
    std::vector<Workspace*> w;
    std::vector<PcgArgs> a;
};

// The whole group in rank order, z-slab plan, a device image on every member
// (check_group of hpccg_batch.hip; a group of one is checked like any other:
// nothing forwards it). Reads the matrices' records only: no device work.
int check_group(hpccg_hip_matrix* const* Ms, int nranks, Group* G)
{
    G->P = nranks;
    G->v.resize(nranks);
    for (int r = 0; r < nranks; r++) {
        if (!Ms[r]) return fail(HPCCG_HIP_EINVAL, "group pcg: Ms[%d] is NULL", r);
        TRY(hpccg_hip_internal_view(Ms[r], &G->v[r]));
        const MatrixView& v = G->v[r];
        if (v.nranks != nranks || v.rank != r || (nranks > 1 && !v.in_group))
            return fail(HPCCG_HIP_EINVAL, "group pcg: Ms[%d] is not rank %d of a %d-rank in-process group", r, r,
                        nranks);
        if (nranks > 1 && v.group_id != G->v[0].group_id)
            return fail(HPCCG_HIP_EINVAL, "group pcg: Ms[%d] is a member of another group than Ms[0]", r);
    }
    for (int r = 0; r < nranks; r++) {
        const MatrixView& v = G->v[r];
        if (v.general)
            return fail(HPCCG_HIP_EPLAN, "group pcg: member %d uses the gather plan (z-slab plan members only)", r);
        // the halo below relies on these (hpccg_slab_plan made them so)
        const int lo_max = r > 0 ? G->v[r - 1].n : 0, hi_max = r < nranks - 1 ? G->v[r + 1].n : 0;
        if (v.ghost_lo < 0 || v.ghost_hi < 0 || v.ghost_lo > lo_max || v.ghost_hi > hi_max)
            return fail(HPCCG_HIP_EPLAN, "group pcg: member %d's ghost rows (%d, %d) are not its neighbours' rows", r,
                        v.ghost_lo, v.ghost_hi);
        if (v.n <= 0) return fail(HPCCG_HIP_EINVAL, "group pcg: member %d has no rows", r);
        if (!v.has_a && !v.has_sell) return fail(HPCCG_HIP_EINVAL, "group pcg: member %d holds no device image", r);
    }
    return 0;
}

int check_group_args(hpccg_hip_matrix* const* Ms, int nranks)
{
    if (!Ms) return fail(HPCCG_HIP_EINVAL, "group pcg: Ms is NULL");
    if (nranks < 1 || nranks > kMaxMembers)
        return fail(HPCCG_HIP_EINVAL, "group pcg: nranks %d (1 to %d members)", nranks, kMaxMembers);
    return 0;
}

int use(const Group& G, int r)
{
    HIP_TRY(hipSetDevice(G.v[r].device));
    return 0;
}

// The member's cache (hpccg_jacobi.h) and its two events.
int ensure_rest(Workspace* w)
{
    HIP_TRY(hipSetDevice(w->v.device));
    if (!w->evr) HIP_TRY(hipEventCreateWithFlags(&w->evr, hipEventDisableTiming));
    if (!w->evs) HIP_TRY(hipEventCreateWithFlags(&w->evs, hipEventDisableTiming));
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
    // a p column (get_workspace of hpccg_batch.hip): [guard | ghost_lo (padded) |
    // local rows (padded) | ghost_hi's spill (padded) | guard]. The ghost_hi
    // rows start at local row n: inside the last slice's padding rows and, past
    // npad, in ghi_pad. glo_pad is whole slices, so local row 0 keeps the
    // buffer's alignment. The ghost rows are stored by the halo only.
    const size_t glo_pad = ((size_t)v.ghost_lo + kSliceRows - 1) / kSliceRows * kSliceRows;
    const size_t ghi_pad = v.ghost_hi ? ((size_t)v.ghost_hi + 2 + kSliceRows - 1) / kSliceRows * kSliceRows : 0;
    const long long pcs = (long long)(npad + glo_pad + ghi_pad + 2 * (size_t)v.guard_rows);
    return ensure_columns(w, ncols, max_iter, true, pcs, 3, [&](int cap) {
        w->p0 = (long long)((size_t)v.guard_rows + glo_pad);
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

#define HPCCG_PCG_R(KERNEL, ...)                                                           \
    do {                                                                                   \
        if (R == 4)                                                                        \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 4>), g, b, 0, s, a, prologue);          \
        else if (R == 2)                                                                   \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 2>), g, b, 0, s, a, prologue);          \
        else                                                                               \
            hipLaunchKernelGGL((KERNEL<__VA_ARGS__ 1>), g, b, 0, s, a, prologue);          \
    } while (0)

void launch_spmm(const Workspace* w, PcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            HPCCG_PCG_R(k_pcg_group_spmm_sell, );
        else if (a.a_width == 27 && R == 4 && a.nt)
            hipLaunchKernelGGL((k_pcg_group_spmm_a<27, 4, 5>), g, b, 0, s, a, prologue);
        else if (a.a_width == 27)
            HPCCG_PCG_R(k_pcg_group_spmm_a, 27, );
        else if (a.a_width == 7)
            HPCCG_PCG_R(k_pcg_group_spmm_a, 7, );
        else
            HPCCG_PCG_R(k_pcg_group_spmm_a, 0, );
    });
}

void launch_p(const Workspace* w, PcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_PCG_R(k_pcg_group_p, );
    });
}

void launch_update(const Workspace* w, PcgArgs a, bool prologue)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        HPCCG_PCG_R(k_pcg_group_update, );
    });
}
#undef HPCCG_PCG_R

// (always a member's part: the state is the group sum's)
void launch_finalize(const Workspace* w, const PcgArgs& a, int which)
{
    hipLaunchKernelGGL(k_pcg_group_finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, which, 1);
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

// The halo of every column's p: member r's ghost_lo rows are member r - 1's
// last rows, its ghost_hi rows (from local row n) member r + 1's first, moved
// on r's stream once the neighbours' streams have stored them (their events),
// by one k_pcg_group_halo launch or, copies: by group_halo's copies of
// hpccg_batch.hip, one per column and side. Frozen columns' planes move too
// (their p no longer changes: harmless).
// p is one buffer per column, not a ring. A neighbour cannot overwrite its p
// before it has been read here: its next p update follows the group sum of p.Ap
// (in the prologue: of r.r) on its stream, that sum waits for every member's
// SpMM, and each member's SpMM follows its halo on its own stream.
int group_halo(const Group& G, int nrhs, bool copies)
{
    if (G.P == 1) return 0;
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    for (int r = 0; r < G.P; r++) {
        const MatrixView& v = G.v[r];
        const PcgArgs& a = G.a[r];
        const bool lo = r > 0 && v.ghost_lo, hi = r < G.P - 1 && v.ghost_hi;
        if (!lo && !hi) continue;
        TRY(use(G, r));
        HaloArgs h{};
        h.dcs = a.pcs;
        if (lo) {
            const PcgArgs& l = G.a[r - 1];
            HIP_TRY(hipStreamWaitEvent(v.stream, G.w[r - 1]->evr, 0));
            h.cnt_lo = v.ghost_lo;
            h.dst_lo = a.p - v.ghost_lo;
            h.src_lo = l.p + (l.n - v.ghost_lo);
            h.scs_lo = l.pcs;
        }
        if (hi) {
            const PcgArgs& u = G.a[r + 1];
            HIP_TRY(hipStreamWaitEvent(v.stream, G.w[r + 1]->evr, 0));
            h.cnt_hi = v.ghost_hi;
            h.dst_hi = a.p + a.n;
            h.src_hi = u.p;
            h.scs_hi = u.pcs;
        }
        if (copies) {
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
        hipLaunchKernelGGL(k_pcg_group_halo, dim3(h.blocks_lo + blocks_hi, nrhs), dim3(kHaloThreads), 0, v.stream, h);
    }
    return 0;
}

// The global dots of every running column and its state on every member:
// member 0's stream waits for every member's local finalize, runs
// k_pcg_group_sum, and the other members' streams wait for it.
int group_sum(const Group& G, const GroupTotals& gt, int which, int nrhs)
{
    for (int r = 1; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipEventRecord(G.w[r]->evr, G.v[r].stream));
    }
    TRY(use(G, 0));
    hipStream_t s0 = G.v[0].stream;
    for (int r = 1; r < G.P; r++) HIP_TRY(hipStreamWaitEvent(s0, G.w[r]->evr, 0));
    hipLaunchKernelGGL(k_pcg_group_sum, dim3((nrhs + 63) / 64), dim3(64), 0, s0, G.a[0], gt, which);
    if (G.P == 1) return 0;
    HIP_TRY(hipEventRecord(G.w[0]->evs, s0));
    for (int r = 1; r < G.P; r++) {
        TRY(use(G, r));
        HIP_TRY(hipStreamWaitEvent(G.v[r].stream, G.w[0]->evs, 0));
    }
    return 0;
}

// The preconditioned CG over the group on the columns staged in the members' b
// and x. copies: the halo by copies (the fallback and the baseline).
int group_run_cg(const Group& G, int nrhs, int max_iter, double tol, bool copies, int* niters, double* normr,
                 double* wall)
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
        hipLaunchKernelGGL(k_pcg_group_init, dim3((nrhs + 63) / 64), dim3(64), 0, G.v[r].stream, G.a[r], max_iter,
                           tol);
        launch_p(G.w[r], G.a[r], true);
    }
    TRY(group_halo(G, nrhs, copies));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        launch_spmm(G.w[r], G.a[r], true);
        launch_update(G.w[r], G.a[r], true);
        launch_finalize(G.w[r], G.a[r], kDotRR);
    }
    TRY(group_sum(G, gt, kDotRR, nrhs));
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < max_iter; k++) {
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_p(G.w[r], G.a[r], false);
        }
        TRY(group_halo(G, nrhs, copies));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_spmm(G.w[r], G.a[r], false);
            launch_finalize(G.w[r], G.a[r], kDotPAP);
        }
        TRY(group_sum(G, gt, kDotPAP, nrhs));
        for (int r = 0; r < G.P; r++) {
            TRY(use(G, r));
            launch_update(G.w[r], G.a[r], false);
            launch_finalize(G.w[r], G.a[r], kDotRR);
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
    // the end on member 0's stream, whose last launch followed every member's
    TRY(use(G, 0));
    HIP_TRY(hipEventRecord(w0->ev1, G.v[0].stream));
    std::vector<ColState> st;
    std::vector<double> hist;
    TRY(read_columns(w0, nrhs, &st, &hist));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, w0->ev0, w0->ev1));
    *wall = 1e-3 * ms;
    w0->trace.assign(nrhs, {});
    for (int c = 0; c < nrhs; c++) {
        niters[c] = column_trace(st[c], hist.data() + (size_t)c * (size_t)w0->hstride, &w0->trace[c]);
        normr[c] = w0->trace[c][niters[c]];
    }
    for (int r = 1; r < G.P; r++) {  // (the last sum's event was their streams' last wait)
        TRY(use(G, r));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
    return 0;
}

int group_solve(hpccg_hip_matrix* const* Ms, const Group& G0, int nrhs, const double* const* B, const long long* ldb,
                double* const* X, const long long* ldx, const double* const* minv, int max_iter, double tol,
                bool copies, int* niters, double* normr, double* times)
{
    Group G = G0;
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
        TRY(copy_cols(w, w->b, w->vcs, B[r], ldb[r], nrhs, hipMemcpyDeviceToDevice));
        TRY(copy_cols(w, w->x, w->vcs, X[r], ldx[r], nrhs, hipMemcpyDeviceToDevice));
    }
    double wall = 0.0;
    TRY(group_run_cg(G, nrhs, max_iter, tol, copies, niters, normr, &wall));
    for (int r = 0; r < G.P; r++) {
        TRY(use(G, r));
        TRY(copy_cols(G.w[r], X[r], ldx[r], G.w[r]->x, G.w[r]->vcs, nrhs, hipMemcpyDeviceToDevice));
        HIP_TRY(hipStreamSynchronize(G.v[r].stream));
    }
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
    TRY(check_group_args(Ms, nranks));
    if (nrhs <= 0) return fail(HPCCG_HIP_EINVAL, "group pcg: nrhs %d (at least 1)", nrhs);
    if (max_iter < 0) return fail(HPCCG_HIP_EINVAL, "group pcg: max_iter %d is negative", max_iter);
    if (!B_dev || !ldb || !X_dev || !ldx || !niters || !normr)
        return fail(HPCCG_HIP_EINVAL, "group pcg: NULL argument (B_dev, ldb, X_dev, ldx, niters or normr)");
    for (int r = 0; r < nranks; r++) {
        if (!B_dev[r] || !X_dev[r]) return fail(HPCCG_HIP_EINVAL, "group pcg: B_dev[%d] or X_dev[%d] is NULL", r, r);
        if (minv_dev && !minv_dev[r]) return fail(HPCCG_HIP_EINVAL, "group pcg: minv_dev[%d] is NULL", r);
    }
    Group G;
    TRY(check_group(Ms, nranks, &G));
    for (int r = 0; r < nranks; r++)
        if (ldb[r] < G.v[r].n || ldx[r] < G.v[r].n)
            return fail(HPCCG_HIP_EINVAL, "group pcg: member %d's leading dimensions (ldb, ldx) %lld, %lld below its %d rows",
                        r, ldb[r], ldx[r], G.v[r].n);
    // diagnostics: the halo by copies, the A/B of k_pcg_group_halo (tools/group_pcg_bench.py)
    const bool copies = std::getenv("HPCCG_GROUP_PCG_HALO_COPIES") != nullptr;
    return keep_device([&] {
        return group_solve(Ms, G, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, tolerance, copies, niters, normr,
                           times);
    });
}

int hpccg_hip_group_pcg_diagonal(hpccg_hip_matrix* const* Ms, int nranks, double* const* d_dev)
{
    TRY(check_group_args(Ms, nranks));
    if (!d_dev) return fail(HPCCG_HIP_EINVAL, "group pcg: d_dev is NULL");
    for (int r = 0; r < nranks; r++)
        if (!d_dev[r]) return fail(HPCCG_HIP_EINVAL, "group pcg: d_dev[%d] is NULL", r);
    Group G;
    TRY(check_group(Ms, nranks, &G));
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
    TRY(check_group_args(Ms, nranks));
    if (!out) return fail(HPCCG_HIP_EINVAL, "group pcg: out is NULL");
    Group G;
    TRY(check_group(Ms, nranks, &G));
    // one set of all-reduced scalars: kept with member 0's record
    const Workspace* w = g_ws<Workspace>.find(Ms[0]);
    if (!w || col < 0 || col >= (int)w->trace.size())
        return fail(HPCCG_HIP_EINVAL, "group pcg: no trace of column %d (the last group solve had %d)", col,
                    w ? (int)w->trace.size() : 0);
    const std::vector<double>& tr = w->trace[col];
    const int n = std::min<int>(std::max(cap, 0), (int)tr.size());
    for (int i = 0; i < n; i++) out[i] = tr[i];
    return n;
}

int hpccg_hip_group_pcg_release(hpccg_hip_matrix* M)
{
    if (!M) return fail(HPCCG_HIP_EINVAL, "group pcg: NULL argument");
    g_ws<Workspace>.drop(M);
    return 0;
}

int hpccg_hip_group_pcg_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    if (!M || !bytes) return fail(HPCCG_HIP_EINVAL, "group pcg: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    *bytes = w ? w->bytes + w->rest_bytes : 0;
    return 0;
}

int hpccg_hip_group_pcg_live_workspaces(int* count)
{
    if (!count) return fail(HPCCG_HIP_EINVAL, "group pcg: NULL argument");
    *count = g_ws<Workspace>.live();
    return 0;
}

}  // extern "C"
