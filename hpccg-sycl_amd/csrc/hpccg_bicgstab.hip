// hpccg_bicgstab.hip -- right-preconditioned BiCGStab (include/hpccg_hip_bicgstab.h,
// lib/bicgstab/libhpccg_hip_bicgstab.so): kernels and host code of the fourteenth library.
//
// Every other solver here is a form of CG, which on a non-symmetric matrix
// returns ierr 0 and a wrong x. This unit runs another Krylov recurrence on the
// same matrix images, the same SpMM loops and the same dot shape, with
// M^-1 = diag(m), by default Jacobi m_i = 1.0 / a_ii (the header states every
// expression with its rounding order):
//   p = r + beta (p - omega v);  y = m p;  v = A y;  alpha = rho / rhat.v
//   s = r - alpha v;             z = m s;  t = A z;  omega = t.s / t.t
//   x = (x + alpha y) + omega z; r = s - omega t;    rho' = rhat.r
// Two passes over the matrix and three synchronisation points per iteration:
//   p step    k_bicg_p<kR>: p = x + 0 x into the guarded buffer (prologue) |
//             p, and y = m p into the guarded buffer
//   SpMM      k_bicg_spmm_a<kW, kR, kWaves> | k_bicg_spmm_sell<kR>: the fp64 loops
//             of hpccg_spmm.h on the guarded buffer, with this unit's ends
//             (BicgEnds): Ap (prologue) | v with the rhat.v slice partial | t
//             with the t.s and t.t slice partials, by the launch's phase
//   s step    k_bicg_s<kR>: s (kept in r's storage), and z = m s into the
//             guarded buffer
//   x step    k_bicg_x<kR>: r = b - Ap, rhat = r (prologue) | x, r (y and z
//             formed again from p, s and m), + the r.r and rhat.r slice partials
//   finalize  k_bicg_finalize: one block per column and stage; completes the
//             stage's dots (col_dot_total) and advances the column: alpha |
//             omega | rho, beta, the history, the loop test, the status
//   diagonal  k_bicg_diag | k_bicg_check (hpccg_jacobi.h's bodies)
// Vectors per column: x, b, r (s between the s and the x step), rhat, p, v, t
// (the engine's Ap) and the guarded SpMM input. The scalars CG does not have
// (omega, rho_old, rv, tt, ts, status) are this unit's BicgState beside the
// engine's ColState, which is unchanged (rtrans holds rho). The workspace
// registry, the dots' completion, the solve around the recurrence and the
// bookkeeping exports are hpccg_columns.h's and hpccg_onerank_host.h's; the
// launch loop is this unit's (the plan differs from CG's). No kernel here waits
// on another block; `ended` is the only atomic.
#include <hip/hip_runtime.h>

#include "../../include/hpccg_hip_bicgstab.h"
#include "hpccg_onerank_host.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

// The dots of the recurrence (slice partials [kBicgDots][cap][nslices]); r.r is the engine's kDotRR.
enum BicgDot : int { kDotRV = 1, kDotTS = 2, kDotTT = 3, kDotRho = 4, kBicgDots = 5 };

// What a finalize launch completes.
enum BicgStage : int { kStageRR = 0, kStageRV = 1, kStageTS = 2 };

// Where the SpMM's row sums go.
enum BicgPhase : int { kPhaseAp = 0, kPhaseV = 1, kPhaseT = 2 };

// Per-column scalars beside ColState (rtrans: rho_k; rr, alpha, beta, tol, k,
// run, niters, max_iter as in CG). Advanced by the finalize only.
struct BicgState {
    double omega;    // t.s / t.t of the last iteration (0.0 where t.t == 0.0)
    double rho_old;  // rho_{k-1}
    double rv;       // rhat.v
    double tt;       // t.t
    double ts;       // t.s
    int status;      // HPCCG_HIP_BICGSTAB_*: 0 the loop test, 1 breakdown, 2 r.r == 0.0
};

struct BicgArgs : ColArgs {
    // (ColArgs' p: the guarded SpMM input, y or z; Ap: t; minv: the call's m)
    int tri;  // width 27: slices whose offsets come in runs of three use the x-triple plan
    const double* aval;
    const double* vals;
    int phase;     // BicgPhase of an SpMM launch
    double* pv;    // the recurrence's p; column c at pv + c * vcs, as rhat, v
    double* rhat;  // r_0
    double* v;     // A y
    BicgState* bs;  // [cap]
};

// Every column of the call runs, with the call's tolerance and limit.
__global__ void k_bicg_init(BicgArgs a, int max_iter, double tol)
{
    col_init(a, max_iter, tol);
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < a.nrhs) a.bs[c] = BicgState{};
}

// ---------------------------------------------------------------------------
// prologue: p = x + 0.0*x into the guarded buffer (col_p's prologue form)
// loop:     p = r + beta*(p + (-omega)*v)   (k == 1 reads r for p; beta 0.0)
//           y = m*p into the guarded buffer, per running column.
// ---------------------------------------------------------------------------
template <int kR>
__global__ __launch_bounds__(kBlock) void k_bicg_p(BicgArgs a, bool prologue)
{
    if (prologue) {  // (grid-uniform)
        col_p<kR, false>(a, true);
        return;
    }
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    const Rows mv = ld(a.minv + row);
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        if (c >= a.nrhs) break;
        if (!a.st[c].run) continue;  // (block-uniform)
        const int k = a.st[c].k;
        const double beta = a.st[c].beta;
        const double omega = a.bs[c].omega;
        double* __restrict__ pc = a.pv + (size_t)c * a.vcs;
        const Rows rv = ld(a.r + (size_t)c * a.rcs + row);
        Rows in = rv;
        if (k != 1) {
            const Rows po = ld(pc + row);
            const Rows vv = ld(a.v + (size_t)c * a.vcs + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) in.v[i] = po.v[i] + (-omega) * vv.v[i];
        }
        Rows pn, y;
#pragma unroll
        for (int i = 0; i < kRpt; i++) {
            pn.v[i] = rv.v[i] + beta * in.v[i];
            y.v[i] = mv.v[i] * pn.v[i];
        }
        st_rows(pc, row, a.n, pn);
        st_rows(a.p + (size_t)c * a.pcs, row, a.n, y);
    }
}

// ---------------------------------------------------------------------------
// s = r + (-alpha)*v, kept in r's storage (r_{k-1} is read no more once alpha
// stands); z = m*s into the guarded buffer, per running column.
// ---------------------------------------------------------------------------
template <int kR>
__global__ __launch_bounds__(kBlock) void k_bicg_s(BicgArgs a, bool)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    const Rows mv = ld(a.minv + row);
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        if (c >= a.nrhs) break;
        if (!a.st[c].run) continue;  // (block-uniform)
        const double alpha = a.st[c].alpha;
        double* __restrict__ rc = a.r + (size_t)c * a.rcs;
        const Rows rv = ld(rc + row);
        const Rows vv = ld(a.v + (size_t)c * a.vcs + row);
        Rows sn, z;
#pragma unroll
        for (int i = 0; i < kRpt; i++) {
            sn.v[i] = rv.v[i] + (-alpha) * vv.v[i];
            z.v[i] = mv.v[i] * sn.v[i];
        }
        st_rows(rc, row, a.n, sn);
        st_rows(a.p + (size_t)c * a.pcs, row, a.n, z);
    }
}

// ---------------------------------------------------------------------------
// prologue: r = b + (-1)*Ap; rhat = r; the r.r slice partial (rho_1 is r_0.r_0)
// loop:     x = (x + alpha*y) + omega*z; r = s + (-omega)*t, with y = m*p and
//           z = m*s formed again (the bits the SpMMs read); the r.r and rhat.r
//           slice partials, per running column.
// ---------------------------------------------------------------------------
template <int kR>
__global__ __launch_bounds__(kBlock) void k_bicg_x(BicgArgs a, bool prologue)
{
    const int s = xcd_slice(a.grid);
    if (s >= a.nslices) return;
    const int row = s * kSliceRows + threadIdx.x * kRpt;
    Rows mv{};
    if (!prologue) mv = ld(a.minv + row);
#pragma unroll
    for (int j = 0; j < kR; j++) {
        const int c = a.c0 + j;
        if (c >= a.nrhs) break;
        if (!a.st[c].run) continue;  // (block-uniform)
        double* __restrict__ rc = a.r + (size_t)c * a.rcs;
        double* __restrict__ hc = a.rhat + (size_t)c * a.vcs;
        const Rows tv = ld(a.Ap + (size_t)c * a.vcs + row);
        Rows rn;
        if (prologue) {
            const Rows bv = ld(a.b + (size_t)c * a.vcs + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) rn.v[i] = bv.v[i] + (-1.0) * tv.v[i];
            st_rows(hc, row, a.n, rn);
        } else {
            const double alpha = a.st[c].alpha;
            const double omega = a.bs[c].omega;
            const Rows sv = ld(rc + row);
            const Rows pv = ld(a.pv + (size_t)c * a.vcs + row);
            double* __restrict__ xc = a.x + (size_t)c * a.vcs;
            const Rows xv = ld(xc + row);
            Rows xn;
#pragma unroll
            for (int i = 0; i < kRpt; i++) {
                const double y = mv.v[i] * pv.v[i];
                const double z = mv.v[i] * sv.v[i];
                xn.v[i] = (xv.v[i] + alpha * y) + omega * z;
                rn.v[i] = sv.v[i] + (-omega) * tv.v[i];
            }
            st_rows(xc, row, a.n, xn);
        }
        st_rows(rc, row, a.n, rn);
        if (!prologue) rw_slice_partial(a, kDotRho, s, row, c, ld(hc + row), rn);
        rr_slice_partial(a, s, row, c, rn);
    }
}

// The ends of this unit's SpMMs: x is the guarded buffer; the row sums are Ap
// (prologue: no dot), v with the rhat.v slice partial, or t with the t.s and
// t.t slice partials (s: r's storage).
struct BicgEnds {
    template <class A>
    static __device__ __forceinline__ const double* x(const A& a)
    {
        return a.p;
    }
    template <int kR, class A>
    static __device__ __forceinline__ void out(const A& a, bool, int s, int row, const bool (&act)[kR],
                                               const double (&sum)[kR][kRpt])
    {
        double* const dst = a.phase == kPhaseV ? a.v : a.Ap;
#pragma unroll
        for (int j = 0; j < kR; j++) {
            if (!act[j]) continue;  // (block-uniform)
            const int c = a.c0 + j;
            const Rows o{{sum[j][0], sum[j][1]}};
            st_rows(dst + (size_t)c * a.vcs, row, a.n, o);
            if (a.phase == kPhaseV) {
                rw_slice_partial(a, kDotRV, s, row, c, ld(a.rhat + (size_t)c * a.vcs + row), o);
            } else if (a.phase == kPhaseT) {
                rw_slice_partial(a, kDotTS, s, row, c, o, ld(a.r + (size_t)c * a.rcs + row));
                rw_slice_partial(a, kDotTT, s, row, c, o, o);
            }
        }
    }
};

// The pcg library's plan choices (hpccg_pcg.hip): kWaves 5 for the 27-wide
// four-column form over images streamed from HBM, else 4.
template <int kW, int kR, int kWaves = 4>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves))) void k_bicg_spmm_a(BicgArgs a,
                                                                                                    bool prologue)
{
    spmm_a_body<kW, kR, BicgArgs, BicgEnds>(a, prologue);
}

template <int kR>
__global__ __launch_bounds__(kBlock) void k_bicg_spmm_sell(BicgArgs a, bool prologue)
{
    spmm_sell_body<kR, BicgArgs, BicgEnds>(a, prologue);
}

// The column ends here: iterations done, why, and the word the host polls.
__device__ __forceinline__ void bicg_end(const BicgArgs& a, ColState* st, BicgState* bs, int niters, int status)
{
    st->run = 0;
    st->niters = niters;
    bs->status = status;
    atomicAdd(a.ended, 1);
}

// ---------------------------------------------------------------------------
// One block per column: the stage's dots (col_dot_total), then the column's
// scalars by one lane.
//   rhat.v: alpha = rho_k / rhat.v; 0.0 ends the column before iteration k
//           touches s, x or r (status 1).
//   t.s, t.t: omega = t.s / t.t, 0.0 where t.t == 0.0.
//   r.r, rhat.r of iteration k (the prologue: r.r alone, rho_1 = r_0.r_0):
//           hist[k]; rho; CG's lagged loop test (advance_column's); then the
//           ends the test does not see: r.r == 0.0 (status 2), rho == 0.0 or
//           omega == 0.0 (status 1: the next beta or alpha has no value);
//           else beta for iteration k + 1.
// Every comparison is false for a NaN, which so runs on to the loop test.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kFinThreads) void k_bicg_finalize(BicgArgs a, int stage, int)
{
    __shared__ double gs[kFinLds];
    const int c = blockIdx.x;
    ColState* const st = a.st + c;
    BicgState* const bs = a.bs + c;
    if (!st->run) return;  // (block-uniform) a frozen column keeps its state
    const int k = st->k;   // the iteration running (kStageRR: the one that has run; 0: the prologue)
    if (stage == kStageRV) {
        const double rv = col_dot_total(a, kDotRV, c, gs);
        if (threadIdx.x != 0) return;
        bs->rv = rv;
        if (rv == 0.0)
            bicg_end(a, st, bs, k - 1, HPCCG_HIP_BICGSTAB_BREAKDOWN);
        else
            st->alpha = st->rtrans / rv;
        return;
    }
    if (stage == kStageTS) {
        const double ts = col_dot_total(a, kDotTS, c, gs);
        __syncthreads();  // the t.s group sums in gs have been read
        const double tt = col_dot_total(a, kDotTT, c, gs);
        if (threadIdx.x != 0) return;
        bs->ts = ts;
        bs->tt = tt;
        bs->omega = tt == 0.0 ? 0.0 : ts / tt;
        return;
    }
    const double rr = col_dot_total(a, kDotRR, c, gs);
    double rho = rr;
    if (k > 0) {          // (block-uniform)
        __syncthreads();  // the r.r group sums in gs have been read
        rho = col_dot_total(a, kDotRho, c, gs);
    }
    if (threadIdx.x != 0) return;
    const double old = st->rtrans;  // rho_k (k >= 1)
    const double oldrr = st->rr;    // r_{k-1}.r_{k-1} (k >= 1)
    a.hist[(size_t)c * a.hstride + k] = rr;
    bs->rho_old = old;
    st->oldrtrans = old;
    st->rtrans = rho;
    st->rr = rr;
    st->k = k + 1;
    const bool run = k + 1 < st->max_iter && sqrt(k == 0 ? rr : oldrr) > st->tol;
    if (!run)
        bicg_end(a, st, bs, k, HPCCG_HIP_BICGSTAB_CONVERGED);
    else if (rr == 0.0)
        bicg_end(a, st, bs, k, HPCCG_HIP_BICGSTAB_EXACT);
    else if (rho == 0.0 || (k > 0 && bs->omega == 0.0))
        bicg_end(a, st, bs, k, HPCCG_HIP_BICGSTAB_BREAKDOWN);
    else
        st->beta = k == 0 ? 0.0 : (rho / old) * (st->alpha / bs->omega);
}

// The diagonal of the image and the check of a caller's m: hpccg_jacobi.h's bodies.
__global__ __launch_bounds__(kBlock) void k_bicg_diag(DiagArgs a, double* d_out, double* minv_out, int* bad)
{
    diag_body(a, d_out, minv_out, bad);
}

__global__ void k_bicg_check(const double* __restrict__ m, int n, int* bad)
{
    check_body(m, n, bad);
}

// ---------------------------------------------------------------------------
// host: hpccg_onerank_host.h over this unit's kernels, and the launch loop
// ---------------------------------------------------------------------------
struct Workspace : TraceWorkspace, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr, *rhat = nullptr, *pv = nullptr, *vv = nullptr;
    BicgState* bs = nullptr;
    std::vector<int> status;  // per column of the last solve

    Workspace() { ndots = kBicgDots; }

    void free_own_vectors()
    {
        for (void* q : {(void*)r, (void*)x, (void*)b, (void*)rhat, (void*)pv, (void*)vv, (void*)bs})
            if (q) (void)hipFree(q);
        r = x = b = rhat = pv = vv = nullptr;
        bs = nullptr;
    }
    void free_own_rest() { free_cache(); }
    long long total_bytes() const { return bytes + rest_bytes; }
};

// Room for ncols columns and a history of max_iter + 1 entries per column.
int ensure_vectors(Workspace* w, int ncols, int max_iter)
{
    const size_t npad = (size_t)w->v.npad;
    return ensure_columns(w, ncols, max_iter, true, p_column(w->v), 0, [&](int cap) {
        for (double** q : {&w->r, &w->x, &w->b, &w->rhat, &w->pv, &w->vv}) TRY(alloc_zero(w, q, npad * cap));
        return alloc_zero(w, &w->bs, (size_t)cap);
    });
}

BicgArgs make_args(const Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    BicgArgs a{};
    fill_args(&a, w, nrhs);  // (Ap: t)
    a.tri = 1;
    a.p = w->pbuf + v.guard_rows;  // y, z
    a.r = w->r;
    a.rcs = w->vcs;
    a.x = w->x;
    a.b = w->b;
    a.minv = m;
    a.aval = v.aval;
    a.vals = v.vals;
    a.phase = kPhaseAp;
    a.pv = w->pv;
    a.rhat = w->rhat;
    a.v = w->vv;
    a.bs = w->bs;
    return a;
}

struct Bicg {
    using Args = BicgArgs;
    using Workspace = hpccg::Workspace;
    static constexpr const char* who = "bicgstab";
    static constexpr const char* solve_name = "BiCGStab";

    static constexpr auto init = k_bicg_init;
    template <int kW, int kR, int kWaves>
    static constexpr auto spmm_a = k_bicg_spmm_a<kW, kR, kWaves>;
    template <int kR>
    static constexpr auto spmm_sell = k_bicg_spmm_sell<kR>;
    static constexpr auto finalize = k_bicg_finalize;
    static constexpr auto diag = k_bicg_diag;
    static constexpr auto check = k_bicg_check;
};

void launch_spmm(const Workspace* w, BicgArgs a, int phase)
{
    a.phase = phase;
    launch_spmm64<Bicg>(w, a, phase == kPhaseAp);
}

// One recurrence per running column of the states on the device: the prologue,
// then iterations 1 .. kmax - 1, eight launches each, launched eagerly on the
// matrix's stream; the "columns ended" word is read as in run_recurrence.
int run_iterations(Workspace* w, const BicgArgs& a, int nrun, int kmax)
{
    hipStream_t s = w->v.stream;
    const auto p = [](auto r) { return k_bicg_p<decltype(r)::value>; };
    const auto sstep = [](auto r) { return k_bicg_s<decltype(r)::value>; };
    const auto x = [](auto r) { return k_bicg_x<decltype(r)::value>; };
    launch_chunks(w, a, true, p);
    launch_spmm(w, a, kPhaseAp);
    launch_chunks(w, a, true, x);
    launch_finalize<Bicg>(w, a, kStageRR, 0);
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < kmax; k++) {
        launch_chunks(w, a, false, p);
        launch_spmm(w, a, kPhaseV);
        launch_finalize<Bicg>(w, a, kStageRV, 0);
        launch_chunks(w, a, false, sstep);
        launch_spmm(w, a, kPhaseT);
        launch_finalize<Bicg>(w, a, kStageTS, 0);
        launch_chunks(w, a, false, x);
        launch_finalize<Bicg>(w, a, kStageRR, 0);
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

// BiCGStab on the columns staged in the workspace's b and x.
int run_bicg(Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr,
             double* wall)
{
    const BicgArgs a = make_args(w, nrhs, m);
    w->status.clear();
    HIP_TRY(hipEventRecord(w->ev0, w->v.stream));
    launch_init<Bicg>(w, a, max_iter, tol);
    TRY(run_iterations(w, a, nrhs, max_iter));
    TRY(finish_recurrence(w, nrhs, niters, normr, wall));
    std::vector<BicgState> bs(nrhs);
    HIP_TRY(hipMemcpyAsync(bs.data(), w->bs, sizeof(BicgState) * nrhs, hipMemcpyDeviceToHost, w->v.stream));
    HIP_TRY(hipStreamSynchronize(w->v.stream));
    // (a column still running when the launches ran out ended by the iteration limit: status 0)
    for (int c = 0; c < nrhs; c++) w->status.push_back(bs[c].status);
    return 0;
}

int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int max_iter, double tol, int* niters, double* normr, double* times, bool host)
{
    return solve_onerank<Bicg>(
        M, nrhs, B, ldb, X, ldx, minv, max_iter, tol, niters, normr, times, host, [] { return 0; }, nullptr,
        [&](Workspace* w, const double*, int kmax) { return ensure_vectors(w, nrhs, kmax); }, run_bicg);
}

}  // namespace

}  // namespace hpccg

using namespace hpccg;

extern "C" {

int hpccg_hip_bicgstab_abi_version(void) { return 1; }

int hpccg_hip_bicgstab_solve_device(hpccg_hip_matrix* M, int nrhs, const double* B_dev, long long ldb, double* X_dev,
                                    long long ldx, const double* minv_dev, int max_iter, double tolerance,
                                    int* niters, double* normr, double* times)
{
    return solve_common(M, nrhs, B_dev, ldb, X_dev, ldx, minv_dev, max_iter, tolerance, niters, normr, times, false);
}

int hpccg_hip_bicgstab_solve(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                             const double* minv, int max_iter, double tolerance, int* niters, double* normr,
                             double* times)
{
    return solve_common(M, nrhs, B, ldb, X, ldx, minv, max_iter, tolerance, niters, normr, times, true);
}

int hpccg_hip_bicgstab_last_trace(const hpccg_hip_matrix* M, int col, double* out, int cap)
{
    return unit_last_trace<Bicg>(M, col, out, cap);
}

int hpccg_hip_bicgstab_last_status(const hpccg_hip_matrix* M, int col, int* status)
{
    if (!M || !status) return fail(HPCCG_HIP_EINVAL, "bicgstab: NULL argument");
    const Workspace* w = g_ws<Workspace>.find(M);
    if (!w || col < 0 || col >= (int)w->status.size())
        return fail(HPCCG_HIP_EINVAL, "bicgstab: no status of column %d (the last BiCGStab solve had %d)", col,
                    w ? (int)w->status.size() : 0);
    *status = w->status[col];
    return 0;
}

int hpccg_hip_bicgstab_release(hpccg_hip_matrix* M) { return unit_release<Bicg>(M); }

int hpccg_hip_bicgstab_workspace_bytes(const hpccg_hip_matrix* M, long long* bytes)
{
    return unit_workspace_bytes<Bicg>(M, bytes);
}

int hpccg_hip_bicgstab_live_workspaces(int* count) { return unit_live_workspaces<Bicg>(count); }

}  // extern "C"
