// hpccg_host.h -- what the main library's host units share (hpccg_plan.cpp, hpccg_comm.cpp,
// hpccg_solver.cpp, hpccg_options.cpp, hpccg_diag.cpp, hpccg_dropin.cpp):
// the error macros, struct hpccg_hip_matrix, the communicator, plan and group types, the shared constants,
// a declaration of every function called across units, and the templates that more than one unit
// instantiates. Host only and private to libhpccg_hip.so: the kernels and the unit libraries never include
// it (they go through MatrixView and hpccg_hip_internal_*). Everything here but the matrix struct has hidden
// visibility, so no helper becomes a dynamic export.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/HPC_Sparse_Matrix.hpp"
#include "../../include/hpccg_hip.h"
#ifndef HPCCG_HOST_DEVICE_FREE
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include "hpccg_internal.h"
static_assert(hpccg::kSliceRows == 512, "the device-free part below mirrors it");
#else
namespace hpccg {
constexpr int kSliceRows = 512;  // hpccg_internal.h's (which includes the HIP runtime)
}  // namespace hpccg
#endif

using namespace hpccg;

// ---- the device-free part: all that hpccg_plan.cpp sees (it defines HPCCG_HOST_DEVICE_FREE) ----
#pragma GCC visibility push(hidden)
namespace hpccg::host {

int set_err(int code, const char* fmt, ...);
const std::string& last_err();
void clear_err();

// Gather halo plan (make_local_matrix.cpp:58-610, exchange_externals.cpp:51-131)
// for partitions the z-slab plan cannot serve: the external columns get local
// indices n, n+1, ... grouped by owning rank, groups in order of first
// appearance and first appearance inside a group, exactly as
// make_local_matrix.cpp:96-200 numbers them.
struct GatherPlan {
    std::vector<long long> ext_global;              // external j <-> local column n + j
    std::unordered_map<long long, int> ext_of;      // global column -> j
    std::vector<int> recv_rank, recv_off, recv_cnt; // externals owned by recv_rank[i]: [off, off + cnt)
    std::vector<std::vector<int>> req;              // per owner: the global columns we need, our order
    std::vector<int> send_rank, send_off, send_cnt; // per requester: a run of send_idx
    std::vector<int> send_idx;                      // local rows packed for the requesters
};

// ---------------------------------------------------------------------------
// SELL-512 build from any row accessor. Entry order per row is preserved.
// ---------------------------------------------------------------------------
// Column map of the slab plan: global column -> index into [ghost_lo | n | ghost_hi].
struct SlabCols {
    long long col_base, ncol_ext;
    long long operator()(long long c) const
    {
        const long long lc = c - col_base;
        return (lc < 0 || lc >= ncol_ext) ? -1 : lc;
    }
};

extern int g_halo_mode;

// hpccg_plan.cpp
int choose_halo_mode(const int* info, int P);
int owner_of(long long c, const int* info, int P);
void gather_sends(long long start, const std::vector<std::vector<int>>& reqs_to_me, GatherPlan& g);

template <class RowLen, class RowAt, class ColMap>
long long sell_build_impl(int nrow, ColMap colmap, RowLen row_len, RowAt row_at, unsigned int* slice_base,
                          int* sell_cols, double* sell_vals, int uniform_width, int* err)
{
    const int nslices = (nrow + kSliceRows - 1) / kSliceRows;
    long long total = 0;
    int wmax = 0;
    std::vector<int> w(nslices, 0);
    for (int s = 0; s < nslices; s++) {
        int m = 0;
        for (int i = s * kSliceRows; i < std::min(nrow, (s + 1) * kSliceRows); i++) m = std::max(m, row_len(i));
        w[s] = m;
        wmax = std::max(wmax, m);
    }
    if (uniform_width) std::fill(w.begin(), w.end(), wmax);
    for (int s = 0; s < nslices; s++) {
        if (slice_base) slice_base[s] = (unsigned int)total;
        total += w[s];
    }
    if (slice_base) slice_base[nslices] = (unsigned int)total;
    if (!sell_cols || !sell_vals) return total * kSliceRows;
    std::atomic<int> bad{0};
    const int nth = std::max(1, std::min<int>(16, (int)std::thread::hardware_concurrency()));
    auto work = [&](int t) {
        for (int s = t; s < nslices; s += nth) {
            const size_t b0 = (size_t)slice_base[s] * kSliceRows;
            for (int lane = 0; lane < kSliceRows; lane++) {
                const int i = s * kSliceRows + lane;
                const int len = i < nrow ? row_len(i) : 0;
                for (int j = 0; j < w[s]; j++) {
                    const size_t e = b0 + (size_t)j * kSliceRows + lane;
                    if (j < len) {
                        double v;
                        long long c;
                        row_at(i, j, &c, &v);
                        const long long lc = colmap(c);
                        if (lc < 0) bad.store(1);
                        sell_cols[e] = (int)lc;
                        sell_vals[e] = v;
                    } else {
                        sell_cols[e] = -1;
                        sell_vals[e] = 0.0;
                    }
                }
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nth; t++) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
    if (err) *err = bad.load();
    return total * kSliceRows;
}

template <class RowLen, class RowAt>
void gather_externals(int nrow, long long start, const int* info, int P, RowLen row_len, RowAt row_at, GatherPlan& g)
{
    std::vector<long long> first;  // externals in order of first appearance
    std::unordered_map<long long, int> seen;
    for (int i = 0; i < nrow; i++) {
        const int len = row_len(i);
        for (int j = 0; j < len; j++) {
            long long c;
            double v;
            row_at(i, j, &c, &v);
            if (c >= start && c < start + nrow) continue;
            if (seen.emplace(c, (int)first.size()).second) first.push_back(c);
        }
    }
    std::vector<std::vector<int>> by_owner(P);
    std::vector<int> order;
    for (int i = 0; i < (int)first.size(); i++) {
        const int q = owner_of(first[i], info, P);
        if (by_owner[q].empty()) order.push_back(q);
        by_owner[q].push_back(i);
    }
    g.ext_global.assign(first.size(), 0);
    g.req.assign(P, {});
    int count = 0;
    for (int q : order) {
        g.recv_rank.push_back(q);
        g.recv_off.push_back(count);
        g.recv_cnt.push_back((int)by_owner[q].size());
        for (int i : by_owner[q]) {
            g.ext_global[count] = first[i];
            g.ext_of[first[i]] = count;
            g.req[q].push_back((int)first[i]);
            count++;
        }
    }
}

}  // namespace hpccg::host
#pragma GCC visibility pop

#ifndef HPCCG_HOST_DEVICE_FREE

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_err(e_ == hipErrorOutOfMemory ? HPCCG_HIP_ENOMEM : HPCCG_HIP_EHIP,          \
                           "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);   \
    } while (0)

#define NCCL_TRY(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return set_err(HPCCG_HIP_ERCCL, "%s: %s (%s:%d)", #expr, ncclGetErrorString(r_),      \
                           __FILE__, __LINE__);                                                    \
    } while (0)

#define TRY(expr)                                                                                  \
    do {                                                                                           \
        int rc_ = (expr);                                                                          \
        if (rc_ != 0) return rc_;                                                                  \
    } while (0)

// ---------------------------------------------------------------------------
// device matrix + CG workspace
// ---------------------------------------------------------------------------
struct hpccg_hip_matrix {
    int device = 0;
    int rank = 0, nranks = 1;  // z-slab rank of this matrix (RCCL communicator or in-process group)
    int in_group = 0;          // 1: halo / all-reduce by hpccg_hip_group_solve, not RCCL
    unsigned long long group_id = 0;  // the in-process group this member was made in (0: none)
    int nrow = 0, start_row = 0, total_nrow = 0;
    int ghost_lo = 0, ghost_hi = 0;
    int send_lo = 0;  // rows to send to rank-1 (its ghost_hi)
    int send_hi = 0;  // rows to send to rank+1 (its ghost_lo)
    // gather plan (partitions the slab plan cannot serve): externals after the
    // local rows (ghost_lo = 0, ghost_hi = number of externals)
    int general = 0;
    std::vector<int> recv_rank, recv_off, recv_cnt, send_rank, send_off, send_cnt;
    int nsend = 0;
    int* d_send_idx = nullptr;
    double* d_send_buf = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_flush = nullptr;  // flush_stream's marker (default flags: system-scope release)
    hipEvent_t ev_mid = nullptr;    // wait_matrix: blocking-sync marker before a solve's last graph chunk
    int mid_pending = 0;            // ev_mid was recorded for the solve in flight
    long long nnz = 0, nslots = 0;
    int nslices = 0, grid = 0, width = 0, uniform = 0;
    int kernel = 0;       // SpMV kernel in use (SpmvKernel)
    int kernel_opt = -1;  // option spmv_kernel (-1 auto)
    int use_graph = 1;
    int fuse_p = -1;      // -1 auto: on where the kernel forms p_k itself
    int fuse_update = -1; // the update as trailing blocks of the SpMV launch; -1 auto (fuse_update_effective)
    int resident_update = -1;     // the resident pair kernels (k_spmv_ar, k_cg_persist; resident_of, persist_ok)
    int nt_opt = -1;              // option nt (diagnostics): -1 auto (image_big), 0 / 1 force the matrix loads' hint
    int resident_retries = 0;     // solves re-run after a resident launch's wait expired (resident_retry)
    int resident_failed = 0;      // a resident launch's wait expired (GPU shared): the unit + update launch from then on
    int resident_used = 0;        // the last solve ran k_spmv_ar
    int last_dev_err = 0;         // the device error code the last failed solve recorded (DevError)
    int last_dev_err_all = 0;     // ... its maximum over a job's ranks (all-reduced: the same on every rank)
    size_t npartial = 0;  // dot slots (the last one: the fused update's p.Ap total)
    int a2_ring = kA2RingDefault;  // pair kernel: LDS-DMA value ring depth per wave (0: register loads; uniform widths 27 and 7)
    int fold = -1;        // -1 auto: 1 (both dots completed in their producers); 0 k_finalize
    int force_comm = 0;   // diagnostics: 1 scalars through the RCCL communicator even at one rank;
                          // 2 also the multi-rank iteration with a self send/recv as its halo
    // SELL-512 (the general kernel; freed once SELL-512-A exists unless kept)
    int has_sell = 0;
    unsigned int* d_slice_base = nullptr;
    int* d_cols = nullptr;
    double* d_vals = nullptr;
    // SELL-512-A
    int has_a = 0, a_width = 0;
    int a_reject = 0;  // SELL-512-A not built (diagnostics): 2 its flag read late, 3 rejected although
                       // the device's columns fit (a kernel fault), 4 rejected and they do not
    long long a_slots = 0;
    double* d_aval = nullptr;
    int* d_aoff = nullptr;
    unsigned int* d_abase = nullptr;
    int has_pairs = 0, alds2_doubles = 0;
    int *d_alds2 = nullptr, *d_awin2 = nullptr, *d_awn2 = nullptr, *d_adiag2 = nullptr;
    unsigned char* d_atri = nullptr;  // direct kernel: slices in the width's triple plan
    // workspace (padded to a multiple of kSliceRows rows)
    size_t npad = 0;
    double* d_pbuf = nullptr;  // ring_alloc buffers of [guard | ghost_lo_pad | npad | ghost_hi_pad | guard]
    int ring_alloc = 0;
    double* d_p = nullptr;     // local rows of ring buffer 0
    long long pstride = 0;
    double* d_ahist = nullptr;
    double* d_pslots = nullptr;   // persistent CG (persist_of): per-iteration dot slots
    long long pslots_cap = 0;     // doubles
    int x_defer = 2;      // deferred x: beside the SpMV where the kernel carries it, else batched (x_defer_effective)
    int x_ring = -1;
    double *d_r = nullptr, *d_Ap = nullptr, *d_x = nullptr, *d_b = nullptr;
    double* d_rbuf = nullptr;
    double* d_partial = nullptr;  // inside the d_kst block (not freed on its own)
    double* d_scal = nullptr;  // g[2], loc[2], spare
    double** d_gtab = nullptr;  // group fold (last member): the members' loc, then their g
    std::vector<double*> h_gtab;
    PullSeg* d_pseg = nullptr;  // group fold (member 0): every member's pull, done by its update
    std::vector<PullSeg> h_pseg;
    int gfold_used = 0;         // the last group solve summed its dots in the last member's kernels
    int* d_kst = nullptr;      // [0, kErrBase) iteration state, then the device error record (kErrWords)
    long long spin_us = kSpinTicksDefault / 100;  // bound of every in-kernel wait (option spin_budget_us)
    int dbg_withhold = 0;      // debug: slice + 1 whose p.Ap partial is withheld (guard test)
    int dbg_resident_stall = 0;  // debug: the resident launch's p.Ap wait expires (the retry test)
    unsigned long long* d_tl = nullptr;  // diagnostics (dbg_timeline): per unit kTlWords block stamps
    int tl_units = 0;
    int solve_dirty = 0;       // a solve started and did not finish cleanly: reset the dot slots first
    // peer-memory all-reduce of the CG scalars (option peer_allreduce)
    int peer_ar = -1;                  // option peer_allreduce: -1 auto (peer_ar_of), 0 off, 1 on
    int peer_auto_ok = 0;              // auto: the creation-time self-test passed on every rank
    // r-halo by pull (option halo_pull: -1 auto, 0 the RCCL / peer-copy planes, 1 k_pull, 2 in-launch)
    int halo_pull = -1;
    int pull_auto_ok = 0;              // RCCL job: the creation-time pull test passed on every rank
    int proto_auto_ok = 0;             // ... and the production-protocol test (protocol_autotest)
    int persist_auto_ok = 0;           // ... and its persistent-launch run (every rank's blocks co-resident, same bits)
    std::string selftest_note;         // why a creation-time self-test failed on this rank (diagnostics)
    double* d_pull_lo = nullptr;       // rank - 1's r (its local row 0), mapped here (RCCL job)
    double* d_pull_hi = nullptr;       // rank + 1's r
    double* d_pullx_lo = nullptr;      // rank - 1's x workspace (d_x, its local row 0): the prologue's p = x halo
    double* d_pullx_hi = nullptr;      // rank + 1's x
    int pull_lo_n = 0;                 // rank - 1's row count
    std::vector<void*> ipc_r_opened;   // the neighbours' r buffers mapped from other processes
    double* d_mbox = nullptr;          // this rank's mailbox (kMboxSlots, uncached / fine-grained)
    double** d_peers = nullptr;        // device table: every rank's mailbox, as this rank addresses it
    int peers_for = 0;                 // ranks the table was built for (0: none)
    std::vector<void*> ipc_opened;     // peers' mailboxes mapped from other processes
    double* d_hist = nullptr;
    unsigned long long* d_stamps = nullptr;
    double* d_emul = nullptr;  // force_comm 2: self-exchange receive buffer (two planes)
    int emul_plane = 0;        // force_comm 2: rows per plane (the largest column offset; 0 unknown)
    int hist_cap = 0;
    long long stamp_cap = 0;
    // pinned readback of a solve's results (state, scalars, r.r history, timer
    // stamps): one batch of async copies and one wait per solve
    char* h_rb = nullptr;
    size_t h_rb_bytes = 0;
    std::vector<void*> graveyard;  // diagnostics: buffers moved by hpccg_hip_diag_realloc, held until destroy
    struct Vmm {
        void* va;  // the mapping (aligned inside the reservation)
        size_t bytes;
        hipMemGenericAllocationHandle_t h;
        void* res;  // the reservation
        size_t res_bytes;
    };
    std::vector<Vmm> vmm;  // diagnostics: hpccg_hip_diag_realloc's VMM mappings (unmapped at destroy)
    std::vector<double> place_us;  // placement probe: SpMV us per candidate (0 = the creation placement)
    int place_pick = 0;            // the candidate kept
    double *d_gen_b = nullptr, *d_gen_x0 = nullptr, *d_gen_xexact = nullptr;
    long long bytes = 0;       // device bytes held
    // hipGraph of graph_chunk iterations (kernel arguments are baked in)
    hipGraphExec_t graph_exec = nullptr;
    int graph_chunk = 0;
    int graph_iters = 32;  // 100^3 same-process A/B: 20 442 vs 20 198 it/s at 8 (200^3 +0.15 %); 499 (one graph per solve) 20 033
    std::vector<CgArgs> graph_args;
    int graph_kernel = -1;
    int graph_failed = 0;      // capture refused here (e.g. RCCL inside a graph): eager from then on
    int graph_used = 0;        // the last solve replayed graphs
    // hipEvent timing (event_timing option)
    int event_timing = 0;
    std::vector<hipEvent_t> ev;
    double ktimes[4] = {0, 0, 0, 0};
    std::vector<double> kiter;  // event_timing: per iteration {SpMV ms, update ms}
    std::vector<double> trace;
    int last_niters = 0;
    // hpccg_hip_internal_on_destroy: run at the start of hpccg_hip_matrix_destroy
    std::vector<std::pair<void (*)(void*), void*>> destroy_hooks;
};

#pragma GCC visibility push(hidden)
namespace hpccg::host {

// ---------------------------------------------------------------------------
// communicator (one rank per GPU per process)
// ---------------------------------------------------------------------------
struct Comm {
    ncclComm_t comm = nullptr;
    int nranks = 1;
    int rank = 0;
    // host-bootstrapped (hpccg_hip_comm_init_host): no RCCL communicator; the
    // setup exchanges go through the caller's all-gather, and the iteration
    // must run without a collective (peer all-reduce + halo pull)
    hpccg_hip_allgather_fn ag = nullptr;
    void* ag_ctx = nullptr;
    // RCCL: the setup collectives' stream and staging buffer
    hipStream_t stream = nullptr;
    unsigned char* d_buf = nullptr;
    size_t buf_bytes = 0;
};

// In-process rank group (hpccg_hip_group_*): while a group member is being
// created on this thread, rank/size come from here instead of the RCCL
// communicator, and the halo plan is made by hpccg_hip_group_* afterwards.
struct GroupCtx {
    int active = 0, nranks = 1, rank = 0;
    const int* info = nullptr;        // every member's {nrow, ghost_lo, ghost_hi, start_row}, or null
    const GatherPlan* plan = nullptr; // this member's gather plan (gather mode), or null
};

constexpr int kPlaceAuto = 6;        // candidates of the automatic probe
constexpr int kPlacePhases = 4;      // values, p ring, r, Ap
constexpr double kPlaceMinBytes = 512e6;  // auto: only images that stream from HBM
// The ranks one host thread enqueues: one matrix (a process of an RCCL job, or
// a single GPU), or every member of an in-process group (hpccg_hip_group_*).
struct Ranks {
    hpccg_hip_matrix* const* M;
    const CgArgs* a;
    int P;
    hipEvent_t* ev;  // group: P "ready" events + 1 "reduced" event
};

extern Comm g_comm;
extern thread_local GroupCtx g_group_ctx;
extern int g_keep_sell;
extern int g_place_tries;

// hpccg_comm.cpp
bool comm_host();
bool comm_up();
int comm_allgather(const void* mine, void* all, size_t bytes);
int comm_min(int v, int* out);
int transport_verdict(const int local[3], int out[3]);
int comm_nranks();
int comm_rank();

// hpccg_solver.cpp
bool canary_on();
hipError_t big_malloc(void** p, size_t b, unsigned flags = hipDeviceMallocDefault);
void big_free(void* p);
int canary_check(std::string* report);
int h2d_stream(hipStream_t s, void* dst, const void* src, size_t bytes);
int flush_stream(hpccg_hip_matrix* M);
int free_matrix(hpccg_hip_matrix* M);
bool nt_load_of(const hpccg_hip_matrix* M);
bool kernel_available(const hpccg_hip_matrix* M, int k);
int choose_kernel(const hpccg_hip_matrix* M);
int a2_ring_effective(const hpccg_hip_matrix* M);
bool nt_store_effective(const hpccg_hip_matrix* M);
bool fuse_p_effective(const hpccg_hip_matrix* M);
bool rhalo_of(const hpccg_hip_matrix* M);
bool peer_ar_of(const hpccg_hip_matrix* M);
bool pull_of(const hpccg_hip_matrix* M);
bool pull_in_of(const hpccg_hip_matrix* M, const CgArgs& a);
int fold_effective(const hpccg_hip_matrix* M);
int x_ring_effective(const hpccg_hip_matrix* M);
int alloc_ring(hpccg_hip_matrix* M, int nbuf);
bool multi_of(const hpccg_hip_matrix* M);
int ensure_hist(hpccg_hip_matrix* M, int max_iter);
int x_defer_effective(const hpccg_hip_matrix* M);
bool fuse_update_effective(const hpccg_hip_matrix* M);
bool resident_of(const hpccg_hip_matrix* M);
bool persist_ok(const hpccg_hip_matrix* M);
CgArgs make_args(hpccg_hip_matrix* M, const double* b, double* x, int max_iter, double tol);
void print_trace(const hpccg_hip_matrix* M, int niters, int max_iter);
int solve_ranks(hpccg_hip_matrix* const* Ms, int P, const double* const* b_dev, double* const* x_dev, int max_iter,
                double tol, int* niters_out, double* normr_out, double* times, int print);

template <class T>
int dev_alloc(hpccg_hip_matrix* M, T** p, size_t count, bool zero = false)
{
    const size_t b = sizeof(T) * std::max<size_t>(1, count);
    HIP_TRY(big_malloc(reinterpret_cast<void**>(p), b));
    if (zero) HIP_TRY(hipMemsetAsync(*p, 0, b, M->stream));  // ordered before M's kernels and copies
    M->bytes += (long long)b;
    return 0;
}

template <class T>
void dev_free(hpccg_hip_matrix* M, T** p, size_t count)
{
    if (*p) {
        (void)flush_stream(M);
        big_free(*p);
        M->bytes -= (long long)(sizeof(T) * std::max<size_t>(1, count));
    }
    *p = nullptr;
}

}  // namespace hpccg::host
#pragma GCC visibility pop

// (C linkage and in the dynamic symbol table since they were written, so they stay there)
extern "C" {
int upload_host(hpccg_hip_matrix* M, const double* b, const double* x, bool with_b);
int download_x(hpccg_hip_matrix* M, double* x);
int solve_host(hpccg_hip_matrix* M, const double* b, const double* x, int max_iter, double tolerance, int* niters,
               double* normr, double* times, int print);
}  // extern "C"

#endif  // HPCCG_HOST_DEVICE_FREE

using namespace hpccg::host;
