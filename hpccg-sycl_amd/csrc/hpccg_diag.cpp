// hpccg_diag.cpp -- diagnostics: the timed SpMV, the placement probe, VMM reallocation, the canary
// check, the block timeline and the slot plan.
#include "hpccg_host.h"

extern "C" {

int hpccg_hip_diag_spmv(hpccg_hip_matrix* M, int kernel, int reps, double* avg_us)
{
    if (!M || !avg_us || reps < 1) return set_err(HPCCG_HIP_EINVAL, "bad argument");
    const bool stream = kernel == kDiagStreamA && M->has_a;
    if (!stream && (!spmv_kernel_ok(kernel) || !kernel_available(M, kernel)))
        return set_err(HPCCG_HIP_EINVAL, "spmv_kernel %d is not available for this matrix", kernel);
    HIP_TRY(hipSetDevice(M->device));
    TRY(ensure_hist(M, 2));
    const int keep = M->kernel;
    if (!stream) M->kernel = kernel;  // make_args sizes the grid for that kernel
    CgArgs a = make_args(M, M->d_b, M->d_x, 2, 0.0);
    M->kernel = keep;
    auto launch = [&]() {
        if (stream)
            launch_stream_a(a, M->stream);
        else
            launch_cg_spmv(a, kernel, true, M->stream);
    };
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    launch();  // warm
    HIP_TRY(hipEventRecord(e0, M->stream));
    for (int i = 0; i < reps; i++) launch();
    HIP_TRY(hipEventRecord(e1, M->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_us = 1e3 * ms / reps;
    return 0;
}

// Physical placement probe: the CG iteration rate of a large
// image depends on where in HBM its values and the p ring were placed (306-350
// us per 200^3 SpMV on one box, same code, same virtual layout). Time a few
// CG iterations on the creation placement and on `tries` candidate
// allocations (each allocated while the earlier ones are held, so each lands
// elsewhere), keep the fastest, free the rest. Values are copied, the ring is
// zeroed as alloc_ring leaves it; nothing else moves and no result changes.
// Off unless asked for (hpccg_hip_set_placement_probe / bench.py --placement).
// Round 3's contiguous candidates found the fast placements and corrupted
// other buffers (big_malloc); plain candidates are safe and rarely faster.
constexpr int kPlaceIters = 10;  // CG iterations per candidate (eager, event-timed)

// Median SpMV + update time (us) of iterations 2.. of a short eager solve on
// scratch b, x. A rank of an RCCL job or a group member is timed as one rank
// (no halo, no all-reduce: the probe must not make collective calls that the
// other ranks' probes might not match; the ghost rows it leaves unwritten are
// the ring's zeros).
int probe_time(hpccg_hip_matrix* M, const double* b, double* x, double* us)
{
    const int nr = M->nranks, ev = M->event_timing, gr = M->use_graph;
    M->nranks = 1;
    M->event_timing = 1;
    M->use_graph = 0;
    int it = 0;
    double normr = 0.0;
    int rc = 0;
    if (hipMemsetAsync(x, 0, sizeof(double) * M->npad, M->stream) != hipSuccess)
        rc = set_err(HPCCG_HIP_EHIP, "placement probe: hipMemsetAsync failed");
    if (!rc) rc = solve_ranks(&M, 1, &b, &x, kPlaceIters, 0.0, &it, &normr, nullptr, 0);
    M->nranks = nr;
    M->event_timing = ev;
    M->use_graph = gr;
    if (rc) return rc;
    std::vector<double> v;
    for (int i = 2; i <= it; i++) v.push_back(M->kiter[2 * i] + M->kiter[2 * i + 1]);
    if (v.empty()) return set_err(HPCCG_HIP_EINVAL, "placement probe: the solve ran %d iterations", it);
    std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
    *us = 1e3 * v[v.size() / 2];
    return 0;
}

// The probe's candidates are plain allocations (big_malloc's reason). Only
// the diagnostics variant of the library (-DHPCCG_DIAG_CONTIG,
// tools/build_variant.sh) lets tools/diag_carry.py ask for others:
// HPCCG_PROBE_ALLOC = hipExtMallocWithFlags flags (4: contiguous -- this
// corrupted other buffers). HPCCG_PROBE_KEEP=1 holds the dropped candidates
// for the life of the process instead of freeing them.
static unsigned probe_alloc_flags()
{
#ifdef HPCCG_DIAG_CONTIG
    const char* e = std::getenv("HPCCG_PROBE_ALLOC");
    return e && *e ? (unsigned)std::atoi(e) : hipDeviceMallocDefault;
#else
    return hipDeviceMallocDefault;
#endif
}
static bool probe_keep()
{
    const char* e = std::getenv("HPCCG_PROBE_KEEP");
    return e && e[0] == '1';
}
static std::vector<double*> g_probe_held;

int hpccg_hip_probe_placement(hpccg_hip_matrix* M, int tries)
{
    if (!M) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    if (tries < 0 || tries > 16) return set_err(HPCCG_HIP_EINVAL, "tries must be 0..16");
    M->place_us.clear();
    M->place_pick = 0;
    if (!tries || !M->has_a || !M->d_aval || !M->d_pbuf) return 0;
    HIP_TRY(hipSetDevice(M->device));
    HIP_TRY(hipStreamSynchronize(M->stream));
    // b | x of the timed solves, each padded to npad rows like the solver's
    // own vectors (the slice kernels load whole slices)
    const size_t n = M->npad;
    double* scratch = nullptr;
    HIP_TRY(hipMalloc(&scratch, 2 * sizeof(double) * n));
    auto done = [&](int rc) {
        (void)flush_stream(M);  // the timed solves ran with the timing events (no system-scope release)
        (void)hipFree(scratch);
        (void)hipGetLastError();  // a refused candidate allocation only ends a phase
        M->trace.clear();         // the probe's solves are not the caller's
        M->last_niters = 0;
        M->kiter.clear();
        for (double& t : M->ktimes) t = 0.0;
        return rc;
    };
    // b: every 32-bit word 0x3ff00000 (each double ~1.0000002; only the rate matters)
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(scratch), 0x3ff00000u, 2 * n, M->stream) != hipSuccess)
        return done(set_err(HPCCG_HIP_EHIP, "placement probe: hipMemsetD32Async failed"));
    double us = 0.0;
    int rc = probe_time(M, scratch, scratch + n, &us);
    if (rc) return done(rc);
    M->place_us.push_back(us);
    double best_us = us;
    // phase 0 places the values (copied), 1 the p ring, 2 r, 3 Ap (zeroed, as
    // workspace allocation leaves them), each against the others' kept placement
    const ptrdiff_t poff = M->d_p - M->d_pbuf, roff = M->d_r - M->d_rbuf;
    for (int phase = 0; phase < kPlacePhases; phase++) {
        if (phase == 2 && M->pull_auto_ok) continue;  // the neighbours have this r mapped (halo_pull)
        double** const slots[kPlacePhases] = {&M->d_aval, &M->d_pbuf, &M->d_rbuf, &M->d_Ap};
        const size_t counts[kPlacePhases] = {(size_t)std::max<long long>(1, M->a_slots),
                                             (size_t)M->pstride * M->ring_alloc, (size_t)M->pstride, M->npad};
        double** slot = slots[phase];
        const size_t bytes = sizeof(double) * counts[phase];
        auto set = [&](double* q) {
            *slot = q;
            if (phase == 1) M->d_p = q + poff;
            if (phase == 2) M->d_r = q + roff;
        };
        std::vector<double*> cand{*slot};
        size_t best = 0;
        for (int t = 0; t < tries && !rc; t++) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < bytes + (size_t(8) << 30)) break;  // headroom
            double* q = nullptr;
            if (big_malloc(reinterpret_cast<void**>(&q), bytes, probe_alloc_flags()) != hipSuccess)
                break;
            cand.push_back(q);
            const hipError_t e = phase == 0 ? hipMemcpyAsync(q, cand[0], bytes, hipMemcpyDeviceToDevice, M->stream)
                                            : hipMemsetAsync(q, 0, bytes, M->stream);
            if (e != hipSuccess) {
                rc = set_err(HPCCG_HIP_EHIP, "placement probe: filling candidate %d failed", t + 1);
                break;
            }
            set(q);
            rc = probe_time(M, scratch, scratch + n, &us);
            if (rc) break;
            M->place_us.push_back(us);
            if (us < best_us) {
                best_us = us;
                best = cand.size() - 1;
            }
        }
        if (rc) best = 0;
        (void)flush_stream(M);  // no launch reads the others any more, and nothing of theirs is left in cache
        set(cand[best]);
        for (size_t i = 0; i < cand.size(); i++)
            if (i != best) {
                if (probe_keep())
                    g_probe_held.push_back(cand[i]);  // diagnostics: never handed out again
                else
                    big_free(cand[i]);
            }
        if (phase > 0 && hipMemsetAsync(cand[best], 0, bytes, M->stream) != hipSuccess && !rc)
            rc = set_err(HPCCG_HIP_EHIP, "placement probe: hipMemsetAsync failed");  // the solves' values
        M->place_pick |= (int)best << (8 * phase);
        if (rc) break;
    }
    return done(rc);
}

int hpccg_hip_diag_placement(const hpccg_hip_matrix* M, double* us_out, int cap)
{
    if (!M || (!us_out && cap > 0)) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    const int n = (int)M->place_us.size();
    for (int i = 0; i < std::min(n, cap); i++) us_out[i] = M->place_us[i];
    return n;
}

// Diagnostics: a mapping through the VMM API at a chosen virtual alignment.
int vmm_alloc(hpccg_hip_matrix* M, size_t bytes, size_t align, double** out)
{
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = M->device;
    size_t gran = 0;
    HIP_TRY(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
    const size_t sz = (bytes + gran - 1) / gran * gran;
    // reserve align more and map at an aligned address inside (the
    // reservation's own alignment argument is not honoured above 2 MB here)
    align = std::max(align, gran);
    void* res = nullptr;
    HIP_TRY(hipMemAddressReserve(&res, sz + align, gran, nullptr, 0));
    const uintptr_t a0 = (reinterpret_cast<uintptr_t>(res) + align - 1) / align * align;
    void* va = reinterpret_cast<void*>(a0);
    hipMemGenericAllocationHandle_t h;
    HIP_TRY(hipMemCreate(&h, sz, &prop, 0));
    HIP_TRY(hipMemMap(va, sz, 0, h, 0));
    hipMemAccessDesc ad = {};
    ad.location = prop.location;
    ad.flags = hipMemAccessFlagsProtReadWrite;
    HIP_TRY(hipMemSetAccess(va, sz, &ad, 1));
    M->vmm.push_back({va, sz, h, res, sz + align});
    *out = static_cast<double*>(va);
    return 0;
}

int hpccg_hip_diag_realloc(hpccg_hip_matrix* M, int which, unsigned long long* va_out)
{
    if (!M) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    const int mode = which >> 8;
    which &= 255;
    HIP_TRY(hipSetDevice(M->device));
    HIP_TRY(hipStreamSynchronize(M->stream));
    double** buf;
    size_t n;
    switch (which) {
    case 0: buf = &M->d_aval; n = (size_t)std::max<long long>(1, M->a_slots); break;
    case 1: buf = &M->d_pbuf; n = (size_t)M->pstride * M->ring_alloc; break;
    case 2: buf = &M->d_rbuf; n = (size_t)M->pstride; break;
    case 3: buf = &M->d_Ap; n = M->npad; break;
    case 4: buf = &M->d_x; n = M->npad; break;
    default: return set_err(HPCCG_HIP_EINVAL, "which must be 0..4");
    }
    if (mode < 0 || mode > 6) return set_err(HPCCG_HIP_EINVAL, "mode must be 0..6");
#ifndef HPCCG_DIAG_CONTIG
    if (mode == 1)
        return set_err(HPCCG_HIP_EINVAL, "mode 1 (physically contiguous memory) exists only in the diagnostics "
                                         "variant of the library (-DHPCCG_DIAG_CONTIG): it corrupted other buffers");
#endif
    if (!*buf) return set_err(HPCCG_HIP_EINVAL, "buffer %d not allocated", which);
    // the neighbours pull from this r through their IPC mappings of it (halo_pull):
    // a moved r would leave them reading the old buffer
    if (which == 2 && M->pull_auto_ok)
        return set_err(HPCCG_HIP_EINVAL, "r cannot move: the neighbours have it mapped (halo_pull)");
    double* nb = nullptr;
    const size_t bytes = sizeof(double) * n;
    if (mode == 0) {
        HIP_TRY(big_malloc(reinterpret_cast<void**>(&nb), bytes));
#ifdef HPCCG_DIAG_CONTIG
    } else if (mode == 1) {
        HIP_TRY(big_malloc(reinterpret_cast<void**>(&nb), bytes, hipDeviceMallocContiguous));
#endif
    } else if (mode == 5) {  // fine-grained (coherent) device memory
        HIP_TRY(big_malloc(reinterpret_cast<void**>(&nb), bytes, hipDeviceMallocFinegrained));
    } else if (mode == 6) {
        HIP_TRY(big_malloc(reinterpret_cast<void**>(&nb), bytes, hipDeviceMallocUncached));
    } else {  // VMM at 2 MB, 64 MB or 1 GB virtual alignment
        const size_t align = mode == 2 ? (size_t(1) << 21) : mode == 3 ? (size_t(1) << 26) : (size_t(1) << 30);
        TRY(vmm_alloc(M, bytes, align, &nb));
    }
    HIP_TRY(hipMemcpyAsync(nb, *buf, bytes, hipMemcpyDeviceToDevice, M->stream));
    HIP_TRY(hipStreamSynchronize(M->stream));
    bool mapped = false;  // a VMM mapping is released at destroy, not hipFree'd
    for (const auto& v : M->vmm) mapped = mapped || v.va == *buf;
    if (!mapped) M->graveyard.push_back(*buf);  // held: the new buffer gets other physical memory
    const ptrdiff_t poff = M->d_p - M->d_pbuf, roff = M->d_r - M->d_rbuf;
    *buf = nb;
    if (which == 1) M->d_p = M->d_pbuf + poff;
    if (which == 2) M->d_r = M->d_rbuf + roff;
    if (va_out) *va_out = reinterpret_cast<unsigned long long>(nb);
    return 0;  // the graph cache compares kernel arguments: the next solve re-captures
}

int hpccg_hip_diag_canary_check(int* enabled, char* report, int cap)
{
    if (enabled) *enabled = canary_on() ? 1 : 0;
    std::string rep;
    const int bad = canary_check(&rep);
    if (report && cap > 0) std::snprintf(report, (size_t)cap, "%s", rep.c_str());
    return bad;
}

int hpccg_hip_diag_timeline(const hpccg_hip_matrix* M, unsigned long long* out, int cap)
{
    if (!M || !out) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    if (!M->d_tl) return set_err(HPCCG_HIP_EINVAL, "dbg_timeline is off");
    const int n = std::min(cap, M->tl_units);
    HIP_TRY(hipSetDevice(M->device));
    HIP_TRY(hipStreamSynchronize(M->stream));
    HIP_TRY(hipMemcpy(out, M->d_tl, (size_t)n * kTlWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return n;
}

int hpccg_hip_diag_slot_plan(int units, int grid, int spu, int rev, int* last_unit, int cap, int* top_group)
{
    if (!last_unit || !top_group || units < 1) return set_err(HPCCG_HIP_EINVAL, "bad argument");
    const int ng = (units * spu + 63) / 64;
    if (ng > cap) return set_err(HPCCG_HIP_EINVAL, "cap %d < %d groups", cap, ng);
    const int r = slot_plan(units, grid, spu, rev, last_unit, top_group);
    if (r < 0) return set_err(HPCCG_HIP_EINVAL, "bad launch shape");
    return r;
}

}  // extern "C"
