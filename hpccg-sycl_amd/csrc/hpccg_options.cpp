// hpccg_options.cpp -- the per-matrix option tables and the three library-wide creation settings.
#include "hpccg_host.h"

#pragma GCC visibility push(hidden)
namespace hpccg::host {

int g_halo_mode = 0;  // 0 auto (slab when it serves every rank), 1 slab only, 2 gather
int g_keep_sell = 0;  // keep the SELL-512 image beside SELL-512-A (kernel A/B, diagnostics)
// placement probe at creation: -1 auto (images over kPlaceMinBytes), 0 off, n
// candidates. Off by default since round 4: the probe's gain is
// box-dependent and it is asked for explicitly (bench.py --placement).
int g_place_tries = 0;

}  // namespace hpccg::host
#pragma GCC visibility pop

extern "C" {

int hpccg_hip_set_halo_mode(int mode)
{
    if (mode < 0 || mode > 2) return set_err(HPCCG_HIP_EINVAL, "halo mode must be 0, 1 or 2");
    g_halo_mode = mode;
    return 0;
}

int hpccg_hip_set_keep_sell(int keep)
{
    g_keep_sell = keep ? 1 : 0;
    return 0;
}

int hpccg_hip_set_placement_probe(int tries)
{
    if (tries < -1 || tries > 16) return set_err(HPCCG_HIP_EINVAL, "placement probe: -1 (auto), 0 (off) or 1..16");
    g_place_tries = tries;
    return 0;
}

// Options (hpccg_hip.h documents each): twelve settings of the solve --
// use_graph, spmv_kernel, fuse_p, fold, x_defer, x_ring, fuse_update,
// resident_update, graph_chunk, a2_ring, peer_allreduce, halo_pull -- and
// diagnostics (event_timing, force_comm, spin_budget_us, nt, dbg_*). Variants
// that measured even or slower than the defaults were removed (DESIGN.md 4,
// "What was dropped"); git history keeps them.
int hpccg_hip_set_option(hpccg_hip_matrix* M, const char* key, long long value)
{
    if (!M || !key) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    if (!std::strcmp(key, "use_graph")) {
        M->use_graph = (int)value;
    } else if (!std::strcmp(key, "event_timing")) {
        M->event_timing = (int)value;
    } else if (!std::strcmp(key, "fuse_p")) {
        M->fuse_p = value < 0 ? -1 : (value ? 1 : 0);
    } else if (!std::strcmp(key, "x_defer")) {
        if (value < 0 || value > 2)
            return set_err(HPCCG_HIP_EINVAL, "x_defer must be 0 (every iteration), 1 (batched in the update) or 2 "
                                             "(beside the SpMV)");
        M->x_defer = (int)value;
    } else if (!std::strcmp(key, "x_ring")) {
        if (value != -1 && (value < 2 || value > kXRingMax))
            return set_err(HPCCG_HIP_EINVAL, "x_ring must be -1 (auto) or 2..%d", kXRingMax);
        const int prev = M->x_ring;
        M->x_ring = (int)value;
        if (x_ring_effective(M) > M->ring_alloc) {
            HIP_TRY(hipSetDevice(M->device));
            HIP_TRY(hipStreamSynchronize(M->stream));
            const int rc = alloc_ring(M, x_ring_effective(M));
            if (rc) {
                M->x_ring = prev;
                return rc;
            }
        }
    } else if (!std::strcmp(key, "fuse_update")) {
        M->fuse_update = value < 0 ? -1 : (value > 2 ? 2 : (int)value);
    } else if (!std::strcmp(key, "resident_update")) {
        if (value < -1 || value > 1)
            return set_err(HPCCG_HIP_EINVAL, "resident_update: -1 (auto: the persistent launch where it fits), 0 off "
                                             "or 1 (the per-iteration resident launch only)");
        M->resident_update = (int)value;
        if (value) M->resident_failed = 0;
    } else if (!std::strcmp(key, "nt")) {
        if (value < -1 || value > 1)
            return set_err(HPCCG_HIP_EINVAL, "nt must be -1 (auto: images beyond the Infinity Cache), 0 or 1");
        M->nt_opt = (int)value;  // (the graph cache compares the kernel arguments: a changed a.nt re-captures)
    } else if (!std::strcmp(key, "graph_chunk")) {
        if (value < 1 || value > 4096) return set_err(HPCCG_HIP_EINVAL, "graph_chunk must be 1..4096");
        M->graph_iters = (int)value;
    } else if (!std::strcmp(key, "fold")) {
        if (value < -1 || value > 1)
            return set_err(HPCCG_HIP_EINVAL, "fold must be -1 (auto: both dots in their producers), 1 or 0 (k_finalize)");
        M->fold = (int)value;
    } else if (!std::strcmp(key, "a2_ring")) {
        if (value != -1 && value != 0 && value != kA2RingDefault)
            return set_err(HPCCG_HIP_EINVAL, "a2_ring must be -1 (auto: %d), 0 (register loads) or %d", kA2RingDefault,
                           kA2RingDefault);
        M->a2_ring = value < 0 ? kA2RingDefault : (int)value;
    } else if (!std::strcmp(key, "force_comm")) {
        if (value < 0 || value > 2) return set_err(HPCCG_HIP_EINVAL, "force_comm is 0, 1 or 2");
        M->force_comm = (int)value;
    } else if (!std::strcmp(key, "spin_budget_us")) {
        if (value < 1 || value > 20000000LL) return set_err(HPCCG_HIP_EINVAL, "spin_budget_us must be 1..2e7");
        M->spin_us = value;
    } else if (!std::strcmp(key, "peer_allreduce")) {
        M->peer_ar = value < 0 ? -1 : (value ? 1 : 0);
    } else if (!std::strcmp(key, "halo_pull")) {
        // -1 auto, 0 off (the RCCL / peer-copy planes), 1 k_pull where possible, 2 in-launch where the
        // peer all-reduce runs (else 1); 3 (diagnostics, the 1-rank emulation): in-launch with no rows
        M->halo_pull = value < 0 ? -1 : (value > 3 ? 3 : (int)value);
    } else if (!std::strcmp(key, "dbg_timeline")) {
        if (value != 0 && value != 1) return set_err(HPCCG_HIP_EINVAL, "dbg_timeline must be 0 or 1");
        HIP_TRY(hipSetDevice(M->device));
        if (M->d_tl) {
            dev_free(M, &M->d_tl, (size_t)M->tl_units * kTlWords);
            M->tl_units = 0;
        }
        if (value) {
            M->tl_units = 3 * M->nslices + 1024;  // >= the blocks of any SpMV launch (units, side, ghost, update)
            TRY(dev_alloc(M, &M->d_tl, (size_t)M->tl_units * kTlWords, true));
        }  // the graph cache compares the kernel arguments: a changed dbg_tl re-captures
    } else if (!std::strcmp(key, "dbg_resident_stall")) {
        M->dbg_resident_stall = value ? 1 : 0;
    } else if (!std::strcmp(key, "dbg_withhold")) {
        if (value < 0 || value > M->nslices) return set_err(HPCCG_HIP_EINVAL, "dbg_withhold must be 0..nslices");
        M->dbg_withhold = (int)value;
    } else if (!std::strcmp(key, "spmv_kernel")) {
        if (value != -1 && !spmv_kernel_ok((int)value))
            return set_err(HPCCG_HIP_EINVAL, "spmv_kernel must be -1 (auto), 0 (SELL-512), 1 (SELL-512-A direct) or "
                                             "2 (SELL-512-A pair windows)");
        if (value >= 0 && !kernel_available(M, (int)value))
            return set_err(HPCCG_HIP_EINVAL, "spmv_kernel %lld: its image was not built for this matrix%s", value,
                           value == kSpmvSell ? " (hpccg_hip_set_keep_sell(1) before creation keeps SELL-512)" : "");
        M->kernel_opt = (int)value;
        M->kernel = choose_kernel(M);
    } else {
        return set_err(HPCCG_HIP_EINVAL, "unknown option '%s'", key);
    }
    return 0;
}

int hpccg_hip_get_option(const hpccg_hip_matrix* M, const char* key, long long* value)
{
    if (!M || !key || !value) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    if (!std::strcmp(key, "use_graph")) *value = M->use_graph;
    else if (!std::strcmp(key, "spmv_kernel")) *value = M->kernel;
    else if (!std::strcmp(key, "event_timing")) *value = M->event_timing;
    else if (!std::strcmp(key, "fuse_p")) *value = fuse_p_effective(M) ? 1 : 0;
    else if (!std::strcmp(key, "fold")) *value = fold_effective(M);
    else if (!std::strcmp(key, "x_defer")) *value = x_defer_effective(M);
    else if (!std::strcmp(key, "x_ring")) *value = x_ring_effective(M);
    else if (!std::strcmp(key, "fuse_update")) *value = fuse_update_effective(M) ? 1 : 0;
    else if (!std::strcmp(key, "resident_update"))
        *value = persist_ok(M) ? kResidentAuto : resident_of(M) ? 1 : 0;
    else if (!std::strcmp(key, "resident_retries")) *value = M->resident_retries;
    else if (!std::strcmp(key, "halo_mode")) *value = M->nranks == 1 ? 0 : (M->general ? 2 : 1);
    else if (!std::strcmp(key, "graph_chunk")) {  // effective: see graph_chunk_of
        long long c = std::max(1, M->graph_iters);
        if (fuse_update_effective(M)) c += c & 1;
        if (multi_of(M) && !rhalo_of(M)) {
            const long long ring = x_defer_effective(M) ? x_ring_effective(M) : (fuse_p_effective(M) ? 2 : 1);
            c = (c + ring - 1) / ring * ring;
        }
        *value = c;
    }
    else if (!std::strcmp(key, "graph_used")) *value = M->graph_used;
    else if (!std::strcmp(key, "force_comm")) *value = M->force_comm;
    else if (!std::strcmp(key, "spin_budget_us")) *value = M->spin_us;
    else if (!std::strcmp(key, "dbg_withhold")) *value = M->dbg_withhold;
    else if (!std::strcmp(key, "dbg_timeline")) *value = M->d_tl ? 1 : 0;
    else if (!std::strcmp(key, "peer_allreduce")) *value = peer_ar_of(M) ? 1 : 0;
    else if (!std::strcmp(key, "group_fold")) *value = M->gfold_used;
    else if (!std::strcmp(key, "rhalo")) *value = rhalo_of(M) ? 1 : 0;
    else if (!std::strcmp(key, "halo_pull")) {
        CgArgs a{};
        a.peer_ar = peer_ar_of(M) ? 1 : 0;
        a.fold = fold_effective(M);
        *value = pull_of(M) ? (pull_in_of(M, a) ? 2 : 1) : 0;
    }
    else if (!std::strcmp(key, "a2_ring")) *value = a2_ring_effective(M);
    else if (!std::strcmp(key, "nt_store")) *value = nt_store_effective(M) ? 1 : 0;
    else if (!std::strcmp(key, "num_external")) *value = M->general ? M->ghost_hi : M->ghost_lo + M->ghost_hi;
    else if (!std::strcmp(key, "has_sell")) *value = M->has_sell;
    else if (!std::strcmp(key, "has_a")) *value = M->has_a;
    else if (!std::strcmp(key, "a_reject")) *value = M->a_reject;
    else if (!std::strcmp(key, "has_pairs")) *value = M->has_pairs;
    else if (!std::strcmp(key, "a_width")) *value = M->a_width;
    else if (!std::strcmp(key, "lds_doubles")) *value = M->has_pairs ? M->alds2_doubles : 0;
    else if (!std::strcmp(key, "nt")) *value = nt_load_of(M) ? 1 : 0;
    else if (!std::strcmp(key, "device_bytes")) *value = M->bytes;
    else if (!std::strcmp(key, "placement_pick")) *value = M->place_pick;
    else if (!std::strcmp(key, "peer_auto_ok")) *value = M->peer_auto_ok;
    else if (!std::strcmp(key, "pull_auto_ok")) *value = M->pull_auto_ok;
    else if (!std::strcmp(key, "proto_auto_ok")) *value = M->proto_auto_ok;
    else if (!std::strcmp(key, "persist_auto_ok")) *value = M->persist_auto_ok;
    else return set_err(HPCCG_HIP_EINVAL, "unknown option '%s'", key);
    return 0;
}

}  // extern "C"
