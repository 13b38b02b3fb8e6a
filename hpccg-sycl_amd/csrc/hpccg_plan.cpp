// hpccg_plan.cpp -- the device-free planning of the main library: which halo plan serves a
// partition (z-slab or gather), what each rank packs for its requesters, and the C entry points of the
// SELL-512 builder and the slab, gather and halo plans. Includes no HIP or RCCL header.
#define HPCCG_HOST_DEVICE_FREE
#include "hpccg_host.h"

#pragma GCC visibility push(hidden)
namespace hpccg::host {

// Can the z-slab plan serve rank r? (ghosts from rank+-1 only, contiguous,
// the planes those ranks own; the condition hpccg_slab_plan enforces)
bool slab_serves(const int* info, int P, int r)
{
    const int* me = info + 4 * r;
    const int glo = me[1], ghi = me[2];
    if (glo > 0 && (r == 0 || glo > info[4 * (r - 1)])) return false;
    if (ghi > 0 && (r == P - 1 || ghi > info[4 * (r + 1)])) return false;
    if (r > 0 && info[4 * (r - 1) + 3] + info[4 * (r - 1)] != me[3]) return false;
    return true;
}

// 1 = slab plan for every rank, 2 = gather plan for every rank (all ranks decide
// the same from the same all-gathered info).
int choose_halo_mode(const int* info, int P)
{
    if (g_halo_mode == 2) return 2;
    for (int r = 0; r < P; r++)
        if (!slab_serves(info, P, r)) return g_halo_mode == 1 ? -1 : 2;
    return 1;
}

int owner_of(long long c, const int* info, int P)  // make_local_matrix.cpp:165-173
{
    int lo = 0, hi = P - 1;
    while (lo < hi) {  // last rank whose start_row <= c
        const int mid = (lo + hi + 1) / 2;
        if (info[4 * mid + 3] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// What rank r packs for its requesters, from every rank's requests
// (reqs_to_me[q] = the global columns rank q needs from r, q's order).
void gather_sends(long long start, const std::vector<std::vector<int>>& reqs_to_me, GatherPlan& g)
{
    g.send_rank.clear();
    g.send_off.clear();
    g.send_cnt.clear();
    g.send_idx.clear();
    for (int q = 0; q < (int)reqs_to_me.size(); q++) {
        if (reqs_to_me[q].empty()) continue;
        g.send_rank.push_back(q);
        g.send_off.push_back((int)g.send_idx.size());
        g.send_cnt.push_back((int)reqs_to_me[q].size());
        for (int c : reqs_to_me[q]) g.send_idx.push_back((int)(c - start));
    }
}

}  // namespace hpccg::host
#pragma GCC visibility pop

extern "C" {

long long hpccg_sell_build(int nrow, long long col_base, long long ncol_ext, const long long* row_ptr, const int* cols,
                           const double* vals, unsigned int* slice_base, int* sell_cols, double* sell_vals)
{
    auto row_len = [row_ptr](int i) { return (int)(row_ptr[i + 1] - row_ptr[i]); };
    auto row_at = [row_ptr, cols, vals](int i, int j, long long* c, double* v) {
        *c = cols[row_ptr[i] + j];
        *v = vals ? vals[row_ptr[i] + j] : 0.0;
    };
    std::vector<unsigned int> tmp;
    if (!slice_base) {
        tmp.resize((nrow + kSliceRows - 1) / kSliceRows + 1);
        slice_base = tmp.data();
    }
    const long long var =
        sell_build_impl(nrow, SlabCols{col_base, ncol_ext}, row_len, row_at, slice_base, nullptr, nullptr, 0, nullptr);
    const long long uni =
        sell_build_impl(nrow, SlabCols{col_base, ncol_ext}, row_len, row_at, slice_base, nullptr, nullptr, 1, nullptr);
    const int uniform = (uni <= var + var / 25) ? 1 : 0;
    int bad = 0;
    const long long r = sell_build_impl(nrow, SlabCols{col_base, ncol_ext}, row_len, row_at, slice_base, sell_cols,
                                        sell_vals, uniform, &bad);
    return bad ? HPCCG_HIP_EPLAN : r;
}

int hpccg_gather_plan(int nranks, const int* info, int nrow, int start_row, const long long* row_ptr, const int* cols,
                      int cap, int* ext_global, int* num_external, int* nrecv, int* recv_rank, int* recv_off,
                      int* recv_cnt)
{
    if (nranks < 1 || !info || nrow < 0 || (nrow > 0 && (!row_ptr || !cols)) || !num_external || !nrecv)
        return set_err(HPCCG_HIP_EINVAL, "bad argument");
    GatherPlan g;
    gather_externals(
        nrow, start_row, info, nranks, [row_ptr](int i) { return (int)(row_ptr[i + 1] - row_ptr[i]); },
        [row_ptr, cols](int i, int j, long long* c, double* v) {
            *c = cols[row_ptr[i] + j];
            *v = 0.0;
        },
        g);
    *num_external = (int)g.ext_global.size();
    *nrecv = (int)g.recv_rank.size();
    if (ext_global && cap >= *num_external)
        for (int j = 0; j < *num_external; j++) ext_global[j] = (int)g.ext_global[j];
    if (recv_rank && recv_off && recv_cnt && cap >= *nrecv)
        for (int i = 0; i < *nrecv; i++) {
            recv_rank[i] = g.recv_rank[i];
            recv_off[i] = g.recv_off[i];
            recv_cnt[i] = g.recv_cnt[i];
        }
    return 0;
}

int hpccg_slab_plan(int nranks, int rank, const int* info, int sends[2])
{
    if (nranks < 1 || rank < 0 || rank >= nranks || !info || !sends) return set_err(HPCCG_HIP_EINVAL, "bad argument");
    const int r = rank, P = nranks;
    const int* me = info + 4 * r;
    const int nrow = me[0], ghost_lo = me[1], ghost_hi = me[2], start_row = me[3];
    // ghosts must come from the adjacent ranks only, contiguously
    if (ghost_lo > 0 && (r == 0 || ghost_lo > info[4 * (r - 1)]))
        return set_err(HPCCG_HIP_EPLAN, "rank %d: ghost_lo %d not owned by rank %d", r, ghost_lo, r - 1);
    if (ghost_hi > 0 && (r == P - 1 || ghost_hi > info[4 * (r + 1)]))
        return set_err(HPCCG_HIP_EPLAN, "rank %d: ghost_hi %d not owned by rank %d", r, ghost_hi, r + 1);
    if (r > 0 && info[4 * (r - 1) + 3] + info[4 * (r - 1)] != start_row)
        return set_err(HPCCG_HIP_EPLAN, "rank %d: row ranges are not contiguous", r);
    sends[0] = (r > 0) ? info[4 * (r - 1) + 2] : 0;      // rank-1's ghost_hi: our first rows
    sends[1] = (r < P - 1) ? info[4 * (r + 1) + 1] : 0;  // rank+1's ghost_lo: our last rows
    if (sends[0] > nrow || sends[1] > nrow) return set_err(HPCCG_HIP_EPLAN, "rank %d: neighbour needs more rows than owned", r);
    return 0;
}

int hpccg_halo_plan(int nrow, int start_row, int total_nrow, const long long* row_ptr, const int* cols, int plan_out[4])
{
    long long mn = start_row, mx = (long long)start_row + nrow - 1;
    for (long long e = 0; e < (nrow > 0 ? row_ptr[nrow] : 0); e++) {
        mn = std::min<long long>(mn, cols[e]);
        mx = std::max<long long>(mx, cols[e]);
    }
    if (mn < 0 || mx >= total_nrow) return set_err(HPCCG_HIP_EPLAN, "column outside [0, total_nrow)");
    plan_out[0] = (int)(start_row - mn);
    plan_out[1] = (int)(mx - ((long long)start_row + nrow - 1));
    plan_out[2] = (int)mn;
    plan_out[3] = (int)mx;
    return 0;
}

}  // extern "C"
