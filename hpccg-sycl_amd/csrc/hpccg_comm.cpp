// hpccg_comm.cpp -- the error channel, the communicator (RCCL or host-bootstrapped; one rank per GPU
// per process), the in-process group's creation context, and the device and communicator entry points.
#include "hpccg_host.h"

#pragma GCC visibility push(hidden)
namespace hpccg::host {

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------

thread_local std::string g_err;

int set_err(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// the channel for the other units: they read and clear this thread's message through these
const std::string& last_err() { return g_err; }
void clear_err() { g_err.clear(); }

}  // namespace hpccg::host
#pragma GCC visibility pop

namespace hpccg {

// error channel for the other host translation units (read_hpc_row.cpp)
int set_error_message(int code, const char* msg) { return set_err(code, "%s", msg); }

}  // namespace hpccg

#pragma GCC visibility push(hidden)
namespace hpccg::host {

Comm g_comm;
bool comm_host() { return g_comm.ag != nullptr; }
bool comm_up() { return g_comm.comm != nullptr || g_comm.ag != nullptr; }

void comm_reset()
{
    if (g_comm.comm) ncclCommDestroy(g_comm.comm);
    if (g_comm.d_buf) (void)hipFree(g_comm.d_buf);
    if (g_comm.stream) (void)hipStreamDestroy(g_comm.stream);
    g_comm = Comm();
}

// All-gather of `bytes` host bytes per rank into all[nranks * bytes] (rank
// order): RCCL staged through device memory, or the host bootstrap's
// callback. The setup-time exchanges of make_local_matrix.cpp:185-201 /
// :286-587 and the self-tests' verdicts go through here.
int comm_allgather(const void* mine, void* all, size_t bytes)
{
    if (g_comm.nranks == 1 || !comm_up()) {
        std::memcpy(all, mine, bytes);
        return 0;
    }
    if (g_comm.ag) {
        if (g_comm.ag(mine, all, (unsigned long long)bytes, g_comm.ag_ctx) != 0)
            return set_err(HPCCG_HIP_EINVAL, "the host all-gather callback failed (%zu B per rank)", bytes);
        return 0;
    }
    const size_t need = bytes * (size_t)(g_comm.nranks + 1);
    if (!g_comm.stream) HIP_TRY(hipStreamCreateWithFlags(&g_comm.stream, hipStreamNonBlocking));
    if (need > g_comm.buf_bytes) {
        if (g_comm.d_buf) (void)hipFree(g_comm.d_buf);
        g_comm.d_buf = nullptr;
        g_comm.buf_bytes = 0;
        HIP_TRY(hipMalloc(&g_comm.d_buf, need));
        g_comm.buf_bytes = need;
    }
    unsigned char* d = g_comm.d_buf;
    HIP_TRY(hipMemcpyAsync(d + bytes * g_comm.nranks, mine, bytes, hipMemcpyHostToDevice, g_comm.stream));
    NCCL_TRY(ncclAllGather(d + bytes * g_comm.nranks, d, bytes, ncclUint8, g_comm.comm, g_comm.stream));
    HIP_TRY(hipStreamSynchronize(g_comm.stream));
    HIP_TRY(hipMemcpy(all, d, bytes * g_comm.nranks, hipMemcpyDeviceToHost));
    return 0;
}

// Minimum over the ranks of one int (the self-tests' verdicts).
int comm_min(int v, int* out)
{
    std::vector<int> all(std::max(1, g_comm.nranks));
    TRY(comm_allgather(&v, all.data(), sizeof v));
    *out = *std::min_element(all.begin(), all.end());
    return 0;
}

// The job's in-kernel transport verdicts from every rank's own self-test
// results (collective; hpccg_hip_transport_verdict): local = {peer all-reduce,
// halo pull, production protocol} as this rank saw them. The peer all-reduce
// and the pull each stay on only where every rank passed; the protocol test
// counts only where both did, and a protocol failure on any rank turns both
// off on every rank (RCCL then carries the scalars and r's planes). Every
// rank computes the same three values from the same gathered table.
int transport_verdict(const int local[3], int out[3])
{
    TRY(comm_min(local[0] ? 1 : 0, &out[0]));
    TRY(comm_min(local[1] ? 1 : 0, &out[1]));
    TRY(comm_min((out[0] && out[1] && local[2]) ? 1 : 0, &out[2]));
    if (out[0] && out[1] && !out[2]) out[0] = out[1] = 0;
    return 0;
}

thread_local GroupCtx g_group_ctx;

int comm_nranks() { return g_group_ctx.active ? g_group_ctx.nranks : g_comm.nranks; }
int comm_rank() { return g_group_ctx.active ? g_group_ctx.rank : g_comm.rank; }

}  // namespace hpccg::host
#pragma GCC visibility pop

extern "C" {

// ===========================================================================
// C ABI
// ===========================================================================

int hpccg_hip_abi_version(void) { return 2; }

const char* hpccg_hip_last_error(void) { return g_err.c_str(); }

int hpccg_hip_device_count(int* count)
{
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    *count = c;
    return c > 0 ? 0 : set_err(HPCCG_HIP_ENODEV, "no HIP device");
}

int hpccg_hip_set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return 0;
}

int hpccg_hip_comm_unique_id(unsigned char id_out[128])
{
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    std::memcpy(id_out, &id, 128);
    return 0;
}

int hpccg_hip_comm_init(const unsigned char id[128], int nranks, int rank)
{
    if (nranks < 1 || rank < 0 || rank >= nranks) return set_err(HPCCG_HIP_EINVAL, "bad nranks/rank");
    comm_reset();
    // a 1-rank communicator is created too (bootstrap + RCCL check on one GPU);
    // the solver still takes its single-rank path when nranks == 1
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    NCCL_TRY(ncclCommInitRank(&g_comm.comm, nranks, uid, rank));
    g_comm.nranks = nranks;
    g_comm.rank = rank;
    return 0;
}

int hpccg_hip_comm_init_host(int nranks, int rank, hpccg_hip_allgather_fn allgather, void* ctx)
{
    if (nranks < 1 || rank < 0 || rank >= nranks || !allgather)
        return set_err(HPCCG_HIP_EINVAL, "bad nranks/rank or no all-gather callback");
    comm_reset();
    g_comm.nranks = nranks;
    g_comm.rank = rank;
    g_comm.ag = allgather;
    g_comm.ag_ctx = ctx;
    // the callback is collective: every rank must see every rank in order
    std::vector<int> all(nranks, -1);
    int rc = comm_allgather(&rank, all.data(), sizeof rank);
    for (int q = 0; q < nranks && rc == 0; q++)
        if (all[q] != q) rc = set_err(HPCCG_HIP_EINVAL, "host all-gather: slot %d holds rank %d", q, all[q]);
    if (rc) comm_reset();
    return rc;
}

int hpccg_hip_comm_destroy(void)
{
    comm_reset();
    return 0;
}

int hpccg_hip_comm_mode(int* mode)
{
    if (!mode) return set_err(HPCCG_HIP_EINVAL, "mode is NULL");
    *mode = g_comm.comm ? 1 : (g_comm.ag ? 2 : 0);
    return 0;
}

int hpccg_hip_comm_size(int* nranks, int* rank)
{
    if (nranks) *nranks = g_comm.nranks;
    if (rank) *rank = g_comm.rank;
    return 0;
}

int hpccg_hip_comm_allreduce_host(double* vals, int n, int op)
{
    if (!vals || n < 0 || op < 0 || op > 2) return set_err(HPCCG_HIP_EINVAL, "bad argument");
    if (comm_host() && n > 0) {  // every rank's values, reduced in rank order
        std::vector<double> all((size_t)n * g_comm.nranks);
        TRY(comm_allgather(vals, all.data(), sizeof(double) * n));
        for (int i = 0; i < n; i++) {
            double v = op == 0 ? 0.0 : all[i];
            for (int q = 0; q < g_comm.nranks; q++) {
                const double w = all[(size_t)q * n + i];
                v = op == 0 ? v + w : op == 1 ? std::min(v, w) : std::max(v, w);
            }
            vals[i] = v;
        }
        return 0;
    }
    if (!g_comm.comm || n == 0) return 0;
    double* d = nullptr;
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&d, sizeof(double) * n));
    TRY(h2d_stream(s, d, vals, sizeof(double) * n));
    const ncclRedOp_t ops[3] = {ncclSum, ncclMin, ncclMax};
    NCCL_TRY(ncclAllReduce(d, d, n, ncclFloat64, ops[op], g_comm.comm, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(vals, d, sizeof(double) * n, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    (void)hipStreamDestroy(s);
    return 0;
}

int hpccg_hip_transport_verdict(const int local[3], int verdict[3])
{
    if (!local || !verdict) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    if (!comm_up()) return set_err(HPCCG_HIP_EINVAL, "no communicator (hpccg_hip_comm_init / _init_host first)");
    return transport_verdict(local, verdict);
}

int hpccg_hip_runtime_info(int ints_out[6], char* pci_bus_id, int pci_cap, char* rccl_path, char* hip_path,
                           int path_cap)
{
    if (!ints_out) return set_err(HPCCG_HIP_EINVAL, "ints_out is NULL");
    int dev = 0, v = 0;
    HIP_TRY(hipGetDevice(&dev));
    ints_out[0] = ints_out[1] = 0;
    if (g_comm.comm) {
        NCCL_TRY(ncclCommCount(g_comm.comm, &ints_out[0]));
        NCCL_TRY(ncclCommUserRank(g_comm.comm, &ints_out[1]));
    }
    NCCL_TRY(ncclGetVersion(&v));
    ints_out[2] = v;
    HIP_TRY(hipRuntimeGetVersion(&v));
    ints_out[3] = v;
    HIP_TRY(hipDriverGetVersion(&v));
    ints_out[4] = v;
    ints_out[5] = dev;
    if (pci_bus_id && pci_cap > 0) HIP_TRY(hipDeviceGetPCIBusId(pci_bus_id, pci_cap, dev));
    // the files the RCCL and HIP entry points of this library resolved to
    auto where = [](const void* sym, char* out, int cap) {
        Dl_info di;
        if (!out || cap <= 0) return;
        if (dladdr(sym, &di) && di.dli_fname)
            std::snprintf(out, cap, "%s", di.dli_fname);
        else
            std::snprintf(out, cap, "?");
    };
    where(reinterpret_cast<const void*>(&ncclGetVersion), rccl_path, path_cap);
    where(reinterpret_cast<const void*>(&hipRuntimeGetVersion), hip_path, path_cap);
    return 0;
}

int hpccg_hip_device_name(char* buf, int cap, int* cus)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (buf && cap > 0) std::snprintf(buf, cap, "%s (%s)", prop.name[0] ? prop.name : "AMD Instinct GPU", prop.gcnArchName);
    if (cus) *cus = prop.multiProcessorCount;
    return 0;
}

int hpccg_hip_internal_set_error(int code, const char* msg) { return set_err(code, "%s", msg ? msg : ""); }

}  // extern "C"
