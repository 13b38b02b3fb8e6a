// hpccg_dropin.cpp -- C++ entry points with the reference signatures
// (HPCCG.hpp:61-63, generate_matrix.hpp:58) forwarding to the C ABI.
// Also the drop-in's cache of device matrices (hpccg_hip_HPCCG): one per caller matrix, keyed by its
// address and a fingerprint of its contents.
#include <iostream>

#include "../../include/HPCCG.hpp"
#include "../../include/hpccg_hip.h"
#include "hpccg_host.h"

#pragma GCC visibility push(hidden)
namespace hpccg::host {

// ---- drop-in cache (hpccg_hip_HPCCG) ----------------------------------------
// A device matrix per caller HPC_Sparse_Matrix, keyed by its address AND a
// fingerprint of its contents (sizes, row lengths, every column index and
// value), so a matrix destroyed and re-created at the same address, or edited
// in place, is converted again instead of reusing a stale image.
struct DropinEntry {
    unsigned long long fp = 0;
    hpccg_hip_matrix* M = nullptr;
};
std::mutex g_dropin_mu;
std::map<const void*, DropinEntry> g_dropin_cache;

inline unsigned long long mix64(unsigned long long h, unsigned long long v)
{
    h ^= v + 0x9e3779b97f4a7c15ULL + (h << 6) + (h >> 2);
    return h * 0xff51afd7ed558ccdULL;
}

unsigned long long fingerprint(const HPC_Sparse_Matrix* A)
{
    const int n = A->local_nrow;
    unsigned long long head = mix64(0x1234, (unsigned long long)(unsigned)n);
    head = mix64(head, (unsigned long long)(unsigned)A->start_row);
    head = mix64(head, (unsigned long long)(unsigned)A->total_nrow);
    head = mix64(head, (unsigned long long)(unsigned)A->local_ncol);
    const int nth = std::max(1, std::min<int>(16, (int)std::thread::hardware_concurrency()));
    std::vector<unsigned long long> part(nth, 0);
    auto work = [&](int t) {
        const int r0 = (int)((long long)n * t / nth), r1 = (int)((long long)n * (t + 1) / nth);
        unsigned long long h = (unsigned long long)t;
        for (int i = r0; i < r1; i++) {
            const int len = A->nnz_in_row[i];
            h = mix64(h, (unsigned long long)(unsigned)len);
            const double* v = A->ptr_to_vals_in_row[i];
            const int* c = A->ptr_to_inds_in_row[i];
            for (int j = 0; j < len; j++) {
                unsigned long long bits;
                std::memcpy(&bits, v + j, 8);
                h = mix64(h, bits ^ ((unsigned long long)(unsigned)c[j] << 17));
            }
        }
        part[t] = h;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nth; t++) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
    for (int t = 0; t < nth; t++) head = mix64(head, part[t]);
    return head;
}

}  // namespace hpccg::host
#pragma GCC visibility pop

extern "C" {

int hpccg_hip_HPCCG(HPC_Sparse_Matrix* A, double* b, double* x, int max_iter, double tolerance, int* niters,
                    double* normr, double* times)
{
    if (!A || !b || !x || !niters || !normr) return set_err(HPCCG_HIP_EINVAL, "NULL argument");
    if (A->local_ncol != A->local_nrow)
        return set_err(HPCCG_HIP_EPLAN,
                       "A has local_ncol %d != local_nrow %d: it has been through make_local_matrix (local column "
                       "indices); pass the matrix with global column indices",
                       A->local_ncol, A->local_nrow);
    // A cached image is solved on at once, while host threads fingerprint A
    // (~23 ms at 200^3, 12 % of the solve); x is written back only if the
    // fingerprint still matches -- otherwise A changed since it was cached, and
    // the image is rebuilt and the solve run again from the caller's x.
    hpccg_hip_matrix* M = nullptr;
    unsigned long long cached_fp = 0;
    {
        std::lock_guard<std::mutex> lk(g_dropin_mu);
        auto it = g_dropin_cache.find(A);
        // (the sizes first: the speculative solve reads nrow values of b and x)
        if (it != g_dropin_cache.end() && it->second.M->nrow == A->local_nrow &&
            it->second.M->start_row == A->start_row && it->second.M->total_nrow == A->total_nrow)
            M = it->second.M, cached_fp = it->second.fp;
    }
    if (M) {
        unsigned long long fp = 0;
        std::thread fth;
        try {
            fth = std::thread([&] { fp = fingerprint(A); });
        } catch (const std::system_error&) {  // no thread to spare: fingerprint first
            fp = fingerprint(A);
        }
        const int rc = solve_host(M, b, x, max_iter, tolerance, niters, normr, times, 0);
        if (fth.joinable()) fth.join();
        if (fp == cached_fp) {
            TRY(rc);
            print_trace(M, *niters, max_iter);
            return download_x(M, x);
        }
        (void)hipGetLastError();
        clear_err();
    }
    double setup = 0.0;
    {
        std::lock_guard<std::mutex> lk(g_dropin_mu);
        const auto t0 = std::chrono::steady_clock::now();
        const unsigned long long fp = fingerprint(A);
        auto it = g_dropin_cache.find(A);
        if (it != g_dropin_cache.end() && it->second.fp == fp) {
            M = it->second.M;
        } else {
            if (it != g_dropin_cache.end()) {  // same address, other contents: a new matrix
                free_matrix(it->second.M);
                g_dropin_cache.erase(it);
            }
            TRY(hpccg_hip_matrix_create(A, &M));
            g_dropin_cache[A] = DropinEntry{fp, M};
        }
        setup = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    TRY(hpccg_hip_solve(M, b, x, max_iter, tolerance, niters, normr, times, 1));
    if (times) times[6] += setup;
    return 0;
}

int hpccg_hip_dropin_release(const HPC_Sparse_Matrix* A)
{
    std::lock_guard<std::mutex> lk(g_dropin_mu);
    auto it = g_dropin_cache.find(A);
    if (it == g_dropin_cache.end()) return 0;
    free_matrix(it->second.M);
    g_dropin_cache.erase(it);
    return 1;
}

int hpccg_hip_dropin_cached(const HPC_Sparse_Matrix* A)
{
    std::lock_guard<std::mutex> lk(g_dropin_mu);
    return g_dropin_cache.count(A) ? 1 : 0;
}

}  // extern "C"

int HPCCG(HPC_Sparse_Matrix* A, double* const b, double* const x, const int max_iter,
          const double tolerance, int& niters, double& normr, double* times)
{
    int it = 0;
    double nr = 0.0;
    const int rc = hpccg_hip_HPCCG(A, b, x, max_iter, tolerance, &it, &nr, times);
    if (rc) std::cerr << "hpccg_hip: " << hpccg_hip_last_error() << std::endl;
    niters = it;
    normr = nr;
    return rc;
}

void generate_matrix(int nx, int ny, int nz, HPC_Sparse_Matrix** A, double** x, double** b,
                     double** xexact)
{
    hpccg_generate_matrix(nx, ny, nz, 0, 1, 0, A, x, b, xexact);
}
