// hpccg_srcg_host.h -- the host code that the single-reduction units share
// (hpccg_srcg.hip, hpccg_srpoly.hip and, under hpccg_srcg_group_host.h,
// hpccg_srcg_group.hip and hpccg_srpoly_group.hip): the recurrence's plain
// columns p and s, the launchers of the prologue's t kernel, of the fused step
// and of the finalize, and for the one-rank units the launch loop of the
// Chronopoulos-Gear recurrence with the frame around it. It stands on
// hpccg_onerank_host.h (the launch dispatch, the solve) and compiles nothing of
// hpccg_group.h's.
// A unit hands over one traits struct U: what hpccg_onerank_host.h asks for and
//   t<kR>, finalize       its kernels, as (a template of) kernel pointers
//   fused_step<kR>(w)     its step kernel for kR columns in workspace w (the
//                         polynomial units: by w's degree)
// Its Workspace is a SrcgColumns. The __global__ entry points and the
// extern "C" definitions stay in the units. Internal linkage (each unit
// compiles its own copy), like hpccg_columns.h.
#pragma once
#include "hpccg_onerank_host.h"
#include "hpccg_srcg_bodies.h"

namespace hpccg {

namespace {

// What a single-reduction unit's workspace adds to its columns.
struct SrcgColumns {
    double *pd = nullptr, *sd = nullptr;  // p and s = A p (never zeroed again: k == 1 reads u and w)

    void free_ps()
    {
        for (double* q : {pd, sd})
            if (q) (void)hipFree(q);
        pd = sd = nullptr;
    }
};

// p and s of count entries each, in w's own workspace.
template <class W>
int alloc_ps(W* w, size_t count)
{
    TRY(alloc_zero(w, &w->pd, count));
    return alloc_zero(w, &w->sd, count);
}

// The prologue's t = x + 0 x (col_p's prologue form).
template <class U>
void launch_srcg_t(const typename U::Workspace* w, const typename U::Args& a)
{
    launch_chunks(w, a, true, [](auto r) { return U::template t<decltype(r)::value>; });
}

template <class U>
void launch_srcg_step(const typename U::Workspace* w, const typename U::Args& a, bool prologue)
{
    launch_chunks(w, a, prologue, [w](auto r) { return U::template fused_step<decltype(r)::value>(w); });
}

// store_total: 0 on one rank; 1 for a group member's part, whose state is the group sum's.
template <class U>
void launch_srcg_finalize(const typename U::Workspace* w, const typename U::Args& a, int store_total)
{
    hipLaunchKernelGGL(U::finalize, dim3(a.nrhs), dim3(kFinThreads), 0, w->v.stream, a, store_total);
}

// One recurrence per column of the states on the device, on (b, x) of a: the
// prologue (t, A t, r and u, A u, the three totals), then iterations
// 1 .. kmax - 1 of step (a polynomial unit's with its d steps), SpMM of u,
// finalize, launched eagerly on the matrix's stream. Every kCheckEvery
// iterations the host reads the "columns ended" word and stops launching once
// every column has ended. The launchers are the unit's, as run_recurrence
// (hpccg_columns.h) takes them.
template <class W, class A>
int run_srcg_recurrence(W* w, const A& a, int nrhs, int kmax, void (*launch_t)(const W*, const A&),
                        void (*launch_spmm)(const W*, A, bool), void (*launch_step)(const W*, const A&, bool),
                        void (*launch_spmm_u)(const W*, A, bool), void (*launch_finalize)(const W*, const A&, int))
{
    hipStream_t s = w->v.stream;
    launch_t(w, a);
    launch_spmm(w, a, true);
    launch_step(w, a, true);
    launch_spmm_u(w, a, false);
    launch_finalize(w, a, 0);
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < kmax; k++) {
        launch_step(w, a, false);
        launch_spmm_u(w, a, false);
        launch_finalize(w, a, 0);
        if (k % kCheckEvery == 0 && k + 1 < kmax) {
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(w->h_ended, w->ended, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (*w->h_ended >= nrhs) break;  // later launches would be no-ops for every column
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The single-reduction CG with the unit's arguments a on the columns staged in
// the workspace's b and x. launch_step, launch_spmm_u: where the units differ.
template <class U>
int run_srcg(typename U::Workspace* w, const typename U::Args& a, int nrhs, int max_iter, double tol, int* niters,
             double* normr, double* wall,
             void (*launch_step)(const typename U::Workspace*, const typename U::Args&, bool),
             void (*launch_spmm_u)(const typename U::Workspace*, typename U::Args, bool))
{
    HIP_TRY(hipEventRecord(w->ev0, w->v.stream));
    launch_init<U>(w, a, max_iter, tol);
    TRY(run_srcg_recurrence(w, a, nrhs, max_iter, launch_srcg_t<U>, launch_spmm64<U>, launch_step, launch_spmm_u,
                            launch_srcg_finalize<U>));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

}  // namespace

}  // namespace hpccg
