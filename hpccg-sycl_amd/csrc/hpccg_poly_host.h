// hpccg_poly_host.h -- the host code of the Chebyshev polynomial preconditioned
// CG, shared by the polynomial units (hpccg_poly.hip, hpccg_poly32.hip and,
// under hpccg_poly_group_host.h, hpccg_poly_group.hip and
// hpccg_poly32_group.hip): the workspace's polynomial state, the kernel
// arguments, the launchers with the degree in them, the checks of a caller's
// bounds and the interval with its coefficients; for the one-rank units (poly,
// poly32) also the Gershgorin bound, the per-call setup and the recurrence that
// hpccg_onerank_host.h's solve runs, and the bodies of their bound and
// last_spectrum exports. What is not polynomial -- the dispatch on a chunk's
// columns and fp64 SpMM form, the init, SpMM and finalize launchers, the matrix
// check, the preconditioner, the solve, the bookkeeping exports -- is
// hpccg_onerank_host.h.
// The single-reduction units (hpccg_srpoly.hip, hpccg_srpoly_group.hip) run the
// solve bodies here and in hpccg_poly_group_host.h with vectors of their own
// (p and s) and their own recurrence (hpccg_srcg_host.h,
// hpccg_srcg_group_host.h) in the bodies' slots.
// A unit hands over one traits struct U: what hpccg_onerank_host.h asks for
// (Args a PolyArgs, Workspace a PolyWorkspace) and
//   row0(w)               local row 0 inside a guarded column: the guard rows
//                         (one rank) or the member's p0 (group)
//   p<kR, kPre>, update<kR, kCheb>   its kernels, as templates of kernel
//                         pointers; with step<kW, kR, kWaves>, step_sell<kR>
//                         where it runs the fp64 steps
// and a one-rank unit further
//   q, bound, bound_top   the bound's kernels
//   launch_spmm(w, a, prologue), launch_step(w, a)   where poly32 differs: the
//                         SpMM and one step over the chunks of columns
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include <algorithm>
#include <cmath>

#include "hpccg_onerank_host.h"
#include "hpccg_poly_bodies.h"
#include "hpccg_poly_coeffs.h"

namespace hpccg {

namespace {

// A polynomial unit's workspace (a group member's adds GroupMember).
struct PolyWorkspace : TraceWorkspace, JacobiCache {
    double *r = nullptr, *x = nullptr, *b = nullptr;
    double *dd = nullptr, *zbuf = nullptr;  // zbuf: two sets of cap columns in p's (guarded) layout
    // the bound's vectors (kept while the columns grow, counted in rest_bytes);
    // qbuf: one guarded column
    double *qbuf = nullptr, *smax = nullptr, *lmax_dev = nullptr;
    bool jac_lmax_built = false;
    double jac_lmax = 0.0;  // the bound with m = 1 / a_ii (a member: its rows' part)
    // the call being run
    int degree = 0;
    double cheb0 = 0.0, aj[kPolyMaxDegree + 1] = {}, bj[kPolyMaxDegree + 1] = {};
    bool solved = false;  // (a group: member 0)
    double last_lmin = 0.0, last_lmax = 0.0;

    PolyWorkspace() { ndots = 3; }

    void free_own_vectors()
    {
        for (double* q : {r, x, b, dd, zbuf})
            if (q) (void)hipFree(q);
        r = x = b = dd = zbuf = nullptr;
    }
    void free_bound_vectors()
    {
        for (double* q : {qbuf, smax, lmax_dev})
            if (q) (void)hipFree(q);
        qbuf = smax = lmax_dev = nullptr;
    }
    void free_own_rest()
    {
        free_bound_vectors();
        free_cache();
    }
    long long total_bytes() const { return bytes + rest_bytes; }
};

// z buffer `which` (0, 1): local row 0 of column 0
template <class U>
double* z_of(const typename U::Workspace* w, int which)
{
    return w->zbuf + (size_t)which * (size_t)w->pcs * (size_t)w->cap + U::row0(w);
}

// (what a unit's Args add to PolyArgs is set where its launchers use it)
template <class U>
typename U::Args make_args(const typename U::Workspace* w, int nrhs, const double* m)
{
    const MatrixView& v = w->v;
    typename U::Args a{};
    fill_args(&a, w, nrhs);
    a.tri = 1;
    a.p = w->pbuf + U::row0(w);
    a.r = w->r;
    a.rcs = w->vcs;
    a.x = w->x;
    a.b = w->b;
    a.minv = m;
    a.aval = v.aval;
    a.vals = v.vals;
    a.dd = w->dd;
    a.cheb0 = w->cheb0;
    return a;
}

// d == 0: z = m r in the register; else the last step's z (buffer d & 1, the
// unit's own rows only) in r's place.
template <class U>
void launch_p(const typename U::Workspace* w, typename U::Args a, bool prologue)
{
    const int d = w->degree;
    if (d > 0) {
        a.r = z_of<U>(w, d & 1);
        a.rcs = a.pcs;
    }
    launch_chunks(w, a, prologue, [d](auto r) {
        return d > 0 ? U::template p<decltype(r)::value, false> : U::template p<decltype(r)::value, true>;
    });
}

// The update with step 0 into z buffer 0 where d >= 1 (d == 0: the engine's kPre update).
template <class U>
void launch_update0(const typename U::Workspace* w, typename U::Args a, bool prologue)
{
    const int d = w->degree;
    a.zout = z_of<U>(w, 0);
    launch_chunks(w, a, prologue, [d](auto r) {
        return d > 0 ? U::template update<decltype(r)::value, true> : U::template update<decltype(r)::value, false>;
    });
}

// Step j's buffers and scalars: it reads z buffer (j - 1) & 1 and stores buffer j & 1.
template <class U>
typename U::Args step_args(const typename U::Workspace* w, typename U::Args a, int j)
{
    a.zin = z_of<U>(w, (j - 1) & 1);
    a.zout = z_of<U>(w, j & 1);
    a.aj = w->aj[j];
    a.bj = w->bj[j];
    a.last = j == w->degree;
    return a;
}

// One step's launches from the fp64 image: the SpMM's forms.
template <class U>
void launch_step64(const typename U::Workspace* w, typename U::Args a)
{
    const dim3 g(a.grid), b(kBlock);
    hipStream_t s = w->v.stream;
    for_chunks(a.nrhs, true, [&](int c0, int R) {
        a.c0 = c0;
        if (!w->v.has_a)
            with_columns(R, [&](auto r) {
                hipLaunchKernelGGL((U::template step_sell<decltype(r)::value>), g, b, 0, s, a);
            });
        else
            with_spmm_form(a, R, [&](auto wd, auto r, auto wv) {
                hipLaunchKernelGGL((U::template step<decltype(wd)::value, decltype(r)::value, decltype(wv)::value>), g,
                                   b, 0, s, a);
            });
    });
}

// A caller's bounds: each finite and >= 0 (0.0: the default); both given, lmin < lmax.
int check_bounds(const char* who, double lmin, double lmax)
{
    if (!(std::isfinite(lmin) && std::isfinite(lmax) && lmin >= 0.0 && lmax >= 0.0))
        return fail(HPCCG_HIP_EINVAL, "%s: spectrum bounds lmin %g, lmax %g (finite and >= 0 needed; 0: the default)",
                    who, lmin, lmax);
    if (lmax > 0.0 && lmin >= lmax)
        return fail(HPCCG_HIP_EINVAL, "%s: spectrum bounds lmin %g >= lmax %g", who, lmin, lmax);
    return 0;
}

// A caller's degree and bounds: what a solve checks before it looks at a matrix.
int check_polynomial(const char* who, int degree, double lmin, double lmax)
{
    if (degree < 0 || degree > kPolyMaxDegree)
        return fail(HPCCG_HIP_EINVAL, "%s: degree %d (0 to %d)", who, degree, kPolyMaxDegree);
    return check_bounds(who, lmin, lmax);
}

// The interval of a call and the polynomial's coefficients on it. *lmax == 0.0:
// bound(lmax), the unit's Gershgorin bound; *lmin == 0.0: lmax / kPolyEigRatio.
// Degree 0 applies no polynomial and needs no interval (what the caller gave is
// kept for last_spectrum).
template <class Bound>
int resolve_interval(const char* who, int degree, double* lmin, double* lmax, double* cheb0, double* aj, double* bj,
                     Bound bound)
{
    if (degree > 0) {
        if (*lmax == 0.0) TRY(bound(lmax));
        if (*lmin == 0.0) *lmin = *lmax / kPolyEigRatio;
        if (!(*lmin > 0.0 && *lmin < *lmax))
            return fail(HPCCG_HIP_EINVAL, "%s: spectrum bounds lmin %g >= lmax %g", who, *lmin, *lmax);
        poly_coefficients(*lmin, *lmax, degree, cheb0, aj, bj);
    } else if (*lmin == 0.0 && *lmax > 0.0) {
        *lmin = *lmax / kPolyEigRatio;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// The one-rank units (poly, poly32)
// ---------------------------------------------------------------------------
// The bound's vectors (zeroed: q's guard zones and its rows past n are read and
// never stored; a member's ghost planes by the halo only). pcs: the guarded column.
int ensure_bound_vectors(PolyWorkspace* w, long long pcs)
{
    if (w->qbuf) return 0;
    HIP_TRY(hipSetDevice(w->v.device));
    const long long before = w->bytes;  // (alloc_zero counts into bytes: the columns')
    int rc = alloc_zero(w, &w->qbuf, (size_t)pcs);
    if (!rc) rc = alloc_zero(w, &w->smax, (size_t)std::max(w->v.nslices, 1));
    if (!rc) rc = alloc_zero(w, &w->lmax_dev, 1);
    if (rc)
        w->free_bound_vectors();
    else
        w->rest_bytes += w->bytes - before;
    w->bytes = before;
    return rc;
}

// The symmetric Gershgorin bound with the padded device vector m (always over
// the fp64 image).
template <class U>
int compute_bound(typename U::Workspace* w, const double* m, double* lmax)
{
    const MatrixView& v = w->v;
    hipStream_t s = v.stream;
    TRY(ensure_bound_vectors(w, p_column(v)));
    double* q = w->qbuf + v.guard_rows;
    hipLaunchKernelGGL(U::q, dim3((v.n + 255) / 256), dim3(256), 0, s, m, v.n, q);
    hipLaunchKernelGGL(U::bound, dim3(v.nslices), dim3(kBlock), 0, s, diag_args(v), (const double*)q, w->smax);
    hipLaunchKernelGGL(U::bound_top, dim3(1), dim3(kBlock), 0, s, (const double*)w->smax, v.nslices, w->lmax_dev);
    HIP_TRY(hipGetLastError());
    double h = 0.0;
    HIP_TRY(hipMemcpyAsync(&h, w->lmax_dev, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!(h > 0.0 && std::isfinite(h)))
        return fail(HPCCG_HIP_EINVAL, "%s: the Gershgorin bound of the matrix is %g (finite and > 0 needed)", U::who, h);
    *lmax = h;
    return 0;
}

// Jacobi's bound: cached with 1 / a_ii.
template <class U>
int jacobi_bound(typename U::Workspace* w, double* lmax)
{
    if (!w->jac_lmax_built) {
        TRY(compute_bound<U>(w, w->jac, &w->jac_lmax));
        w->jac_lmax_built = true;
    }
    *lmax = w->jac_lmax;
    return 0;
}

// Room for ncols columns of the guarded width pcs and a history of max_iter + 1
// entries per column; ntot: totals per column (a group member's). more(cap):
// allocates what a unit's workspace W adds to the polynomial's vectors (the
// single-reduction units: p and s, hpccg_srcg_host.h), last.
template <class W, class More>
int ensure_vectors(W* w, int ncols, int max_iter, long long pcs, int ntot, More more)
{
    const size_t npad = (size_t)w->v.npad;
    return ensure_columns(w, ncols, max_iter, true, pcs, ntot, [&](int cap) {
        TRY(alloc_zero(w, &w->r, npad * cap));
        TRY(alloc_zero(w, &w->x, npad * cap));
        TRY(alloc_zero(w, &w->b, npad * cap));
        TRY(alloc_zero(w, &w->dd, npad * cap));
        // zeroed: z's guard zones and the rows past n are read and never stored
        // (a member's ghost planes by the halo only)
        TRY(alloc_zero(w, &w->zbuf, 2 * (size_t)pcs * cap));
        return more(cap);
    });
}

// The update with step 0, then steps 1 .. d: z_d ends in buffer d & 1.
template <class U>
void launch_update(const typename U::Workspace* w, typename U::Args a, bool prologue)
{
    launch_update0<U>(w, a, prologue);
    for (int j = 1; j <= w->degree; j++) U::launch_step(w, step_args<U>(w, a, j));
}

// The preconditioned CG on the columns staged in the workspace's b and x.
template <class U>
int run_cg(typename U::Workspace* w, int nrhs, const double* m, int max_iter, double tol, int* niters, double* normr,
           double* wall)
{
    const typename U::Args a = make_args<U>(w, nrhs, m);
    HIP_TRY(hipEventRecord(w->ev0, w->v.stream));
    launch_init<U>(w, a, max_iter, tol);
    TRY(run_recurrence(w, a, nrhs, max_iter, launch_p<U>, U::launch_spmm, launch_update<U>, launch_finalize<U>));
    return finish_recurrence(w, nrhs, niters, normr, wall);
}

// The solve: hpccg_onerank_host.h's, with the degree and the bounds checked
// before the matrix and the interval resolved once m is in hand. prepare (may
// be null): poly32's image. more(w, cap) (may be null): allocates what the
// unit's workspace adds to the polynomial's vectors; run: its recurrence.
template <class U>
int solve_common(hpccg_hip_matrix* M, int nrhs, const double* B, long long ldb, double* X, long long ldx,
                 const double* minv, int degree, double lmin, double lmax, int max_iter, double tol, int* niters,
                 double* normr, double* times, bool host, int (*prepare)(typename U::Workspace*) = nullptr,
                 int (*more)(typename U::Workspace*, int cap) = nullptr,
                 int (*run)(typename U::Workspace*, int, const double*, int, double, int*, double*, double*) = run_cg<U>)
{
    using W = typename U::Workspace;
    const char* who = U::who;
    return solve_onerank<U>(
        M, nrhs, B, ldb, X, ldx, minv, max_iter, tol, niters, normr, times, host,
        [&] { return check_polynomial(who, degree, lmin, lmax); },
        prepare,
        [&](W* w, const double* m, int kmax) -> int {
            TRY(resolve_interval(who, degree, &lmin, &lmax, &w->cheb0, w->aj, w->bj, [&](double* top) {
                return minv ? compute_bound<U>(w, m, top) : jacobi_bound<U>(w, top);
            }));
            TRY(ensure_vectors(w, nrhs, kmax, p_column(w->v), 0, [&](int cap) { return more ? more(w, cap) : 0; }));
            w->degree = degree;
            w->last_lmin = lmin;
            w->last_lmax = lmax;
            w->solved = true;
            return 0;
        },
        run);
}

// The bodies of a one-rank unit's bound and last_spectrum exports.
template <class U>
int poly_bound(hpccg_hip_matrix* M, const double* minv_dev, double* lmax)
{
    using W = typename U::Workspace;
    if (!M || !lmax) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    MatrixView v;
    TRY(check_matrix(U::who, M, &v));
    if (v.n == 0) {
        *lmax = 0.0;
        return 0;
    }
    return keep_device([&]() -> int {
        W* w = nullptr;
        TRY(g_ws<W>.record(M, v, &w));
        TRY(ensure_cache(w));
        if (minv_dev) {
            TRY(stage_minv<U>(w, minv_dev, false));
            return compute_bound<U>(w, w->muser, lmax);
        }
        TRY(ensure_jacobi<U>(w));
        return jacobi_bound<U>(w, lmax);
    });
}

template <class U>
int poly_last_spectrum(const hpccg_hip_matrix* M, double* lmin, double* lmax)
{
    if (!M || !lmin || !lmax) return fail(HPCCG_HIP_EINVAL, "%s: NULL argument", U::who);
    const typename U::Workspace* w = g_ws<typename U::Workspace>.find(M);
    if (!w || !w->solved)
        return fail(HPCCG_HIP_EINVAL, "%s: no spectrum (no %s solve ran on the matrix)", U::who, U::solve_name);
    *lmin = w->last_lmin;
    *lmax = w->last_lmax;
    return 0;
}

}  // namespace

}  // namespace hpccg
