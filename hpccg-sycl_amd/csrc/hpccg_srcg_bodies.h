// hpccg_srcg_bodies.h -- the device code of the single-reduction
// (Chronopoulos-Gear) form of the diagonally preconditioned CG
// (include/hpccg_hip_srcg.h), on top of hpccg_columns.h: one definition of
// every rounding-relevant expression of that recurrence, so that a unit over a
// rank group computes a member's rows as the one-rank unit (hpccg_srcg.hip)
// computes them.
//   device  SrcgArgs; the fused vector step (srcg_step: p, s, x, r, u and the
//           slice partials of r.u and r.r in one pass) and the finalize
//           (srcg_finalize: the three totals, then the column's scalars once).
//           A unit's __global__ entry points are thin wrappers.
// The recurrence keeps u = m r where the classic one keeps p: in the guarded
// column buffer ColArgs::p points to, which the SpMM reads at neighbour offsets
// (hpccg_spmm.h with a.p = u, a.Ap = w = A u, so u.w is the kDotPAP partial).
// The search direction p and s = A p are plain columns, updated by recurrence.
// ColState is used as it is: rtrans / oldrtrans hold gamma = r.u, pap holds
// delta = u.w, alpha is still the previous one when the new one is formed.
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include "hpccg_columns.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct SrcgArgs : ColArgs {
    // (ColArgs' p: u, a guard zone around each column; Ap: w; minv: the call's m)
    int tri;  // width 27: slices whose offsets come in runs of three use the x-triple plan
    const double* aval;
    const double* vals;
    double* pd;  // the search direction, column c at pd + c * vcs
    double* sd;  // s = A p by recurrence, column c at sd + c * vcs
};

// ---------------------------------------------------------------------------
// prologue: r = b + (-1)*w (w = A t, t = x + 0.0*x by col_p);  u = m*r
// loop:     p = u + beta*p (k == 1: u read for p, beta 0.0)
//           s = w + beta*s (k == 1: w read for s)
//           x = x + alpha*p;  r = r + (-alpha)*s;  u = m*r
// then the r.u slice partial (slot kDotRZ) and the r.r one, in col_update<kR,
// true>'s shapes and order, per running column. m is loaded once for the
// launch's columns; u is stored to the rows below n only (the guard zones and
// the padding stay zero).
// ---------------------------------------------------------------------------
template <int kR>
__device__ __forceinline__ void srcg_step(const SrcgArgs& a, bool prologue)
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
        double* __restrict__ rc = a.r + (size_t)c * a.rcs;
        double* __restrict__ uc = a.p + (size_t)c * a.pcs;
        const Rows wv = ld(a.Ap + (size_t)c * a.vcs + row);
        Rows rn;
        if (prologue) {
            const Rows bv = ld(a.b + (size_t)c * a.vcs + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) rn.v[i] = bv.v[i] + (-1.0) * wv.v[i];
        } else {
            const int k = a.st[c].k;
            const double alpha = a.st[c].alpha, beta = a.st[c].beta;
            const Rows uv = ld(uc + row);
            double* __restrict__ pc = a.pd + (size_t)c * a.vcs;
            double* __restrict__ sc = a.sd + (size_t)c * a.vcs;
            const Rows po = (k == 1) ? uv : ld(pc + row);
            const Rows so = (k == 1) ? wv : ld(sc + row);
            Rows pn, sn, xn;
#pragma unroll
            for (int i = 0; i < kRpt; i++) pn.v[i] = uv.v[i] + beta * po.v[i];
#pragma unroll
            for (int i = 0; i < kRpt; i++) sn.v[i] = wv.v[i] + beta * so.v[i];
            st_rows(pc, row, a.n, pn);
            st_rows(sc, row, a.n, sn);
            double* __restrict__ xc = a.x + (size_t)c * a.vcs;
            const Rows xv = ld(xc + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) xn.v[i] = xv.v[i] + alpha * pn.v[i];
            st_rows(xc, row, a.n, xn);
            const Rows rv = ld(rc + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) rn.v[i] = rv.v[i] + (-alpha) * sn.v[i];
        }
        st_rows(rc, row, a.n, rn);
        Rows un;
#pragma unroll
        for (int i = 0; i < kRpt; i++) un.v[i] = mv.v[i] * rn.v[i];
        st_rows(uc, row, a.n, un);
        rw_slice_partial(a, kDotRZ, s, row, c, rn, un);
        rr_slice_partial(a, s, row, c, rn);
    }
}

// The column's scalars once the three totals of iteration k are known (one
// lane): hist[k] = rr and advance_column's loop test on it, unchanged;
//   beta  = gamma / gamma_old                          (0.0 for k == 0)
//   alpha = gamma / (delta - (beta*gamma) / alpha_old) (gamma / delta for k == 0)
__device__ __forceinline__ void srcg_advance(const ColArgs& a, ColState* st, int c, double rr, double gamma,
                                             double delta)
{
    const int k = st->k;
    const double old = st->rtrans;  // gamma of iteration k - 1 (k >= 1)
    const double oldrr = st->rr;    // r_{k-1}.r_{k-1} (k >= 1)
    const double aold = st->alpha;
    a.hist[(size_t)c * a.hstride + k] = rr;
    st->oldrtrans = old;
    st->rtrans = gamma;
    st->rr = rr;
    st->pap = delta;
    const double beta = (k == 0) ? 0.0 : gamma / old;
    st->beta = beta;
    st->alpha = (k == 0) ? gamma / delta : gamma / (delta - (beta * gamma) / aold);
    st->k = k + 1;
    const bool run = k + 1 < st->max_iter && sqrt(k == 0 ? rr : oldrr) > st->tol;
    if (!run) {
        st->run = 0;
        st->niters = k;
        atomicAdd(a.ended, 1);
    }
}

// ---------------------------------------------------------------------------
// One block per column (kFinThreads threads): the totals of r.r, r.u and u.w
// from their slice partials (col_dot_total's shape), then the column's scalars.
// store_total: the three go to tot[kDotRR | kDotRZ | kDotPAP][c] instead and
// the state is left alone (a group member's parts of the iteration's one sum).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void srcg_finalize(const ColArgs& a, int store_total)
{
    __shared__ double gs[kFinLds];
    const int c = blockIdx.x;
    ColState* const st = a.st + c;
    if (!st->run) return;  // (block-uniform) a frozen column keeps its state
    const double rr = col_dot_total(a, kDotRR, c, gs);
    __syncthreads();  // the group sums in gs have been read
    const double gamma = col_dot_total(a, kDotRZ, c, gs);
    __syncthreads();
    const double delta = col_dot_total(a, kDotPAP, c, gs);
    if (threadIdx.x != 0) return;
    if (store_total) {
        a.tot[(size_t)kDotRR * a.cap + c] = rr;
        a.tot[(size_t)kDotRZ * a.cap + c] = gamma;
        a.tot[(size_t)kDotPAP * a.cap + c] = delta;
        return;
    }
    srcg_advance(a, st, c, rr, gamma, delta);
}

}  // namespace

}  // namespace hpccg
