// hpccg_srpoly_bodies.h -- the device code of the single-reduction
// (Chronopoulos-Gear) CG with the Chebyshev polynomial preconditioner
// (include/hpccg_hip_srpoly.h), on top of hpccg_srcg_bodies.h and
// hpccg_poly_bodies.h: one definition of the one rounding-relevant body neither
// of them has, so that a unit over a rank group computes a member's rows as the
// one-rank unit (hpccg_srpoly.hip) computes them.
//   device  SrpolyArgs; the fused vector step (srpoly_step: srcg_step's p, s, x
//           and r, then poly_update0's step 0 and the r.r slice partial on the
//           new r, in one pass). A unit's __global__ entry points are thin
//           wrappers.
// The recurrence is hpccg_srcg_bodies.h's with u = P(r) in place of u = m r: u
// is the last Chebyshev step's z (buffer degree & 1 of the polynomial's two, p's
// guarded column layout), which the SpMM reads at neighbour offsets
// (hpccg_spmm.h with a.p = u, a.Ap = w = A u, so u.w is the kDotPAP partial).
// The r.u slice partial is the last step's (PolyStep, slot kDotRZ); the three
// totals are completed by srcg_finalize, unchanged. Degree 0 is srcg_step
// itself on the arguments' SrcgArgs view (srcg_view).
// Internal linkage (each unit compiles its own copy), like hpccg_columns.h.
#pragma once
#include "hpccg_poly_bodies.h"
#include "hpccg_srcg_bodies.h"

#pragma clang fp contract(off)

namespace hpccg {

namespace {

struct SrpolyArgs : PolyArgs {
    // (PolyArgs' zout: step 0's z, buffer 0; Ap: w = A u)
    const double* u;  // the last step's z of the previous iteration, column c at u + c * pcs
    double* pd;       // the search direction, column c at pd + c * vcs
    double* sd;       // s = A p by recurrence, column c at sd + c * vcs
};

// The arguments as srcg_step takes them (degree 0: u = m r lives in p's buffer).
__device__ __forceinline__ SrcgArgs srcg_view(const SrpolyArgs& a)
{
    SrcgArgs s;
    static_cast<ColArgs&>(s) = a;
    s.tri = a.tri;
    s.aval = a.aval;
    s.vals = a.vals;
    s.pd = a.pd;
    s.sd = a.sd;
    return s;
}

// ---------------------------------------------------------------------------
// prologue: r = b + (-1)*w (w = A t, t = x + 0.0*x by col_p)
// loop:     p = u + beta*p (k == 1: u read for p, beta 0.0)
//           s = w + beta*s (k == 1: w read for s)
//           x = x + alpha*p;  r = r + (-alpha)*s
// (srcg_step's statements in its order), then step 0 of P on the new r in the
// same pass (poly_update0's):  t = m*r;  dd = c0*t;  z = dd  -> z buffer 0
// and the r.r slice partial, per running column. The r.u slice partial is the
// last step's. m is loaded once for the launch's columns.
// u is z buffer d & 1: for an even d the buffer step 0 stores. A thread loads
// its two rows of u before it stores them, and no other thread of the launch
// reads them (u and zout carry no __restrict__ for that).
// 13 streams per thread and column (u, w, p, s, x, r in; p, s, x, r, dd, z out;
// m once): 8 + 104 kR bytes per row.
// ---------------------------------------------------------------------------
template <int kR>
__device__ __forceinline__ void srpoly_step(const SrpolyArgs& a, bool prologue)
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
        const Rows wv = ld(a.Ap + (size_t)c * a.vcs + row);
        Rows rn;
        if (prologue) {
            const Rows bv = ld(a.b + (size_t)c * a.vcs + row);
#pragma unroll
            for (int i = 0; i < kRpt; i++) rn.v[i] = bv.v[i] + (-1.0) * wv.v[i];
        } else {
            const int k = a.st[c].k;
            const double alpha = a.st[c].alpha, beta = a.st[c].beta;
            const Rows uv = ld(a.u + (size_t)c * a.pcs + row);
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
        Rows dn;
#pragma unroll
        for (int i = 0; i < kRpt; i++) {
            const double t = mv.v[i] * rn.v[i];
            dn.v[i] = a.cheb0 * t;
        }
        st_rows(a.dd + (size_t)c * a.vcs, row, a.n, dn);
        st_rows(a.zout + (size_t)c * a.pcs, row, a.n, dn);
        rr_slice_partial(a, s, row, c, rn);
    }
}

}  // namespace

}  // namespace hpccg
