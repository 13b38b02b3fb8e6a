#!/usr/bin/env python3
"""Diagonally preconditioned CG (hpccg_hip_pcg_solve_device): what the
preconditioner costs per iteration, and what it buys in time to solution. One
matrix per size in one process (same allocations, so the per-process placement
spread does not enter).

1. Per-iteration cost. Per size and column count, HPCCG_pcg with Jacobi and
   HPCCG_batch on the same device columns, both max_iter 500 at tolerance 0;
   after a warm-up of each, the two alternate `--reps` times. Reported:
   RHS-iterations per second (median, min, max), their ratio, and the byte
   model's ratio (bytes per row, column and iteration, 88 +
   (8 W + 16) / R for the preconditioned recurrence against the batch's 88 +
   8 W / R -- one column: the single solve's 64 + 8 W, which the batch forwards
   to; W slots per row, R columns per launch). Before the timing the
   preconditioned solve with m = 1 is compared bitwise with the batch (x,
   niters, traces); a mismatch ends the run with exit status 1.

2. Time to solution. The 27-point n^3 stencil (--scaled-n, default 100) with
   every entry a_ij s_i s_j, s_i = 2^e_i, e_i random in [-6, 6], b = A 1:
   iterations and wall time until normr <= 1e-10 normr_0 for Jacobi and for the
   plain solve (capped at --plain-cap iterations), median of `--reps` runs.

usage: tools/pcg_bench.py [--sizes 27:200,27:100,7:256] [--nrhs 1,4] [--reps 5]
                          [--scaled-n 100] [--out profiles/pcg/pcg_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from bench import load_pkg  # noqa: E402

MAX_R = 4  # columns per launch (the widest instantiation)


def model_ratio(width, nrhs):
    """Predicted preconditioned / batch rate from the byte model."""
    if nrhs == 1:
        return (64 + 8 * width) / (88 + 8 * width + 16)
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    per_col = launches / nrhs  # matrix (and m) passes per column and iteration
    return (88 + 8 * width * per_col) / (88 + (8 * width + 16) * per_col)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_size(hp, torch, stencil, n, nrhs_list, reps, max_iter):
    dev = torch.device("cuda:0")
    M = hp.Matrix.generate(n, n, n, use_7pt=stencil == 7)
    rows = n ** 3
    out = []
    try:
        kmax = max(nrhs_list)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        B = torch.rand((kmax, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), B[0])  # column 0: b = A 1
        ones = torch.ones(rows, dtype=torch.float64, device=dev)
        for nrhs in nrhs_list:
            Xp = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)
            Xb = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)

            def batch():
                Xb.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, its, _, _ = hp.HPCCG_batch(M, B[:nrhs], Xb, max_iter=max_iter, tolerance=0.0, device=True)
                return int(its.sum()) / (time.perf_counter() - t0), its

            def pcg(minv=None):
                Xp.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, its, _, _ = hp.HPCCG_pcg(M, B[:nrhs], Xp, max_iter=max_iter, tolerance=0.0, minv=minv, device=True)
                return int(its.sum()) / (time.perf_counter() - t0), its

            # warm-up of both paths, and the bitwise check: m = 1 is the batch
            _, itb = batch()
            trb = [M.last_trace_batch(c).tobytes() for c in range(nrhs)]
            _, itp = pcg(ones)
            same = all(int(itp[c]) == int(itb[c]) and M.last_trace_pcg(c).tobytes() == trb[c]
                       for c in range(nrhs)) and bool(torch.equal(Xp, Xb))
            pcg()
            rp, rb = [], []
            for _ in range(reps):
                rb.append(batch()[0])
                r, its = pcg()
                rp.append(r)
            width = int(M.get_option("a_width")) or stencil
            rec = {"stencil": stencil, "n": n, "rows": rows, "nrhs": nrhs, "max_iter": max_iter, "reps": reps,
                   "iters_per_column": int(its[0]),
                   "pcg_rhs_it_per_s": summary(rp), "batch_rhs_it_per_s": summary(rb),
                   "ratio_of_medians": statistics.median(rp) / statistics.median(rb),
                   "model_ratio": model_ratio(width, nrhs), "slots_per_row": width,
                   "unit_m_bitwise_equal_to_batch": same}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            M.batch_release()
            M.pcg_release()
    finally:
        M.close()
    return out


def run_scaled(hp, torch, n, reps, plain_cap):
    import numpy as np
    import oracle
    dev = torch.device("cuda:0")
    A = oracle.generate(n, n, n)
    rows = A.nrow
    s = 2.0 ** np.random.default_rng(77).integers(-6, 7, rows)
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(A.row_ptr))
    vals = (A.vals * s[r]) * s[A.cols.astype(np.int64)]
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, vals)
    del r, vals
    try:
        b = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), b)
        x = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPCCG(M, b, x, max_iter=1, device=True)
        r0 = float(M.last_trace()[0])
        tol = 1e-10 * r0

        def jacobi():
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, its, nrs, _ = hp.HPCCG_pcg(M, b, x, max_iter=plain_cap, tolerance=tol, device=True)
            return time.perf_counter() - t0, int(its[0]), float(nrs[0])

        def plain():
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, it, nr, _ = hp.HPCCG(M, b, x, max_iter=plain_cap, tolerance=tol, device=True)
            return time.perf_counter() - t0, it, nr

        jacobi()
        plain()
        tj, tp = [], []
        for _ in range(reps):
            t, itj, nrj = jacobi()
            tj.append(t)
            err = float((x - 1.0).abs().max())
            t, itp, nrp = plain()
            tp.append(t)
        rec = {"stencil": 27, "n": n, "rows": rows, "scale": "s_i = 2^e_i, e_i in [-6, 6]", "normr0": r0,
               "tolerance": tol, "reps": reps, "a_width": int(M.get_option("a_width")),
               "jacobi": {"niters": itj, "normr_over_normr0": nrj / r0, "reached": nrj <= tol, "seconds": summary(tj),
                          "max_abs_x_minus_xexact": err},
               "plain": {"niters": itp, "cap": plain_cap, "normr_over_normr0": nrp / r0, "reached": nrp <= tol,
                         "seconds": summary(tp)}}
        print(json.dumps(rec), flush=True)
        return rec
    finally:
        M.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="27:200,27:100,7:256", help="stencil:n, comma separated (empty: none)")
    ap.add_argument("--nrhs", default="1,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--scaled-n", type=int, default=100, help="0: no time-to-solution run")
    ap.add_argument("--plain-cap", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg", "pcg_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5 alternations")
    import torch
    hp = load_pkg()
    hp.set_device(0)
    recs = []
    for sz in [v for v in args.sizes.split(",") if v]:
        st, n = (int(v) for v in sz.split(":"))
        recs += run_size(hp, torch, st, n, [int(v) for v in args.nrhs.split(",")], args.reps, args.max_iter)
    doc = {"device": hp.device_name()[0], "per_iteration": recs}
    if args.scaled_n > 0:
        doc["time_to_solution"] = run_scaled(hp, torch, args.scaled_n, args.reps, args.plain_cap)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in recs if not r["unit_m_bitwise_equal_to_batch"]]
    for r in bad:
        print(f"MISMATCH: {r['stencil']}-pt {r['n']}^3 nrhs {r['nrhs']}: the preconditioned solve with m = 1 is not "
              "bitwise the batch", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
