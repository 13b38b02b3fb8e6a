#!/usr/bin/env python3
"""Mixed-precision CG (fp32 matrix image, include/hpccg_hip_mixed.h) against
its fp64 baseline on the same matrix and columns in one process (same
allocations, so the per-process placement spread does not enter).

Exact configurations (generated stencils: the fp32 image is the matrix). One
process per configuration; after a warm-up of each side the mixed solve and its
baseline alternate `--reps` times at max_iter 500, tolerance 0:
  nrhs 1   baseline hpccg_hip_solve_device, iterations per second
  nrhs 4   baseline hpccg_hip_batch_solve_device, RHS-iterations per second
Every run also checks that x, niters and the traces are bitwise the
baseline's; a mismatch ends the run with exit status 1. Reported: the rates
(median, min, max), their ratio and the byte model's prediction (bytes per row
per column per iteration: mixed 88 + 4 W / R, single solve 64 + 8 W, batch
88 + 8 W / R; W slots per row, R columns per SpMM launch).

Refined configuration (--refined N): 27-pt N^3 through from_csr with every
value scaled by a symmetric random factor s_i s_j in [0.5, 1.5), solved to 1e-10 ||b||
by the fp64 single solve and by the mixed solve: wall time, iterations, sweeps.

usage: tools/mixed_bench.py                      every configuration, one child process each
       tools/mixed_bench.py --one 27:200:1       one exact configuration (stencil:n:nrhs)
       tools/mixed_bench.py --refined 100        the refined configuration
       [--reps 5] [--out profiles/mixed/mixed_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_pkg  # noqa: E402

CONFIGS = ["27:200:1", "27:200:4", "27:100:1", "27:100:4", "7:256:1", "7:256:4"]
REFINED = 100


def model_ratio(width, nrhs):
    """Predicted mixed / baseline rate from the byte model."""
    mixed = 88 + 4 * width / nrhs
    base = 64 + 8 * width if nrhs == 1 else 88 + 8 * width / nrhs
    return base / mixed


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_exact(hp, torch, stencil, n, nrhs, reps, max_iter):
    dev = torch.device("cuda:0")
    M = hp.Matrix.generate(n, n, n, use_7pt=stencil == 7)
    rows = n ** 3
    try:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        B = torch.rand((nrhs, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        # column 0: the generated right-hand side (b = A 1, exact: bitwise the generator's)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), B[0])
        Xb = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)
        Xm = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)
        info = M.mixed_info()
        assert info["exact"] == 1, info
        base_tr, base_it = [None] * nrhs, [0] * nrhs

        def baseline():
            Xb.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if nrhs == 1:
                _, it, _, _ = hp.HPCCG(M, B[0], Xb[0], max_iter=max_iter, tolerance=0.0, device=True)
                dt = time.perf_counter() - t0
                base_it[0], base_tr[0] = it, M.last_trace().tobytes()
            else:
                _, its, _, _ = hp.HPCCG_batch(M, B, Xb, max_iter=max_iter, tolerance=0.0, device=True)
                dt = time.perf_counter() - t0
                for c in range(nrhs):
                    base_it[c], base_tr[c] = int(its[c]), M.last_trace_batch(c).tobytes()
            return sum(base_it) / dt

        def mixed():
            Xm.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, its, _, _ = hp.HPCCG_mixed(M, B, Xm, max_iter=max_iter, tolerance=0.0, device=True)
            return int(its.sum()) / (time.perf_counter() - t0), its

        baseline()  # warm-up of both paths (graph capture, workspaces)
        mixed()
        rb, rm = [], []
        same = True
        for _ in range(reps):
            rb.append(baseline())
            r, its = mixed()
            rm.append(r)
            same = same and all(int(its[c]) == base_it[c] and M.last_trace_mixed(c).tobytes() == base_tr[c]
                                for c in range(nrhs)) and bool(torch.equal(Xm, Xb))
        width = int(M.get_option("a_width")) or stencil
        unit = "it_per_s" if nrhs == 1 else "rhs_it_per_s"
        return {"kind": "exact", "stencil": stencil, "n": n, "rows": rows, "nrhs": nrhs, "max_iter": max_iter,
                "reps": reps, "iters_per_column": base_it[0], "unit": unit,
                "baseline": "hpccg_hip_solve_device" if nrhs == 1 else "hpccg_hip_batch_solve_device",
                "mixed": summary(rm), "fp64": summary(rb),
                "ratio_of_medians": statistics.median(rm) / statistics.median(rb),
                "model_ratio": model_ratio(width, nrhs), "slots_per_row": width,
                "image_bytes": info["image_bytes"], "bitwise_equal": same}
    finally:
        M.close()


def run_refined(hp, torch, n, reps):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    dev = torch.device("cuda:0")
    G = oracle.generate(n, n, n)
    rows = G.nrow
    # a congruence S A S with S = diag(s), s_i in [sqrt(0.5), sqrt(1.5)): entry (i, j) is scaled by s_i s_j in
    # [0.5, 1.5) and the matrix stays positive definite at any size (an independent factor per pair does not
    # keep it so at 100^3: the fp64 solve itself stalls at 3e-4 ||b|| after 3999 iterations)
    s = np.random.default_rng(31).uniform(0.5 ** 0.5, 1.5 ** 0.5, rows)
    vals = G.vals * s[np.repeat(np.arange(rows, dtype=np.int64), np.diff(G.row_ptr))] * s[G.cols]
    M = hp.Matrix.from_csr(G.row_ptr, G.cols, vals)
    try:
        ones = torch.ones(rows, dtype=torch.float64, device=dev)
        b = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPC_sparsemv(M, ones, b)
        bnorm = float(torch.linalg.vector_norm(b))
        tol = 1e-10 * bnorm
        info = M.mixed_info()
        assert info["exact"] == 0, info
        x64 = torch.zeros_like(b)
        xm = torch.zeros_like(b)
        res = torch.zeros_like(b)

        def true_residual(x):
            hp.HPC_sparsemv(M, x, res)
            return float(torch.linalg.vector_norm(b - res)) / bnorm

        def fp64():
            x64.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, it, nr, _ = hp.HPCCG(M, b, x64, max_iter=4000, tolerance=tol, device=True)
            return time.perf_counter() - t0, it, nr

        def mixed():
            xm.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, its, nrs, _ = hp.HPCCG_mixed(M, b, xm, max_iter=4000, tolerance=tol, device=True)
            return time.perf_counter() - t0, int(its[0]), float(nrs[0])

        fp64()
        mixed()
        t64, tm = [], []
        for _ in range(reps):
            t, it64, nr64 = fp64()
            t64.append(t)
            t, itm, nrm = mixed()
            tm.append(t)
        sweeps, resid = M.last_sweeps_mixed(0)
        return {"kind": "refined", "stencil": 27, "n": n, "rows": rows, "reps": reps, "tolerance_rel": 1e-10,
                "slots_per_row": int(M.get_option("a_width")), "inexact_values": info["inexact_values"],
                "fp64": {"wall_s": summary(t64), "niters": it64, "normr_rel": nr64 / bnorm,
                         "true_residual_rel": true_residual(x64)},
                "mixed": {"wall_s": summary(tm), "niters": itm, "normr_rel": nrm / bnorm,
                          "true_residual_rel": true_residual(xm), "sweep_iters": [int(v) for v in sweeps],
                          "sweep_residuals_rel": [float(v) / bnorm for v in resid]},
                "wall_ratio_fp64_over_mixed": statistics.median(t64) / statistics.median(tm)}
    finally:
        M.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", help="stencil:n:nrhs, one exact configuration in this process")
    ap.add_argument("--refined", type=int, help="n: the refined configuration in this process")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed", "mixed_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5 alternations")
    if args.one or args.refined:
        import torch
        hp = load_pkg()
        hp.set_device(0)
        if args.one:
            st, n, nrhs = (int(v) for v in args.one.split(":"))
            rec = run_exact(hp, torch, st, n, nrhs, args.reps, args.max_iter)
        else:
            rec = run_refined(hp, torch, args.refined, args.reps)
        rec["device"] = hp.device_name()[0]
        print(json.dumps(rec), flush=True)
        return 0 if rec.get("bitwise_equal", True) else 1
    # one child process per configuration, one after the other; the first failure ends the run
    recs, rc = [], 0
    jobs = [["--one", c] for c in args.configs.split(",") if c] + [["--refined", str(REFINED)]]
    for job in jobs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--max-iter",
                                str(args.max_iter)] + job, capture_output=True, text=True, timeout=args.child_timeout)
        except subprocess.TimeoutExpired:
            print(f"TIMED OUT: {' '.join(job)}", file=sys.stderr)
            rc = 1
            break
        sys.stderr.write(p.stderr[-2000:])
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if lines:
            print(lines[-1], flush=True)
            recs.append(json.loads(lines[-1]))
        if p.returncode != 0:
            print(f"FAILED ({p.returncode}): {' '.join(job)}", file=sys.stderr)
            rc = 1
            break
    doc = {"device": recs[0]["device"] if recs else None, "results": recs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
