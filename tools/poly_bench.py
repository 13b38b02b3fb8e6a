#!/usr/bin/env python3
"""Chebyshev polynomial preconditioned CG (hpccg_hip_poly_solve_device): what a
degree costs per iteration, and what it buys in time to solution. The driver
starts one child process per configuration and visits the configurations in
turn, `--rounds` times (so a configuration's processes are spread over the
run); inside a process the solvers alternate `--reps` times after a warm-up of
each. Reported per configuration and solver: the median with min and max over
every repetition of every process, and the raw records.

1. Per-iteration cost (configuration: stencil, size, columns). HPCCG_pcg with
   Jacobi and HPCCG_poly at degrees 0 to 4 on the same device columns, max_iter
   `--max-iter` at tolerance 0; microseconds per iteration from the solve's
   device events. Degree 0 must be even with HPCCG_pcg, and is compared with it
   bitwise (x, niters, traces) before the timing; a mismatch ends the run with
   exit status 1. Beside the measured cost of a degree (the difference to
   degree 0, per degree) stands the byte model of one step: the matrix slots,
   8 W bytes per row, once per launch of R columns, plus 48 bytes of vectors
   per row and column (z in, r, dd in; dd and z out; the neighbours' z from
   cache) and 8 / R of m.

2. Time to solution (configuration: plain or "p2" scaling). The 27-point n^3
   pattern (--lap-n, default 100) with every diagonal entry 26.0 (weakly
   diagonally dominant), plain and with every entry a_ij s_i s_j, s_i = 2^e_i,
   e_i random in [-6, 6]; b = A 1. Iterations and wall time until
   normr <= 1e-10 normr_0 for Jacobi PCG, for degrees 1 to 4 at the default
   eigenvalue ratio 30, and for degree 3 at ratios 10 and 100. Every run's
   final x is checked against xexact = 1 (the record keeps the error).

usage: tools/poly_bench.py [--sizes 27:200,27:100,7:256] [--nrhs 1,4] [--reps 3] [--rounds 2]
                           [--lap-n 100] [--out profiles/poly/poly_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from bench import load_pkg  # noqa: E402

DEGREES = (0, 1, 2, 3, 4)
MAX_R = 4  # columns per launch (the widest instantiation)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "count": len(v)}


def step_model_bytes_per_row(width, nrhs):
    """Bytes per row one step moves for all nrhs columns (the docstring's model)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    return launches * (8 * width + 8) + 48 * nrhs


# ---------------------------------------------------------------------------
# children
# ---------------------------------------------------------------------------
def child_per_iteration(args):
    import torch
    hp = load_pkg()
    hp.set_device(0)
    dev = torch.device("cuda:0")
    n, nrhs, max_iter = args.n, args.child_nrhs, args.max_iter
    M = hp.Matrix.generate(n, n, n, use_7pt=args.stencil == 7)
    rows = n ** 3
    try:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        B = torch.rand((nrhs, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), B[0])  # column 0: b = A 1
        X = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)

        def run(solver):
            X.zero_()
            torch.cuda.synchronize()
            if solver == "pcg":
                _, its, _, times = hp.HPCCG_pcg(M, B, X, max_iter=max_iter, tolerance=0.0, device=True)
            else:
                _, its, _, times = hp.HPCCG_poly(M, B, X, degree=solver, max_iter=max_iter, tolerance=0.0, device=True)
            assert all(int(i) == max_iter - 1 for i in its), its
            return 1e6 * float(times[0]) / (max_iter - 1)

        solvers = ["pcg"] + list(DEGREES)
        for s in solvers:  # warm-up
            run(s)
        run("pcg")
        ref = (X.clone(), [M.last_trace_pcg(c).tobytes() for c in range(nrhs)])
        run(0)
        same = bool(torch.equal(X, ref[0])) and [M.last_trace_poly(c).tobytes() for c in range(nrhs)] == ref[1]
        us = {str(s): [] for s in solvers}
        for _ in range(args.reps):
            for s in solvers:
                us[str(s)].append(run(s))
        width = int(M.get_option("a_width")) or args.stencil
        print(json.dumps({"kind": "per_iteration", "stencil": args.stencil, "n": n, "rows": rows, "nrhs": nrhs,
                          "max_iter": max_iter, "slots_per_row": width, "us_per_iteration": us,
                          "spectrum": list(M.last_spectrum_poly()), "degree_0_bitwise_equal_to_pcg": same}), flush=True)
    finally:
        M.close()
    return 0


def child_time_to_solution(args):
    import numpy as np
    import oracle
    import torch
    hp = load_pkg()
    hp.set_device(0)
    dev = torch.device("cuda:0")
    n = args.n
    A = oracle.generate(n, n, n)
    rows = A.nrow
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(A.row_ptr))
    vals = A.vals.copy()
    vals[r == A.cols] = 26.0
    if args.scale == "p2":
        s = 2.0 ** np.random.default_rng(77).integers(-6, 7, rows)
        vals = (vals * s[r]) * s[A.cols.astype(np.int64)]
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, vals)
    del r, vals
    try:
        b = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), b)
        x = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPCCG(M, b, x, max_iter=1, device=True)
        r0 = float(M.last_trace()[0])
        tol = 1e-10 * r0
        lmax = hp.poly_bound(M)
        # (name, degree, eigenvalue ratio); degree None: Jacobi PCG
        runs = [("jacobi", None, None)] + [(f"degree_{d}", d, 30) for d in (1, 2, 3, 4)] + \
               [("degree_3_ratio_10", 3, 10), ("degree_3_ratio_100", 3, 100)]

        def run(degree, ratio):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if degree is None:
                _, its, nrs, _ = hp.HPCCG_pcg(M, b, x, max_iter=args.cap, tolerance=tol, device=True)
            else:
                _, its, nrs, _ = hp.HPCCG_poly(M, b, x, degree=degree, lmin=lmax / ratio, lmax=lmax, max_iter=args.cap,
                                               tolerance=tol, device=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, int(its[0]), float(nrs[0])

        for _, d, ratio in runs:  # warm-up
            run(d, ratio)
        out = {name: {"degree": d, "ratio": ratio, "seconds": []} for name, d, ratio in runs}
        for _ in range(args.reps):
            for name, d, ratio in runs:
                t, it, nr = run(d, ratio)
                rec = out[name]
                rec["seconds"].append(t)
                rec["niters"] = it
                rec["spmvs"] = it * ((d or 0) + 1)
                rec["normr_over_normr0"] = nr / r0
                rec["reached"] = nr <= tol
                rec["max_abs_x_minus_xexact"] = float((x - 1.0).abs().max())
        print(json.dumps({"kind": "time_to_solution", "n": n, "rows": rows, "scale": args.scale, "normr0": r0,
                          "tolerance": tol, "lmax": lmax, "a_width": int(M.get_option("a_width")), "runs": out}),
              flush=True)
    finally:
        M.close()
    return 0


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def spawn(extra, timeout):
    """One child process; its JSON record (the last line it prints)."""
    cmd = [sys.executable, os.path.abspath(__file__)] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {' '.join(extra)} ended with status {p.returncode}: nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="27:200,27:100,7:256", help="stencil:n, comma separated (empty: none)")
    ap.add_argument("--nrhs", default="1,4")
    ap.add_argument("--reps", type=int, default=3, help="alternations inside a process")
    ap.add_argument("--rounds", type=int, default=2, help="processes per configuration")
    ap.add_argument("--max-iter", type=int, default=150)
    ap.add_argument("--lap-n", type=int, default=100, help="0: no time-to-solution runs")
    ap.add_argument("--cap", type=int, default=2000, help="iteration limit of the time-to-solution runs")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly", "poly_bench.json"))
    ap.add_argument("--child", choices=["per_iteration", "time_to_solution"])
    ap.add_argument("--stencil", type=int, default=27)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--child-nrhs", type=int, default=1)
    ap.add_argument("--scale", choices=["plain", "p2"], default="plain")
    args = ap.parse_args()
    if args.child == "per_iteration":
        return child_per_iteration(args)
    if args.child == "time_to_solution":
        return child_time_to_solution(args)

    common = ["--reps", str(args.reps), "--max-iter", str(args.max_iter), "--cap", str(args.cap)]
    configs = []
    for sz in [v for v in args.sizes.split(",") if v]:
        st, n = (int(v) for v in sz.split(":"))
        for nrhs in [int(v) for v in args.nrhs.split(",")]:
            configs.append(["--child", "per_iteration", "--stencil", str(st), "--n", str(n), "--child-nrhs", str(nrhs)])
    if args.lap_n > 0:
        for scale in ("plain", "p2"):
            configs.append(["--child", "time_to_solution", "--n", str(args.lap_n), "--scale", scale])
    raw = []
    for rnd in range(args.rounds):
        for cfg in configs:
            rec = spawn(cfg + common, args.child_timeout)
            rec["round"] = rnd
            raw.append(rec)
            print(json.dumps(rec), flush=True)

    per_it, tts = [], []
    for cfg in configs:
        if cfg[1] == "per_iteration":
            st, n, nrhs = int(cfg[3]), int(cfg[5]), int(cfg[7])
            recs = [r for r in raw if r["kind"] == "per_iteration" and (r["stencil"], r["n"], r["nrhs"]) == (st, n, nrhs)]
            us = {s: summary([v for r in recs for v in r["us_per_iteration"][s]]) for s in recs[0]["us_per_iteration"]}
            w = recs[0]["slots_per_row"]
            d0 = us["0"]["median"]
            per_it.append({"stencil": st, "n": n, "nrhs": nrhs, "slots_per_row": w, "us_per_iteration": us,
                           "degree_0_over_pcg": d0 / us["pcg"]["median"],
                           "us_per_step": {str(d): (us[str(d)]["median"] - d0) / d for d in DEGREES if d},
                           "step_model_bytes_per_row": step_model_bytes_per_row(w, nrhs),
                           "degree_0_bitwise_equal_to_pcg": all(r["degree_0_bitwise_equal_to_pcg"] for r in recs)})
        else:
            scale = cfg[5]
            recs = [r for r in raw if r["kind"] == "time_to_solution" and r["scale"] == scale]
            runs = {}
            for name, last in recs[-1]["runs"].items():
                runs[name] = {k: v for k, v in last.items() if k != "seconds"}
                runs[name]["seconds"] = summary([v for r in recs for v in r["runs"][name]["seconds"]])
            tts.append({"n": recs[0]["n"], "scale": scale, "lmax": recs[0]["lmax"], "runs": runs})
    doc = {"per_iteration": per_it, "time_to_solution": tts, "raw": raw}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in per_it if not r["degree_0_bitwise_equal_to_pcg"]]
    bad += [r for t in tts for r in t["runs"].values() if not r["reached"] or r["max_abs_x_minus_xexact"] > 1e-4]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
