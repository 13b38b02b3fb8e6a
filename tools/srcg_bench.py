#!/usr/bin/env python3
"""Single-reduction preconditioned CG (hpccg_hip_srcg_solve_device) against the
classic recurrence (hpccg_hip_pcg_solve_device): what three launches and one
finalize per iteration are worth against five and two, for one more vector.
The driver starts one child process per configuration and visits the
configurations in turn, `--rounds` times (so a configuration's processes are
spread over the run); inside a process the two solvers alternate `--reps` times
on the same matrix and vectors after a warm-up of each. Reported per
configuration and solver: the median with min and max over every repetition of
every process, the ratio of the medians, and the raw records. No ratio is
required: the run fails on a wrong result only.

Before any timing every child compares HPCCG_srcg at max_iter 2 with HPCCG_pcg
bitwise (x, niters, normr, traces: the first iteration is the same arithmetic);
a mismatch ends the run with exit status 1.

1. Per-iteration cost (configuration: stencil, size, columns). Both solvers
   with Jacobi on the same device columns, max_iter `--max-iter` at tolerance
   0; microseconds per iteration from the solve's device events. Beside the
   measured ratio stands the byte model's (bytes per row and
   iteration for R columns of one launch, 8 W + 16 + 88 R for the classic
   recurrence, 8 W + 8 + 104 R for this one; W slots per row).

2. Time to solution (configuration: matrix). The 27-point n^3 stencil
   (--tts-n, default 100) with every entry a_ij s_i s_j, s_i = 2^e_i, e_i
   random in [-6, 6] ("p2"), and the same pattern with every diagonal entry
   26.0 (weakly diagonally dominant, "lap26"); b = A 1. Iterations and wall
   time until normr <= 1e-10 normr_0 for both solvers; every run's final x is
   checked against xexact = 1 (the record keeps the error).

usage: tools/srcg_bench.py [--sizes 27:200,27:100,7:256] [--nrhs 1,4] [--reps 3] [--rounds 2]
                           [--tts-n 100] [--out profiles/srcg/srcg_bench.json]
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

MAX_R = 4  # columns per launch (the widest instantiation)
SOLVERS = ("pcg", "srcg")


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "count": len(v)}


def model_ratio(width, nrhs):
    """Predicted srcg / pcg rate from the byte model (the docstring's)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    return (launches * (8 * width + 16) + 88 * nrhs) / (launches * (8 * width + 8) + 104 * nrhs)


def solver_of(hp, name):
    return hp.HPCCG_pcg if name == "pcg" else hp.HPCCG_srcg


def trace_of(M, name, c):
    return (M.last_trace_pcg if name == "pcg" else M.last_trace_srcg)(c).tobytes()


def first_iteration_is_bitwise(hp, torch, M, B, X):
    """max_iter 2: the two solvers' x, niters, normr and traces, bit for bit."""
    got = {}
    for name in SOLVERS:
        X.zero_()
        _, its, nrs, _ = solver_of(hp, name)(M, B, X, max_iter=2, tolerance=0.0, device=True)
        nrhs = 1 if B.dim() == 1 else B.shape[0]
        got[name] = (X.clone(), its.tobytes(), nrs.tobytes(), [trace_of(M, name, c) for c in range(nrhs)])
    a, b = got["pcg"], got["srcg"]
    return bool(torch.equal(a[0], b[0])) and a[1:] == b[1:]


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
        same = first_iteration_is_bitwise(hp, torch, M, B, X)

        def run(name):
            X.zero_()
            torch.cuda.synchronize()
            _, its, _, times = solver_of(hp, name)(M, B, X, max_iter=max_iter, tolerance=0.0, device=True)
            assert all(int(i) == max_iter - 1 for i in its), its
            return 1e6 * float(times[0]) / (max_iter - 1)

        for s in SOLVERS:  # warm-up
            run(s)
        us = {s: [] for s in SOLVERS}
        for _ in range(args.reps):
            for s in SOLVERS:
                us[s].append(run(s))
        width = int(M.get_option("a_width")) or args.stencil
        print(json.dumps({"kind": "per_iteration", "stencil": args.stencil, "n": n, "rows": rows, "nrhs": nrhs,
                          "max_iter": max_iter, "slots_per_row": width, "nt": int(M.get_option("nt")),
                          "us_per_iteration": us, "first_iteration_bitwise_equal_to_pcg": same}), flush=True)
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
    if args.matrix == "lap26":
        vals[r == A.cols] = 26.0
    else:
        s = 2.0 ** np.random.default_rng(77).integers(-6, 7, rows)
        vals = (vals * s[r]) * s[A.cols.astype(np.int64)]
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, vals)
    del r, vals
    try:
        b = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), b)
        x = torch.zeros(rows, dtype=torch.float64, device=dev)
        same = first_iteration_is_bitwise(hp, torch, M, b, x)
        x.zero_()
        hp.HPCCG(M, b, x, max_iter=1, device=True)
        r0 = float(M.last_trace()[0])
        tol = 1e-10 * r0

        def run(name):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, its, nrs, _ = solver_of(hp, name)(M, b, x, max_iter=args.cap, tolerance=tol, device=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, int(its[0]), float(nrs[0])

        for s in SOLVERS:  # warm-up
            run(s)
        out = {s: {"seconds": []} for s in SOLVERS}
        for _ in range(args.reps):
            for s in SOLVERS:
                t, it, nr = run(s)
                rec = out[s]
                rec["seconds"].append(t)
                rec["niters"] = it
                rec["normr_over_normr0"] = nr / r0
                rec["reached"] = nr <= tol
                rec["max_abs_x_minus_xexact"] = float((x - 1.0).abs().max())
        print(json.dumps({"kind": "time_to_solution", "n": n, "rows": rows, "matrix": args.matrix, "normr0": r0,
                          "tolerance": tol, "a_width": int(M.get_option("a_width")), "runs": out,
                          "first_iteration_bitwise_equal_to_pcg": same}), flush=True)
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
    ap.add_argument("--tts-n", type=int, default=100, help="0: no time-to-solution runs")
    ap.add_argument("--cap", type=int, default=2000, help="iteration limit of the time-to-solution runs")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srcg", "srcg_bench.json"))
    ap.add_argument("--child", choices=["per_iteration", "time_to_solution"])
    ap.add_argument("--stencil", type=int, default=27)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--child-nrhs", type=int, default=1)
    ap.add_argument("--matrix", choices=["p2", "lap26"], default="p2")
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
    if args.tts_n > 0:
        for matrix in ("p2", "lap26"):
            configs.append(["--child", "time_to_solution", "--n", str(args.tts_n), "--matrix", matrix])
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
            us = {s: summary([v for r in recs for v in r["us_per_iteration"][s]]) for s in SOLVERS}
            w = recs[0]["slots_per_row"]
            # per process: the ratio of that process's medians (the placement of a process's allocations cancels)
            per_proc = [statistics.median(r["us_per_iteration"]["pcg"]) / statistics.median(r["us_per_iteration"]["srcg"])
                        for r in recs]
            per_it.append({"stencil": st, "n": n, "nrhs": nrhs, "slots_per_row": w, "us_per_iteration": us,
                           "srcg_rate_over_pcg": us["pcg"]["median"] / us["srcg"]["median"],
                           "srcg_rate_over_pcg_per_process": per_proc, "model_ratio": model_ratio(w, nrhs),
                           "first_iteration_bitwise_equal_to_pcg": all(r["first_iteration_bitwise_equal_to_pcg"]
                                                                       for r in recs)})
        else:
            matrix = cfg[5]
            recs = [r for r in raw if r["kind"] == "time_to_solution" and r["matrix"] == matrix]
            runs = {}
            for name, last in recs[-1]["runs"].items():
                runs[name] = {k: v for k, v in last.items() if k != "seconds"}
                runs[name]["seconds"] = summary([v for r in recs for v in r["runs"][name]["seconds"]])
            tts.append({"n": recs[0]["n"], "matrix": matrix, "runs": runs,
                        "srcg_speed_over_pcg": runs["pcg"]["seconds"]["median"] / runs["srcg"]["seconds"]["median"],
                        "first_iteration_bitwise_equal_to_pcg": all(r["first_iteration_bitwise_equal_to_pcg"]
                                                                    for r in recs)})
    doc = {"per_iteration": per_it, "time_to_solution": tts, "raw": raw}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in per_it + tts if not r["first_iteration_bitwise_equal_to_pcg"]]
    bad += [r for t in tts for r in t["runs"].values() if not r["reached"] or r["max_abs_x_minus_xexact"] > 1e-4]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
