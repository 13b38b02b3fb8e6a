#!/usr/bin/env python3
"""Single-reduction CG with the Chebyshev polynomial preconditioner on one rank
(hpccg_hip_srpoly_solve_device) against the polynomial preconditioned CG
(hpccg_hip_poly_solve_device) and the single-reduction CG
(hpccg_hip_srcg_solve_device) on the same matrix and columns: what 3 + d
launches and one finalize per outer iteration cost against 5 + d and two, with
16 R more bytes per row. The driver starts one child process per configuration,
one after another, each under its own `timeout`, and visits the configurations
in turn `--rounds` times; it stops at the first child that fails. Inside a
process the solvers alternate `--reps` times after a warm-up of each. Times are
the solves' own (device events around the recurrence). Reported per
configuration, degree and solver: the median with min and max over every
repetition of every process, the ratio of the medians, the ratio per process,
the byte model's ratio (per row and outer iteration for R columns
of one launch a step is 8 W + 8 + 48 R in both forms; around the steps the
classic form moves 8 W + 8 + 104 R and this one 8 W + 8 + 120 R, W slots per
row) and the raw records. No ratio is required: the run fails on a wrong result
only.

Before any timing every child compares, bitwise (x, niters, normr, traces):
HPCCG_srpoly at max_iter 2 with HPCCG_poly at every degree, and HPCCG_srpoly at
degree 0 with HPCCG_srcg over 20 iterations; a mismatch ends the run with exit
status 1.

usage: tools/srpoly_bench.py [--sizes 27:200x200x200,27:100x100x100,7:256x256x256] [--nrhs 1,4]
                             [--degrees 0,1,2,3,4] [--reps 3] [--rounds 2] [--out profiles/srpoly/srpoly_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from bench import load_pkg  # noqa: E402

MAX_R = 4  # columns per launch (the widest instantiation)
CHECK = "bitwise_equal_first_iteration_to_poly_and_degree_0_to_srcg"


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "count": len(v)}


def model_ratio(width, nrhs, d):
    """Predicted srpoly / poly rate at degree d >= 1 from the byte model (the docstring's)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    steps = d * (launches * (8 * width + 8) + 48 * nrhs)
    return (steps + launches * (8 * width + 8) + 104 * nrhs) / (steps + launches * (8 * width + 8) + 120 * nrhs)


def solve(hp, name, d, M, B, X, max_iter):
    if name == "srcg":
        return hp.HPCCG_srcg(M, B, X, max_iter=max_iter, tolerance=0.0, device=True)
    f = hp.HPCCG_poly if name == "poly" else hp.HPCCG_srpoly
    return f(M, B, X, degree=d, max_iter=max_iter, tolerance=0.0, device=True)


def trace_of(name, M, c):
    return {"srcg": M.last_trace_srcg, "poly": M.last_trace_poly, "srpoly": M.last_trace_srpoly}[name](c).tobytes()


def same_bits(hp, torch, M, B, X, nrhs, a, b, max_iter):
    """Solvers a and b, (name, degree) each: x, niters, normr and traces, bit for bit."""
    got = []
    for name, d in (a, b):
        X.zero_()
        _, its, nrs, _ = solve(hp, name, d, M, B, X, max_iter)
        got.append((X.clone(), its.tobytes(), nrs.tobytes(), [trace_of(name, M, c) for c in range(nrhs)]))
    return bool(torch.equal(got[0][0], got[1][0])) and got[0][1:] == got[1][1:]


def solvers(degrees):
    return [("srcg", 0)] + [(s, d) for d in degrees for s in ("poly", "srpoly")]


def key(s):
    return s[0] if s[0] == "srcg" else f"{s[0]}_{s[1]}"


def child(args):
    import torch
    hp = load_pkg()
    hp.set_device(0)
    dev = torch.device("cuda:0")
    nx, ny, nz = (int(v) for v in args.grid.split("x"))
    nrhs, max_iter = args.child_nrhs, args.max_iter
    degrees = [int(v) for v in args.degrees.split(",")]
    M = hp.Matrix.generate(nx, ny, nz, use_7pt=args.stencil == 7)
    rows = nx * ny * nz
    same = False
    try:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        B = torch.rand((nrhs, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        y = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), y)  # column 0: b = A 1
        B[0].copy_(y)
        del y
        X = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)
        same = all(same_bits(hp, torch, M, B, X, nrhs, ("srpoly", d), ("poly", d), 2) for d in degrees)
        same = same and same_bits(hp, torch, M, B, X, nrhs, ("srpoly", 0), ("srcg", 0), 20)
        short = {}

        def run(s):
            X.zero_()
            torch.cuda.synchronize()
            _, its, _, times = solve(hp, s[0], s[1], M, B, X, max_iter)
            # (a column whose recurrence breaks down in rounding noise ends early: the launches go on
            # until the last column ends, so the time is divided by the iterations of that one)
            short[key(s)] = min(short.get(key(s), max_iter), int(min(its)))
            return 1e6 * float(times[0]) / int(max(its))

        todo = solvers(degrees)
        us = {key(s): [] for s in todo}
        if same:
            for s in todo:  # warm-up
                run(s)
            for _ in range(args.reps):
                for s in todo:
                    us[key(s)].append(run(s))
        width = int(M.get_option("a_width")) or args.stencil
        print(json.dumps({"grid": [nx, ny, nz], "stencil": args.stencil, "rows": rows, "nrhs": nrhs,
                          "max_iter": max_iter, "slots_per_row": width, "nt": int(M.get_option("nt")),
                          "degrees": degrees, "us_per_iteration": us, "fewest_iterations_of_a_column": short,
                          CHECK: same}), flush=True)
    finally:
        M.close()
    return 0 if same else 1


def spawn(extra, timeout):
    """One child process under its own `timeout`; its JSON record (the last line it prints)."""
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {' '.join(extra)} ended with status {p.returncode}: nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="27:200x200x200,27:100x100x100,7:256x256x256", help="stencil:nx x ny x nz")
    ap.add_argument("--nrhs", default="1,4")
    ap.add_argument("--degrees", default="0,1,2,3,4")
    ap.add_argument("--reps", type=int, default=3, help="alternations inside a process")
    ap.add_argument("--rounds", type=int, default=2, help="processes per configuration")
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srpoly", "srpoly_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--grid", default="100x100x100")
    ap.add_argument("--stencil", type=int, default=27)
    ap.add_argument("--child-nrhs", type=int, default=1)
    args = ap.parse_args()
    if args.child:
        return child(args)

    degrees = [int(v) for v in args.degrees.split(",")]
    assert 0 in degrees, "degree 0 is the check against HPCCG_srcg"
    common = ["--child", "--reps", str(args.reps), "--max-iter", str(args.max_iter), "--degrees", args.degrees]
    configs = [(st, grid, nrhs) for st, grid in (v.split(":") for v in args.sizes.split(",") if v)
               for nrhs in (int(v) for v in args.nrhs.split(","))]
    raw = []
    for rnd in range(args.rounds):
        for st, grid, nrhs in configs:
            rec = spawn(["--stencil", st, "--grid", grid, "--child-nrhs", str(nrhs)] + common, args.child_timeout)
            rec["round"] = rnd
            raw.append(rec)
            print(json.dumps(rec), flush=True)

    names = [key(s) for s in solvers(degrees)]
    out = []
    for st, grid, nrhs in configs:
        g = [int(v) for v in grid.split("x")]
        recs = [r for r in raw if (r["stencil"], r["grid"], r["nrhs"]) == (int(st), g, nrhs)]
        us = {s: summary([v for r in recs for v in r["us_per_iteration"][s]]) for s in names}
        # per process: the ratio of that process's medians (the placement of a process's allocations cancels)
        med = [{s: statistics.median(r["us_per_iteration"][s]) for s in names} for r in recs]
        w = recs[0]["slots_per_row"]
        by_degree = []
        for d in degrees:
            p, q = f"poly_{d}", f"srpoly_{d}"
            by_degree.append({"degree": d, "us_per_iteration": {"poly": us[p], "srpoly": us[q]},
                              "us_per_step": {"poly": us[p]["median"] / (d + 1), "srpoly": us[q]["median"] / (d + 1)},
                              "srpoly_rate_over_poly": us[p]["median"] / us[q]["median"],
                              "srpoly_rate_over_poly_per_process": [m[p] / m[q] for m in med],
                              "model_ratio": model_ratio(w, nrhs, d) if d else None})
        out.append({"stencil": int(st), "grid": g, "nrhs": nrhs, "slots_per_row": w, "us_per_iteration_srcg": us["srcg"],
                    "srpoly_0_rate_over_srcg": us["srcg"]["median"] / us["srpoly_0"]["median"], "degrees": by_degree,
                    CHECK: all(r[CHECK] for r in recs)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"per_iteration": out, "raw": raw}, f, indent=1)
        f.write("\n")
    bad = [r for r in out if not r[CHECK]]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
