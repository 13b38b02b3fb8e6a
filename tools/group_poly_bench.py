#!/usr/bin/env python3
"""Chebyshev polynomial preconditioned CG over an in-process rank group
(hpccg_hip_group_poly_solve_device): what a step costs per iteration against
the group pcg's iteration, what the halo kernel of z buys against the halo by
copies, and whether trading iterations (two group sums with their event waits
each) for steps (one halo each, no dot) pays in time to solution. All members on
one GPU. The driver starts one child process per configuration, one after
another, and visits the configurations in turn `--rounds` times; inside a
process the solvers alternate `--reps` times after a warm-up of each. Times are
the solves' own (device events on member 0's stream). Reported per
configuration and solver: the median with min and max over every repetition of
every process, and the raw records.

1. Per-iteration cost (configuration: members x local grid, columns).
   group_HPCCG_pcg with Jacobi, group_HPCCG_poly at degrees 0 to 4, and degree 3
   with the halos by copies, on the same device columns, max_iter `--max-iter`
   at tolerance 0; microseconds per iteration. Degree 0 is compared with the
   group pcg bitwise (every member's x, niters, traces) before any timing; a
   mismatch ends the run with exit status 1. The cost of a step is the
   difference to degree 0 per degree: it includes the step's halo of z. Beside
   it the byte model of one step per row and column: (8 W + 8) / R + 48 bytes
   (tools/poly_bench.py) plus the ghost planes the halo moves, 16 bytes per
   ghost row and column (read and written once).

2. Time to solution (configuration: plain or "p2" scaling, members). The
   27-point n^3 pattern (--lap-n) with every diagonal entry 26.0, plain and
   scaled by s_i = 2^e_i, split into z-slabs; b = A 1, one column. Iterations,
   SpMVs and milliseconds until normr <= 1e-10 normr_0 for group_HPCCG_pcg and
   for degrees 1 to 4 at the default interval. Every run's final x is checked
   against xexact = 1.

usage: tools/group_poly_bench.py [--sizes 2:200x200x100,2:100x100x50] [--nrhs 1,4] [--reps 3] [--rounds 2]
                                 [--lap-n 100] [--lap-members 2,8] [--out profiles/group_poly/group_poly_bench.json]
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

DEGREES = (0, 1, 2, 3, 4)
MAX_R = 4  # columns per launch (the widest instantiation)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "count": len(v)}


def step_model_bytes_per_row(width, nrhs, rows, ghost_rows):
    """Bytes per row one step moves for all nrhs columns (the docstring's model)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    return launches * (8 * width + 8) + 48 * nrhs + 16.0 * nrhs * ghost_rows / rows


# ---------------------------------------------------------------------------
# children
# ---------------------------------------------------------------------------
def child_per_iteration(args):
    import torch
    hp = load_pkg()
    hp.set_device(0)
    dev = torch.device("cuda:0")
    P, (nx, ny, nz) = args.members, (int(v) for v in args.grid.split("x"))
    nrhs, max_iter = args.child_nrhs, args.max_iter
    Ms = hp.group_generate(nx, ny, nz, P)
    rows = nx * ny * nz
    try:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        Bs = [torch.rand((nrhs, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0 for _ in Ms]
        one2 = [torch.ones((2, rows), dtype=torch.float64, device=dev) for _ in Ms]
        y2 = [torch.zeros((2, rows), dtype=torch.float64, device=dev) for _ in Ms]
        hp.group_sparsemv_batch(Ms, one2, y2)  # column 0: b = A 1
        for b, y in zip(Bs, y2):
            b[0].copy_(y[0])
        del one2, y2
        Xs = [torch.zeros((nrhs, rows), dtype=torch.float64, device=dev) for _ in Ms]

        def run(solver):
            for x in Xs:
                x.zero_()
            torch.cuda.synchronize()
            if solver == "pcg":
                its, _, times = hp.group_HPCCG_pcg(Ms, Bs, Xs, max_iter=max_iter, tolerance=0.0)
            elif solver == "3_copies":
                its, _, times = hp.group_HPCCG_poly(Ms, Bs, Xs, degree=3, max_iter=max_iter, tolerance=0.0,
                                                    halo_copies=True)
            else:
                its, _, times = hp.group_HPCCG_poly(Ms, Bs, Xs, degree=solver, max_iter=max_iter, tolerance=0.0)
            assert all(int(i) == max_iter - 1 for i in its), its
            return 1e6 * float(times[0]) / (max_iter - 1)

        # the bitwise check before any timing: degree 0 is the group pcg
        run("pcg")
        ref = ([x.clone() for x in Xs], [hp.group_last_trace_pcg(Ms, c).tobytes() for c in range(nrhs)])
        run(0)
        same = all(bool(torch.equal(a, b)) for a, b in zip(Xs, ref[0])) and \
            [hp.group_last_trace_poly(Ms, c).tobytes() for c in range(nrhs)] == ref[1]
        solvers = ["pcg"] + list(DEGREES) + ["3_copies"]
        us = {str(s): [] for s in solvers}
        if same:
            for s in solvers:  # warm-up
                run(s)
            for _ in range(args.reps):
                for s in solvers:
                    us[str(s)].append(run(s))
        width = int(Ms[0].get_option("a_width")) or 27
        print(json.dumps({"kind": "per_iteration", "members": P, "grid": [nx, ny, nz], "rows_per_member": rows,
                          "ghost_rows_per_member": 2.0 * nx * ny * (P - 1) / P, "nrhs": nrhs, "max_iter": max_iter,
                          "slots_per_row": width, "us_per_iteration": us,
                          "spectrum": list(hp.group_last_spectrum_poly(Ms)),
                          "degree_0_bitwise_equal_to_group_pcg": same}), flush=True)
    finally:
        for M in Ms:
            M.close()
    return 0 if same else 1


def child_time_to_solution(args):
    import numpy as np
    import oracle
    import torch
    hp = load_pkg()
    hp.set_device(0)
    dev = torch.device("cuda:0")
    n, P = args.n, args.members
    A = oracle.generate(n, n, n)
    rows = A.nrow
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(A.row_ptr))
    vals = A.vals.copy()
    vals[r == A.cols] = 26.0
    if args.scale == "p2":
        s = 2.0 ** np.random.default_rng(77).integers(-6, 7, rows)
        vals = (vals * s[r]) * s[A.cols.astype(np.int64)]
    b = np.bincount(r, weights=vals, minlength=rows)  # b = A 1
    del r
    planes = [n // P + (1 if k < n % P else 0) for k in range(P)]
    parts, start = [], 0
    for pl in planes:
        cnt = pl * n * n
        lo, hi = int(A.row_ptr[start]), int(A.row_ptr[start + cnt])
        parts.append((A.row_ptr[start:start + cnt + 1] - lo, A.cols[lo:hi], vals[lo:hi], start))
        start += cnt
    Ms = hp.group_from_csr(parts, rows)
    try:
        assert all(M.get_option("halo_mode") == 1 for M in Ms), "members of the z-slab plan expected"
        Bs, Xs = [], []
        for rp, _, _, st in parts:
            cnt = len(rp) - 1
            Bs.append(torch.from_numpy(b[st:st + cnt].copy()).to(dev).reshape(1, cnt))
            Xs.append(torch.zeros((1, cnt), dtype=torch.float64, device=dev))
        r0 = float(np.sqrt(np.dot(b, b)))
        tol = 1e-10 * r0
        runs = [("jacobi", None)] + [(f"degree_{d}", d) for d in (1, 2, 3, 4)]

        def run(degree):
            for x in Xs:
                x.zero_()
            torch.cuda.synchronize()
            if degree is None:
                its, nrs, times = hp.group_HPCCG_pcg(Ms, Bs, Xs, max_iter=args.cap, tolerance=tol)
            else:
                its, nrs, times = hp.group_HPCCG_poly(Ms, Bs, Xs, degree=degree, max_iter=args.cap, tolerance=tol)
            return float(times[0]), int(its[0]), float(nrs[0])

        for _, d in runs:  # warm-up
            run(d)
        out = {name: {"degree": d, "seconds": []} for name, d in runs}
        for _ in range(args.reps):
            for name, d in runs:
                t, it, nr = run(d)
                rec = out[name]
                rec["seconds"].append(t)
                rec["niters"] = it
                rec["spmvs"] = it * ((d or 0) + 1)
                rec["normr_over_normr0"] = nr / r0
                rec["reached"] = nr <= tol
                rec["max_abs_x_minus_xexact"] = max(float((x - 1.0).abs().max()) for x in Xs)
        print(json.dumps({"kind": "time_to_solution", "n": n, "rows": rows, "scale": args.scale, "members": P,
                          "planes": planes, "normr0": r0, "tolerance": tol, "lmax": hp.group_poly_bound(Ms),
                          "a_width": int(Ms[0].get_option("a_width")), "runs": out}), flush=True)
    finally:
        for M in Ms:
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
    ap.add_argument("--sizes", default="2:200x200x100,2:100x100x50",
                    help="members:nx x ny x nz of every member, comma separated (empty: none)")
    ap.add_argument("--nrhs", default="1,4")
    ap.add_argument("--reps", type=int, default=3, help="alternations inside a process")
    ap.add_argument("--rounds", type=int, default=2, help="processes per configuration")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--lap-n", type=int, default=100, help="0: no time-to-solution runs")
    ap.add_argument("--lap-members", default="2,8")
    ap.add_argument("--cap", type=int, default=2000, help="iteration limit of the time-to-solution runs")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_poly", "group_poly_bench.json"))
    ap.add_argument("--child", choices=["per_iteration", "time_to_solution"])
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--grid", default="100x100x50")
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
        P, grid = sz.split(":")
        for nrhs in [int(v) for v in args.nrhs.split(",")]:
            configs.append(["--child", "per_iteration", "--members", P, "--grid", grid, "--child-nrhs", str(nrhs)])
    if args.lap_n > 0:
        for scale in ("plain", "p2"):
            for P in [v for v in args.lap_members.split(",") if v]:
                configs.append(["--child", "time_to_solution", "--n", str(args.lap_n), "--scale", scale, "--members", P])
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
            P, grid, nrhs = int(cfg[3]), [int(v) for v in cfg[5].split("x")], int(cfg[7])
            recs = [r for r in raw if r["kind"] == "per_iteration" and
                    (r["members"], r["grid"], r["nrhs"]) == (P, grid, nrhs)]
            us = {s: summary([v for r in recs for v in r["us_per_iteration"][s]]) for s in recs[0]["us_per_iteration"]}
            w = recs[0]["slots_per_row"]
            d0, pcg = us["0"]["median"], us["pcg"]["median"]
            step = {str(d): (us[str(d)]["median"] - d0) / d for d in DEGREES if d}
            per_it.append({"members": P, "grid": grid, "nrhs": nrhs, "slots_per_row": w, "us_per_iteration": us,
                           "degree_0_over_group_pcg": d0 / pcg, "us_per_step": step,
                           "step_over_group_pcg_iteration": {d: v / pcg for d, v in step.items()},
                           "us_per_step_degree_3_halo_copies": (us["3_copies"]["median"] - d0) / 3,
                           "degree_3_copies_over_kernel": us["3_copies"]["median"] / us["3"]["median"],
                           "step_model_bytes_per_row": step_model_bytes_per_row(
                               w, nrhs, recs[0]["rows_per_member"], recs[0]["ghost_rows_per_member"]),
                           "degree_0_bitwise_equal_to_group_pcg":
                               all(r["degree_0_bitwise_equal_to_group_pcg"] for r in recs)})
        else:
            scale, P = cfg[5], int(cfg[7])
            recs = [r for r in raw if r["kind"] == "time_to_solution" and (r["scale"], r["members"]) == (scale, P)]
            runs = {}
            for name, last in recs[-1]["runs"].items():
                runs[name] = {k: v for k, v in last.items() if k != "seconds"}
                runs[name]["seconds"] = summary([v for r in recs for v in r["runs"][name]["seconds"]])
            jac = runs["jacobi"]["seconds"]["median"]
            for v in runs.values():
                v["seconds_over_jacobi"] = v["seconds"]["median"] / jac
            tts.append({"n": recs[0]["n"], "scale": scale, "members": P, "lmax": recs[0]["lmax"], "runs": runs})
    doc = {"per_iteration": per_it, "time_to_solution": tts, "raw": raw}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in per_it if not r["degree_0_bitwise_equal_to_group_pcg"]]
    bad += [r for t in tts for r in t["runs"].values() if not r["reached"] or r["max_abs_x_minus_xexact"] > 1e-4]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
