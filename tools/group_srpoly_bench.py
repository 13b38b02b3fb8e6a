#!/usr/bin/env python3
"""Single-reduction CG with the Chebyshev polynomial preconditioner over an
in-process rank group (hpccg_hip_group_srpoly_solve_device) against the two
solvers it combines, over the same group: the polynomial preconditioned CG
(hpccg_hip_group_poly_solve_device: two sums over the members per outer
iteration) and the single-reduction CG (hpccg_hip_group_srcg_solve_device: one
sum, diag(m) only). What one sum instead of two is worth at degree d against
the 16 R bytes per row the fused step costs more. All members on one GPU. The
driver starts one child process per configuration, one after another, each
under its own `timeout`, and visits the configurations in turn `--rounds` times;
it stops at the first child that fails. Inside a process the solvers alternate
`--reps` times on the same members and columns after a warm-up of each. Times
are the solves' own (device events on member 0's stream). Reported per
configuration, degree and solver: the median with min and max over every
repetition of every process, the ratio of the medians, the ratio per process,
and the raw records. No ratio is required: the run fails on a wrong result only.

Before any timing every child compares, bitwise (every member's x, niters,
normr, traces): group_HPCCG_srpoly at max_iter 2 with group_HPCCG_poly at every
degree (the first iteration is the same arithmetic), and group_HPCCG_srpoly at
degree 0 with group_HPCCG_srcg over the whole run; a mismatch ends the run with
exit status 1.

1. Per-iteration cost (configuration: members x local grid, stencil, columns).
   Degrees `--degrees`, Jacobi, the default interval, max_iter `--max-iter` at
   tolerance 0: microseconds per outer iteration and per polynomial step (an
   outer iteration is d + 1 passes over the matrix: divided by d + 1). Beside
   the measured ratio stands the byte model's (bytes per row and
   outer iteration for R columns of one launch; a step is 8 W + 8 + 48 R in
   both; around them the classic form has p, SpMM and the update with step 0,
   8 W + 8 + 104 R, and this one the fused step and the SpMM, 8 W + 8 + 120 R,
   W slots per row; both plus 16 bytes per ghost row, column and halo).

2. Time to solution (configuration: matrix, members). The 27-point n^3 pattern
   (--tts-n, default 100) with every diagonal entry 26.0 ("lap26") and the
   same with every entry a_ij s_i s_j, s_i = 2^e_i, e_i random in [-6, 6]
   ("lap26_p2"), split into z-slabs; b = A 1, one column. Iterations and
   milliseconds until normr <= 1e-10 normr_0 for group_HPCCG_poly and
   group_HPCCG_srpoly at every degree and for group_HPCCG_srcg; every run's
   final x is checked against xexact = 1 (the record keeps the error).

usage: tools/group_srpoly_bench.py [--sizes 2:100x100x50:27,8:100x100x13:27] [--nrhs 1,4]
                                   [--sizes-one 2:200x200x100:27] [--degrees 0,1,2,3,4] [--reps 3] [--rounds 2]
                                   [--tts-n 100] [--tts-members 2,8]
                                   [--out profiles/srpoly/group_srpoly_bench.json]
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
CHECK = "bitwise_equal_first_iteration_to_group_poly_and_degree_0_to_group_srcg"


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "count": len(v)}


def model_ratio(width, nrhs, rows, ghost_rows, d):
    """Predicted srpoly / poly rate at degree d >= 1 from the byte model (the docstring's)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    halo = 16.0 * nrhs * ghost_rows / rows * (d + 1)
    steps = d * (launches * (8 * width + 8) + 48 * nrhs)
    return (steps + launches * (8 * width + 8) + 104 * nrhs + halo) / \
        (steps + launches * (8 * width + 8) + 120 * nrhs + halo)


def solve(hp, name, d, Ms, Bs, Xs, max_iter, tol):
    if name == "srcg":
        return hp.group_HPCCG_srcg(Ms, Bs, Xs, max_iter=max_iter, tolerance=tol)
    f = hp.group_HPCCG_poly if name == "poly" else hp.group_HPCCG_srpoly
    return f(Ms, Bs, Xs, degree=d, max_iter=max_iter, tolerance=tol)


def trace_of(hp, name, Ms, c):
    f = {"srcg": hp.group_last_trace_srcg, "poly": hp.group_last_trace_poly, "srpoly": hp.group_last_trace_srpoly}
    return f[name](Ms, c).tobytes()


def same_bits(hp, torch, Ms, Bs, Xs, nrhs, a, b, max_iter):
    """Solvers a and b, (name, degree) each: every member's x, niters, normr and traces, bit for bit."""
    got = []
    for name, d in (a, b):
        for x in Xs:
            x.zero_()
        its, nrs, _ = solve(hp, name, d, Ms, Bs, Xs, max_iter, 0.0)
        got.append(([x.clone() for x in Xs], its.tobytes(), nrs.tobytes(),
                    [trace_of(hp, name, Ms, c) for c in range(nrhs)]))
    return all(bool(torch.equal(p, q)) for p, q in zip(got[0][0], got[1][0])) and got[0][1:] == got[1][1:]


def checks(hp, torch, Ms, Bs, Xs, nrhs, degrees, max_iter):
    ok = all(same_bits(hp, torch, Ms, Bs, Xs, nrhs, ("srpoly", d), ("poly", d), 2) for d in degrees)
    return ok and same_bits(hp, torch, Ms, Bs, Xs, nrhs, ("srpoly", 0), ("srcg", 0), max_iter)


def solvers(degrees):
    return [("srcg", 0)] + [(s, d) for d in degrees for s in ("poly", "srpoly")]


def key(s):
    return s[0] if s[0] == "srcg" else f"{s[0]}_{s[1]}"


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
    degrees = [int(v) for v in args.degrees.split(",")]
    Ms = hp.group_generate(nx, ny, nz, P, use_7pt=args.stencil == 7)
    rows = nx * ny * nz
    same = False
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
        same = checks(hp, torch, Ms, Bs, Xs, nrhs, degrees, 20)

        def run(s):
            for x in Xs:
                x.zero_()
            torch.cuda.synchronize()
            its, _, times = solve(hp, s[0], s[1], Ms, Bs, Xs, max_iter, 0.0)
            # (a column whose recurrence breaks down in rounding noise ends early: the launches go on
            # until the last column ends, so the time is divided by the iterations of that one)
            short[key(s)] = min(short.get(key(s), max_iter), int(min(its)))
            return 1e6 * float(times[0]) / int(max(its))

        todo = solvers(degrees)
        short = {}
        us = {key(s): [] for s in todo}
        if same:
            for s in todo:  # warm-up
                run(s)
            for _ in range(args.reps):
                for s in todo:
                    us[key(s)].append(run(s))
        width = int(Ms[0].get_option("a_width")) or args.stencil
        print(json.dumps({"kind": "per_iteration", "members": P, "grid": [nx, ny, nz], "stencil": args.stencil,
                          "rows_per_member": rows, "ghost_rows_per_member": 2.0 * nx * ny * (P - 1) / P, "nrhs": nrhs,
                          "max_iter": max_iter, "slots_per_row": width, "nt": int(Ms[0].get_option("nt")),
                          "degrees": degrees, "us_per_iteration": us, "fewest_iterations_of_a_column": short,
                          CHECK: same}), flush=True)
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
    degrees = [int(v) for v in args.degrees.split(",")]
    A = oracle.generate(n, n, n)
    rows = A.nrow
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(A.row_ptr))
    vals = A.vals.copy()
    vals[r == A.cols] = 26.0
    if args.matrix == "lap26_p2":
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
    same = False
    try:
        assert all(M.get_option("halo_mode") == 1 for M in Ms), "members of the z-slab plan expected"
        Bs, Xs = [], []
        for rp, _, _, st in parts:
            cnt = len(rp) - 1
            Bs.append(torch.from_numpy(b[st:st + cnt].copy()).to(dev).reshape(1, cnt))
            Xs.append(torch.zeros((1, cnt), dtype=torch.float64, device=dev))
        same = checks(hp, torch, Ms, Bs, Xs, 1, degrees, 20)
        r0 = float(hp.group_last_trace_srcg(Ms, 0)[0])
        tol = 1e-10 * r0
        todo = solvers(degrees)

        def run(s):
            for x in Xs:
                x.zero_()
            torch.cuda.synchronize()
            its, nrs, times = solve(hp, s[0], s[1], Ms, Bs, Xs, args.cap, tol)
            return float(times[0]), int(its[0]), float(nrs[0])

        out = {key(s): {"seconds": []} for s in todo}
        if same:
            for s in todo:  # warm-up
                run(s)
            for _ in range(args.reps):
                for s in todo:
                    t, it, nr = run(s)
                    rec = out[key(s)]
                    rec["seconds"].append(t)
                    rec["niters"] = it
                    rec["normr_over_normr0"] = nr / r0
                    rec["reached"] = nr <= tol
                    rec["max_abs_x_minus_xexact"] = max(float((x - 1.0).abs().max()) for x in Xs)
        print(json.dumps({"kind": "time_to_solution", "n": n, "rows": rows, "matrix": args.matrix, "members": P,
                          "planes": planes, "normr0": r0, "tolerance": tol, "degrees": degrees,
                          "a_width": int(Ms[0].get_option("a_width")), "runs": out, CHECK: same}), flush=True)
    finally:
        for M in Ms:
            M.close()
    return 0 if same else 1


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
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
    ap.add_argument("--sizes", default="2:100x100x50:27,8:100x100x13:27",
                    help="members:nx x ny x nz of every member:stencil, run with every --nrhs (empty: none)")
    ap.add_argument("--nrhs", default="1,4")
    ap.add_argument("--sizes-one", default="2:200x200x100:27", help="the same, one column only")
    ap.add_argument("--degrees", default="0,1,2,3,4")
    ap.add_argument("--reps", type=int, default=3, help="alternations inside a process")
    ap.add_argument("--rounds", type=int, default=2, help="processes per configuration")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--tts-n", type=int, default=100, help="0: no time-to-solution runs")
    ap.add_argument("--tts-members", default="2,8")
    ap.add_argument("--cap", type=int, default=2000, help="iteration limit of the time-to-solution runs")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srpoly", "group_srpoly_bench.json"))
    ap.add_argument("--child", choices=["per_iteration", "time_to_solution"])
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--grid", default="100x100x50")
    ap.add_argument("--stencil", type=int, default=27)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--child-nrhs", type=int, default=1)
    ap.add_argument("--matrix", choices=["lap26", "lap26_p2"], default="lap26")
    args = ap.parse_args()
    if args.child == "per_iteration":
        return child_per_iteration(args)
    if args.child == "time_to_solution":
        return child_time_to_solution(args)

    degrees = [int(v) for v in args.degrees.split(",")]
    assert 0 in degrees, "degree 0 is the check against group_HPCCG_srcg"
    common = ["--reps", str(args.reps), "--max-iter", str(args.max_iter), "--cap", str(args.cap), "--degrees",
              args.degrees]
    configs = []
    for sizes, cols in ((args.sizes, [int(v) for v in args.nrhs.split(",")]), (args.sizes_one, [1])):
        for sz in [v for v in sizes.split(",") if v]:
            P, grid, st = sz.split(":")
            for nrhs in cols:
                configs.append(["--child", "per_iteration", "--members", P, "--grid", grid, "--stencil", st,
                                "--child-nrhs", str(nrhs)])
    if args.tts_n > 0:
        for matrix in ("lap26", "lap26_p2"):
            for P in [v for v in args.tts_members.split(",") if v]:
                configs.append(["--child", "time_to_solution", "--n", str(args.tts_n), "--matrix", matrix,
                                "--members", P])
    raw = []
    for rnd in range(args.rounds):
        for cfg in configs:
            rec = spawn(cfg + common, args.child_timeout)
            rec["round"] = rnd
            raw.append(rec)
            print(json.dumps(rec), flush=True)

    names = [key(s) for s in solvers(degrees)]
    per_it, tts = [], []
    for cfg in configs:
        if cfg[1] == "per_iteration":
            P, grid, st, nrhs = int(cfg[3]), [int(v) for v in cfg[5].split("x")], int(cfg[7]), int(cfg[9])
            recs = [r for r in raw if r["kind"] == "per_iteration" and
                    (r["members"], r["grid"], r["stencil"], r["nrhs"]) == (P, grid, st, nrhs)]
            us = {s: summary([v for r in recs for v in r["us_per_iteration"][s]]) for s in names}
            w = recs[0]["slots_per_row"]
            # per process: the ratio of that process's medians (the placement of a process's allocations cancels)
            med = [{s: statistics.median(r["us_per_iteration"][s]) for s in names} for r in recs]
            by_degree = []
            for d in degrees:
                p, q = f"poly_{d}", f"srpoly_{d}"
                by_degree.append({
                    "degree": d, "us_per_iteration": {"poly": us[p], "srpoly": us[q]},
                    "us_per_step": {"poly": us[p]["median"] / (d + 1), "srpoly": us[q]["median"] / (d + 1)},
                    "srpoly_rate_over_group_poly": us[p]["median"] / us[q]["median"],
                    "srpoly_rate_over_group_poly_per_process": [m[p] / m[q] for m in med],
                    "model_ratio": model_ratio(w, nrhs, recs[0]["rows_per_member"], recs[0]["ghost_rows_per_member"],
                                               d) if d else None})
            per_it.append({"members": P, "grid": grid, "stencil": st, "nrhs": nrhs, "slots_per_row": w,
                           "us_per_iteration_group_srcg": us["srcg"],
                           "srpoly_0_rate_over_group_srcg": us["srcg"]["median"] / us["srpoly_0"]["median"],
                           "degrees": by_degree, CHECK: all(r[CHECK] for r in recs)})
        else:
            matrix, P = cfg[5], int(cfg[7])
            recs = [r for r in raw if r["kind"] == "time_to_solution" and (r["matrix"], r["members"]) == (matrix, P)]
            runs = {}
            for name, last in recs[-1]["runs"].items():
                runs[name] = {k: v for k, v in last.items() if k != "seconds"}
                runs[name]["seconds"] = summary([v for r in recs for v in r["runs"][name]["seconds"]])
            best = {s: min((f"{s}_{d}" for d in degrees), key=lambda k: runs[k]["seconds"]["median"])
                    for s in ("poly", "srpoly")}
            tts.append({"n": recs[0]["n"], "matrix": matrix, "members": P, "runs": runs, "best": best,
                        "best_srpoly_speed_over_best_group_poly":
                            runs[best["poly"]]["seconds"]["median"] / runs[best["srpoly"]]["seconds"]["median"],
                        "best_srpoly_speed_over_group_srcg":
                            runs["srcg"]["seconds"]["median"] / runs[best["srpoly"]]["seconds"]["median"],
                        "srpoly_speed_over_group_poly_by_degree":
                            {str(d): runs[f"poly_{d}"]["seconds"]["median"] / runs[f"srpoly_{d}"]["seconds"]["median"]
                             for d in degrees},
                        CHECK: all(r[CHECK] for r in recs)})
    doc = {"per_iteration": per_it, "time_to_solution": tts, "raw": raw}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in per_it + tts if not r[CHECK]]
    bad += [r for t in tts for r in t["runs"].values() if not r["reached"] or r["max_abs_x_minus_xexact"] > 1e-4]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
