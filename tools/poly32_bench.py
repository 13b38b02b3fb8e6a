#!/usr/bin/env python3
"""The polynomial solve with its steps streamed from an fp32 matrix image
(hpccg_hip_poly32_solve_device) beside the fp64 polynomial solve (HPCCG_poly)
and Jacobi PCG (HPCCG_pcg) of the same tree: what a step costs, and what that
does to the time to solution. The driver starts one child process per
configuration and visits the configurations in turn, `--rounds` times (so a
configuration's processes are spread over the run); inside a process the
solvers alternate `--reps` times after a warm-up of each. Reported per
configuration and solver: the median with min and max over every repetition of
every process, and the raw records. Times are the solves' device events.

Every matrix here has an exact fp32 image (the generated stencils; the "lap"
matrices and their power-of-two scalings), so HPCCG_poly32 must be HPCCG_poly
bit for bit: before every timing each degree's x, niters and traces are
compared, and a mismatch ends the run with exit status 1.

1. Per-iteration cost (configuration: stencil, size, columns). HPCCG_pcg,
   HPCCG_poly and HPCCG_poly32 at degrees 0 to 4 on the same device columns,
   max_iter `--max-iter` at tolerance 0; microseconds per iteration. The cost
   of a step is the difference to the library's own degree 0, per degree.
   Beside the measured ratio of the two step costs stands the byte model's:
   the matrix slots, 8 W bytes per row against 4 W, once per launch of R
   columns, plus 48 bytes of vectors per row and column and 8 / R of m.

2. Time to solution (configuration: size, plain or "p2" scaling). The
   27-point n^3 pattern (--lap-n, comma separated) with every diagonal entry
   26.0, plain and with every entry a_ij s_i s_j, s_i = 2^e_i, e_i random in
   [-6, 6]; b = A 1. Iterations and solve time until normr <= 1e-10 normr_0
   for Jacobi PCG, for HPCCG_poly32 at degree 0 (Jacobi PCG with the outer
   SpMM from the fp32 image: what the image alone buys) and for degrees 1 to 4
   of both polynomial libraries at the default eigenvalue ratio 30. Every
   run's final x is checked against xexact = 1 (the record keeps the error; it
   is flagged above 1e-4 or twice Jacobi PCG's own, whichever is larger).

usage: tools/poly32_bench.py [--sizes 27:200,27:100,7:256] [--nrhs 1,4] [--reps 3] [--rounds 2]
                             [--lap-n 100] [--lap-scales plain,p2] [--out profiles/poly32/poly32_bench.json]
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


def step_model_bytes_per_row(width, nrhs, value_bytes):
    """Bytes per row one step moves for all nrhs columns (the docstring's model)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    return launches * (value_bytes * width + 8) + 48 * nrhs


def note(msg):
    print(f"[poly32_bench] {msg}", file=sys.stderr, flush=True)


def solve(hp, M, lib, B, X, **kw):
    f = hp.HPCCG_poly32 if lib == "poly32" else hp.HPCCG_poly
    return f(M, B, X, device=True, **kw)


def traces(M, lib, nrhs):
    f = M.last_trace_poly32 if lib == "poly32" else M.last_trace_poly
    return [f(c).tobytes() for c in range(nrhs)]


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
        info = hp.poly32_info(M)

        def run(solver):
            X.zero_()
            torch.cuda.synchronize()
            if solver == "pcg":
                _, its, _, times = hp.HPCCG_pcg(M, B, X, max_iter=max_iter, tolerance=0.0, device=True)
            else:
                _, its, _, times = solve(hp, M, solver[0], B, X, degree=solver[1], max_iter=max_iter, tolerance=0.0)
            assert all(int(i) == max_iter - 1 for i in its), its
            return 1e6 * float(times[0]) / (max_iter - 1)

        solvers = ["pcg"] + [(lib, d) for d in DEGREES for lib in ("poly", "poly32")]
        for s in solvers:  # warm-up
            run(s)
        same = True
        for d in DEGREES:  # the bitwise check
            run(("poly", d))
            ref = (X.clone(), traces(M, "poly", nrhs))
            run(("poly32", d))
            same = same and bool(torch.equal(X, ref[0])) and traces(M, "poly32", nrhs) == ref[1]
        key = lambda s: s if s == "pcg" else f"{s[0]}_{s[1]}"  # noqa: E731
        us = {key(s): [] for s in solvers}
        for _ in range(args.reps):
            for s in solvers:
                us[key(s)].append(run(s))
        width = int(M.get_option("a_width")) or args.stencil
        print(json.dumps({"kind": "per_iteration", "stencil": args.stencil, "n": n, "rows": rows, "nrhs": nrhs,
                          "max_iter": max_iter, "slots_per_row": width, "us_per_iteration": us, "image": info,
                          "poly32_bitwise_equal_to_poly": same}), flush=True)
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
    t0 = time.perf_counter()
    A = oracle.generate(n, n, n)
    rows = A.nrow
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(A.row_ptr))
    vals = A.vals.copy()
    vals[r == A.cols] = 26.0
    if args.scale == "p2":
        s = 2.0 ** np.random.default_rng(77).integers(-6, 7, rows)
        vals = (vals * s[r]) * s[A.cols.astype(np.int64)]
    note(f"lap {n}^3 {args.scale}: host matrix in {time.perf_counter() - t0:.1f} s")
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, vals)
    note(f"lap {n}^3 {args.scale}: device matrix after {time.perf_counter() - t0:.1f} s")
    del r, vals
    try:
        b = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), b)
        x = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPCCG(M, b, x, max_iter=1, device=True)
        r0 = float(M.last_trace()[0])
        tol = 1e-10 * r0
        lmax = hp.poly_bound(M)
        info = hp.poly32_info(M)
        # (name, library, degree); library None: Jacobi PCG
        # (poly32 at degree 0: Jacobi PCG with the outer SpMM from the fp32 image -- what the image
        # alone buys, without a polynomial)
        runs = [("jacobi", None, None), ("poly32_degree_0", "poly32", 0)] + \
               [(f"{lib}_degree_{d}", lib, d) for d in (1, 2, 3, 4) for lib in ("poly", "poly32")]

        def run(lib, degree):
            x.zero_()
            torch.cuda.synchronize()
            if lib is None:
                _, its, nrs, times = hp.HPCCG_pcg(M, b, x, max_iter=args.cap, tolerance=tol, device=True)
            else:
                _, its, nrs, times = solve(hp, M, lib, b, x, degree=degree, lmin=lmax / 30.0, lmax=lmax,
                                           max_iter=args.cap, tolerance=tol)
            return float(times[0]), int(its[0]), float(nrs[0])

        for _, lib, d in runs:  # warm-up
            run(lib, d)
        same = True
        for d in (1, 2, 3, 4):  # the bitwise check
            ref = run("poly", d)[1:]
            xr, tr = x.clone(), traces(M, "poly", 1)
            got = run("poly32", d)[1:]
            same = same and got == ref and bool(torch.equal(x, xr)) and traces(M, "poly32", 1) == tr
        out = {name: {"library": lib, "degree": d, "seconds": []} for name, lib, d in runs}
        for _ in range(args.reps):
            for name, lib, d in runs:
                t, it, nr = run(lib, d)
                rec = out[name]
                rec["seconds"].append(t)
                rec["niters"] = it
                rec["spmvs"] = it * ((d or 0) + 1)
                rec["normr_over_normr0"] = nr / r0
                rec["reached"] = nr <= tol
                rec["max_abs_x_minus_xexact"] = float((x - 1.0).abs().max())
        print(json.dumps({"kind": "time_to_solution", "n": n, "rows": rows, "scale": args.scale, "normr0": r0,
                          "tolerance": tol, "lmax": lmax, "a_width": int(M.get_option("a_width")), "image": info,
                          "poly32_bitwise_equal_to_poly": same, "runs": out}), flush=True)
    finally:
        M.close()
    return 0


# ---------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------
def spawn(extra, timeout):
    """One child process; its JSON record (the last line it prints)."""
    cmd = [sys.executable, os.path.abspath(__file__)] + extra
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=timeout)  # (its notes go to our stderr)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:])
        raise SystemExit(f"child {' '.join(extra)} ended with status {p.returncode}: nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="27:200,27:100,7:256", help="stencil:n, comma separated (empty: none)")
    ap.add_argument("--nrhs", default="1,4")
    ap.add_argument("--reps", type=int, default=3, help="alternations inside a process")
    ap.add_argument("--rounds", type=int, default=2, help="processes per configuration")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--lap-n", default="100", help="sizes of the time-to-solution runs, comma separated (empty: none)")
    ap.add_argument("--lap-scales", default="plain,p2")
    ap.add_argument("--cap", type=int, default=2000, help="iteration limit of the time-to-solution runs")
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly32", "poly32_bench.json"))
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
    for n in [int(v) for v in args.lap_n.split(",") if v]:
        for scale in [v for v in args.lap_scales.split(",") if v]:
            configs.append(["--child", "time_to_solution", "--n", str(n), "--scale", scale])
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
            step = {lib: {str(d): (us[f"{lib}_{d}"]["median"] - us[f"{lib}_0"]["median"]) / d for d in DEGREES if d}
                    for lib in ("poly", "poly32")}
            m64, m32 = step_model_bytes_per_row(w, nrhs, 8), step_model_bytes_per_row(w, nrhs, 4)
            per_it.append({"stencil": st, "n": n, "nrhs": nrhs, "slots_per_row": w, "us_per_iteration": us,
                           "us_per_step": step,
                           "step_ratio_poly32_over_poly": {d: step["poly32"][d] / step["poly"][d] for d in step["poly"]},
                           "iteration_ratio_poly32_over_poly": {str(d): us[f"poly32_{d}"]["median"] /
                                                                us[f"poly_{d}"]["median"] for d in DEGREES},
                           "step_model_bytes_per_row": {"poly": m64, "poly32": m32, "ratio": m32 / m64},
                           "image": recs[0]["image"],
                           "poly32_bitwise_equal_to_poly": all(r["poly32_bitwise_equal_to_poly"] for r in recs)})
        else:
            n, scale = int(cfg[3]), cfg[5]
            recs = [r for r in raw if r["kind"] == "time_to_solution" and (r["n"], r["scale"]) == (n, scale)]
            runs = {}
            for name, last in recs[-1]["runs"].items():
                runs[name] = {k: v for k, v in last.items() if k != "seconds"}
                runs[name]["seconds"] = summary([v for r in recs for v in r["runs"][name]["seconds"]])
            tts.append({"n": n, "scale": scale, "lmax": recs[0]["lmax"], "image": recs[0]["image"], "runs": runs,
                        "poly32_bitwise_equal_to_poly": all(r["poly32_bitwise_equal_to_poly"] for r in recs)})
    doc = {"per_iteration": per_it, "time_to_solution": tts, "raw": raw}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in per_it + tts if not r["poly32_bitwise_equal_to_poly"]]
    for t in tts:
        limit = max(1e-4, 2.0 * t["runs"]["jacobi"]["max_abs_x_minus_xexact"])
        bad += [r for r in t["runs"].values() if not r["reached"] or r["max_abs_x_minus_xexact"] > limit]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
