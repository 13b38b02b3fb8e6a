#!/usr/bin/env python3
"""Chebyshev polynomial preconditioned CG over an in-process rank group with the
polynomial steps streamed from the members' fp32 images
(hpccg_hip_group_poly32_solve_device) against its two parents on the same
members: the fp64 group polynomial (hpccg_hip_group_poly_solve_device) and the
group Jacobi solve (hpccg_hip_group_pcg_solve_device). All members on one GPU.
The driver starts one child process per configuration, one after another, and
visits the configurations in turn `--rounds` times; inside a process the solvers
alternate `--reps` times after a warm-up of each. Times are the solves' own
(device events on member 0's stream). Reported per configuration and solver:
the median with min and max over every repetition of every process, and the raw
records.

Every child checks bits before it times anything, on its own members: degree 0
of group_HPCCG_poly32 against group_HPCCG_pcg, and (the generated stencil's
images are exact) degrees 1 to 4 against group_HPCCG_poly -- every member's x
and every trace. A mismatch ends the run with exit status 1.

1. Per-iteration cost (configuration: members x local grid, columns).
   group_HPCCG_pcg with Jacobi, group_HPCCG_poly and group_HPCCG_poly32 at
   degrees 0 to 4 on the same device columns, max_iter `--max-iter` at tolerance
   0; microseconds per iteration. The cost of a step is the difference to the
   same library's degree 0 per degree: it includes the step's halo of z. The
   step ratio is the fp32 step over the fp64 step. Beside it the byte model of
   one step per row for all columns: launches * (V W + 8) + 48 nrhs bytes
   (tools/poly_bench.py; V = 8 or 4 bytes per stored slot) plus the ghost planes
   the halo moves, 16 bytes per ghost row and column.

2. Time to solution (configuration: members). The 27-point n^3 pattern
   (--lap-n) with every diagonal entry 26.0 (its fp32 image is exact, so the
   outer SpMM of group_HPCCG_poly32 streams it too), split into z-slabs; b = A 1,
   one column. Iterations, SpMVs and milliseconds until normr <= 1e-10 normr_0
   for group_HPCCG_pcg, for group_HPCCG_poly32 at degree 0 (the same Jacobi
   recurrence with the outer SpMM from the images) and for both polynomial
   libraries at degrees 1 to 4 at the default interval. Every run's final x is
   checked against xexact = 1.

usage: tools/group_poly32_bench.py [--sizes 2:200x200x100,2:100x100x50] [--nrhs 1,4] [--reps 3] [--rounds 2]
                                   [--lap-n 100] [--lap-members 2,8]
                                   [--out profiles/group_poly32/group_poly32_bench.json]
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


def step_model_bytes_per_row(value_bytes, width, nrhs, rows, ghost_rows):
    """Bytes per row one step moves for all nrhs columns (the docstring's model)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    return launches * (value_bytes * width + 8) + 48 * nrhs + 16.0 * nrhs * ghost_rows / rows


def solve(hp, lib, Ms, Bs, Xs, degree, max_iter, tol):
    """(niters, normr, times) of one solve from x = 0; lib: "pcg", "p64" or "p32"."""
    import torch
    for x in Xs:
        x.zero_()
    torch.cuda.synchronize()
    if lib == "pcg":
        return hp.group_HPCCG_pcg(Ms, Bs, Xs, max_iter=max_iter, tolerance=tol)
    f = hp.group_HPCCG_poly if lib == "p64" else hp.group_HPCCG_poly32
    return f(Ms, Bs, Xs, degree=degree, max_iter=max_iter, tolerance=tol)


def traces(hp, lib, Ms, nrhs):
    f = {"pcg": hp.group_last_trace_pcg, "p64": hp.group_last_trace_poly, "p32": hp.group_last_trace_poly32}[lib]
    return [f(Ms, c).tobytes() for c in range(nrhs)]


def bitwise_checks(hp, Ms, Bs, Xs, nrhs, max_iter, exact):
    """Degree 0 against the group pcg; on exact images degrees 1 to 4 against the fp64 group polynomial."""
    import torch
    pairs = [(("pcg", None), ("p32", 0))]
    if exact:
        pairs += [(("p64", d), ("p32", d)) for d in DEGREES if d]
    for (la, da), (lb, db) in pairs:
        solve(hp, la, Ms, Bs, Xs, da, max_iter, 0.0)
        ref = ([x.clone() for x in Xs], traces(hp, la, Ms, nrhs))
        solve(hp, lb, Ms, Bs, Xs, db, max_iter, 0.0)
        if not (all(bool(torch.equal(a, b)) for a, b in zip(Xs, ref[0])) and traces(hp, lb, Ms, nrhs) == ref[1]):
            return False
    return True


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
        info = hp.group_poly32_info(Ms)
        exact = all(i["exact"] for i in info)

        def run(lib, degree):
            its, _, times = solve(hp, lib, Ms, Bs, Xs, degree, max_iter, 0.0)
            assert all(int(i) == max_iter - 1 for i in its), its
            return 1e6 * float(times[0]) / (max_iter - 1)

        same = exact and bitwise_checks(hp, Ms, Bs, Xs, nrhs, min(max_iter, 25), exact)
        solvers = [("pcg", None)] + [(lib, d) for d in DEGREES for lib in ("p64", "p32")]
        us = {f"{lib}_{d}" if d is not None else lib: [] for lib, d in solvers}
        if same:
            for lib, d in solvers:  # warm-up
                run(lib, d)
            for _ in range(args.reps):
                for lib, d in solvers:
                    us[f"{lib}_{d}" if d is not None else lib].append(run(lib, d))
        width = int(Ms[0].get_option("a_width")) or 27
        print(json.dumps({"kind": "per_iteration", "members": P, "grid": [nx, ny, nz], "rows_per_member": rows,
                          "ghost_rows_per_member": 2.0 * nx * ny * (P - 1) / P, "nrhs": nrhs, "max_iter": max_iter,
                          "slots_per_row": width, "us_per_iteration": us,
                          "image_bytes_per_member": [i["image_bytes"] for i in info],
                          "spectrum": list(hp.group_last_spectrum_poly32(Ms)),
                          "bitwise_equal_to_the_parents": same}), flush=True)
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
        info = hp.group_poly32_info(Ms)
        exact = all(i["exact"] for i in info)
        same = bitwise_checks(hp, Ms, Bs, Xs, 1, 25, exact)
        # (p32 at degree 0: the group Jacobi solve with its outer SpMM from the exact images)
        runs = [("jacobi", "pcg", None), ("p32_degree_0", "p32", 0)]
        runs += [(f"{lib}_degree_{d}", lib, d) for d in (1, 2, 3, 4) for lib in ("p64", "p32")]

        def run(lib, degree):
            its, nrs, times = solve(hp, lib, Ms, Bs, Xs, degree, args.cap, tol)
            return float(times[0]), int(its[0]), float(nrs[0])

        out = {name: {"library": lib, "degree": d, "seconds": []} for name, lib, d in runs}
        if same:
            for _, lib, d in runs:  # warm-up
                run(lib, d)
            for _ in range(args.reps):
                for name, lib, d in runs:
                    t, it, nr = run(lib, d)
                    rec = out[name]
                    rec["seconds"].append(t)
                    rec["niters"] = it
                    rec["spmvs"] = it * ((d or 0) + 1)
                    rec["normr_over_normr0"] = nr / r0
                    rec["reached"] = nr <= tol
                    rec["max_abs_x_minus_xexact"] = max(float((x - 1.0).abs().max()) for x in Xs)
        print(json.dumps({"kind": "time_to_solution", "n": n, "rows": rows, "members": P, "planes": planes,
                          "normr0": r0, "tolerance": tol, "lmax": hp.group_poly32_bound(Ms),
                          "a_width": int(Ms[0].get_option("a_width")), "images_exact": exact,
                          "bitwise_equal_to_the_parents": same, "runs": out}), flush=True)
    finally:
        for M in Ms:
            M.close()
    return 0 if same else 1


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_poly32", "group_poly32_bench.json"))
    ap.add_argument("--child", choices=["per_iteration", "time_to_solution"])
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--grid", default="100x100x50")
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--child-nrhs", type=int, default=1)
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
        for P in [v for v in args.lap_members.split(",") if v]:
            configs.append(["--child", "time_to_solution", "--n", str(args.lap_n), "--members", P])
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
            pcg = us["pcg"]["median"]
            step = {lib: {str(d): (us[f"{lib}_{d}"]["median"] - us[f"{lib}_0"]["median"]) / d for d in DEGREES if d}
                    for lib in ("p64", "p32")}
            model = {lib: step_model_bytes_per_row(vb, w, nrhs, recs[0]["rows_per_member"],
                                                   recs[0]["ghost_rows_per_member"])
                     for lib, vb in (("p64", 8), ("p32", 4))}
            per_it.append({"members": P, "grid": grid, "nrhs": nrhs, "slots_per_row": w, "us_per_iteration": us,
                           "us_per_step": step,
                           "step_ratio_fp32_over_fp64": {d: step["p32"][d] / step["p64"][d] for d in step["p64"]},
                           "iteration_ratio_fp32_over_fp64": {str(d): us[f"p32_{d}"]["median"] / us[f"p64_{d}"]["median"]
                                                              for d in DEGREES},
                           "iteration_over_group_pcg": {s: v["median"] / pcg for s, v in us.items()},
                           "step_model_bytes_per_row": model,
                           "step_model_ratio": model["p32"] / model["p64"],
                           "bitwise_equal_to_the_parents": all(r["bitwise_equal_to_the_parents"] for r in recs)})
        else:
            P = int(cfg[5])
            recs = [r for r in raw if r["kind"] == "time_to_solution" and r["members"] == P]
            runs = {}
            for name, last in recs[-1]["runs"].items():
                runs[name] = {k: v for k, v in last.items() if k != "seconds"}
                runs[name]["seconds"] = summary([v for r in recs for v in r["runs"][name]["seconds"]])
            jac = runs["jacobi"]["seconds"]["median"]
            for name, v in runs.items():
                v["seconds_over_jacobi"] = v["seconds"]["median"] / jac
                if name.startswith("p32_") and "p64_" + name[4:] in runs:
                    v["seconds_over_fp64_polynomial"] = v["seconds"]["median"] / \
                        runs["p64_" + name[4:]]["seconds"]["median"]
            tts.append({"n": recs[0]["n"], "members": P, "lmax": recs[0]["lmax"], "images_exact": recs[0]["images_exact"],
                        "bitwise_equal_to_the_parents": all(r["bitwise_equal_to_the_parents"] for r in recs),
                        "runs": runs})
    doc = {"per_iteration": per_it, "time_to_solution": tts, "raw": raw}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in per_it + tts if not r["bitwise_equal_to_the_parents"]]
    bad += [r for t in tts for r in t["runs"].values() if not r["reached"] or r["max_abs_x_minus_xexact"] > 1e-4]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
