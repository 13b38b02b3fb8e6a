#!/usr/bin/env python3
"""BiCGStab (hpccg_hip_bicgstab_solve_device) against the preconditioned CG
(hpccg_hip_pcg_solve_device): what an iteration of the non-symmetric solver
costs beside CG's on the same matrix images and SpMM loops, and what it buys
where CG does not converge. The driver starts one child process per
configuration and visits the configurations in turn, `--rounds` times; inside a
process the two solvers alternate `--reps` times on the same matrix and vectors
after a warm-up of each. Reported per configuration and solver: the median with
min and max over every repetition of every process, the ratio of the medians
per process, and the raw records. No ratio is required: the run fails on a
wrong result only.

Before any timing every child makes the bitwise check of the tests
(tests/test_gpu_bicgstab.py, 2.): HPCCG_bicgstab with m = 2^-3 everywhere
against m = 1 (x, niters, normr, traces); a mismatch ends the run with exit
status 1.

1. Per-iteration cost (configuration: stencil, size, columns). Both solvers
   with Jacobi on the same device columns, max_iter `--max-iter` at tolerance
   0; microseconds per iteration from the solve's device events. Beside the
   measured ratio stands the byte model's (bytes per row and
   iteration for R columns of one launch, 8 W + 16 + 88 R for CG and
   16 W + 24 + 176 R for BiCGStab; W slots per row). Where the measured rate is
   below 0.85 of the model's, tools/bicgstab_profile.py under a kernel trace
   names the kernel.

2. Time to solution (configuration: eps). The 27-point n^3 stencil (--tts-n,
   default 100) with off-diagonals -1 + eps sign(j - i), eps 0.25 and 0.5;
   b = A 1. BiCGStab: iterations and wall time until normr <= 1e-10 normr_0,
   the final x checked against xexact = 1. CG on the same matrix, `--cg-cap`
   iterations: where it ends (it does not get there), recorded beside.

usage: tools/bicgstab_bench.py [--sizes 27:200,27:100,7:256] [--nrhs 1,4] [--reps 3] [--rounds 2]
                               [--tts-n 100] [--out profiles/bicgstab/bicgstab_bench.json]
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
SOLVERS = ("pcg", "bicgstab")


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "count": len(v)}


def model_ratio(width, nrhs):
    """Predicted bicgstab / pcg time per iteration from the byte model (the docstring's)."""
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    return (launches * (16 * width + 24) + 176 * nrhs) / (launches * (8 * width + 16) + 88 * nrhs)


def solver_of(hp, name):
    return hp.HPCCG_pcg if name == "pcg" else hp.HPCCG_bicgstab


def uniform_m_is_bitwise(hp, torch, M, B, X, max_iter=4):
    """HPCCG_bicgstab with m = 2^-3 against m = 1: x, niters, normr and traces, bit for bit."""
    rows = B.shape[-1]
    nrhs = 1 if B.dim() == 1 else B.shape[0]
    got = []
    for m in (1.0, 2.0 ** -3):
        X.zero_()
        mv = torch.full((rows,), m, dtype=torch.float64, device=B.device)
        _, its, nrs, _ = hp.HPCCG_bicgstab(M, B, X, max_iter=max_iter, tolerance=0.0, minv=mv, device=True)
        got.append((X.clone(), its.tobytes(), nrs.tobytes(), [M.last_trace_bicgstab(c).tobytes() for c in range(nrhs)]))
    return bool(torch.equal(got[0][0], got[1][0])) and got[0][1:] == got[1][1:]


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
        same = uniform_m_is_bitwise(hp, torch, M, B, X)

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
                          "us_per_iteration": us, "uniform_m_bitwise": same}), flush=True)
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
    c = A.cols.astype(np.int64)
    vals = np.where(r == c, A.vals, -1.0 + args.eps * np.sign(c - r))
    M = hp.Matrix.from_csr(A.row_ptr, A.cols, vals)
    del r, c, vals
    try:
        b = torch.zeros(rows, dtype=torch.float64, device=dev)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), b)
        x = torch.zeros(rows, dtype=torch.float64, device=dev)
        same = uniform_m_is_bitwise(hp, torch, M, b, x)
        x.zero_()
        hp.HPCCG_bicgstab(M, b, x, max_iter=1, device=True)
        r0 = float(M.last_trace_bicgstab(0)[0])
        tol = 1e-10 * r0

        def run(name):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cap = args.cap if name == "bicgstab" else args.cg_cap
            _, its, nrs, _ = solver_of(hp, name)(M, b, x, max_iter=cap, tolerance=tol, device=True)
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
        out["bicgstab"]["status"] = M.last_status_bicgstab(0)
        print(json.dumps({"kind": "time_to_solution", "n": n, "rows": rows, "eps": args.eps, "normr0": r0,
                          "tolerance": tol, "a_width": int(M.get_option("a_width")), "runs": out,
                          "uniform_m_bitwise": same}), flush=True)
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
    ap.add_argument("--max-iter", type=int, default=50,
                    help="iterations timed (few enough that no column ends first: 7-pt 256^3 reaches r.r = 0 at 89)")
    ap.add_argument("--tts-n", type=int, default=100, help="0: no time-to-solution runs")
    ap.add_argument("--tts-eps", default="0.25,0.5")
    ap.add_argument("--cap", type=int, default=2000, help="BiCGStab's iteration limit in the time-to-solution runs")
    ap.add_argument("--cg-cap", type=int, default=300, help="CG's iteration limit there")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicgstab", "bicgstab_bench.json"))
    ap.add_argument("--child", choices=["per_iteration", "time_to_solution"])
    ap.add_argument("--stencil", type=int, default=27)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--child-nrhs", type=int, default=1)
    ap.add_argument("--eps", type=float, default=0.25)
    args = ap.parse_args()
    if args.child == "per_iteration":
        return child_per_iteration(args)
    if args.child == "time_to_solution":
        return child_time_to_solution(args)

    common = ["--reps", str(args.reps), "--max-iter", str(args.max_iter), "--cap", str(args.cap), "--cg-cap",
              str(args.cg_cap)]
    configs = []
    for sz in [v for v in args.sizes.split(",") if v]:
        st, n = (int(v) for v in sz.split(":"))
        for nrhs in [int(v) for v in args.nrhs.split(",")]:
            configs.append(["--child", "per_iteration", "--stencil", str(st), "--n", str(n), "--child-nrhs", str(nrhs)])
    if args.tts_n > 0:
        for eps in [v for v in args.tts_eps.split(",") if v]:
            configs.append(["--child", "time_to_solution", "--n", str(args.tts_n), "--eps", eps])
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
            per_proc = [statistics.median(r["us_per_iteration"]["bicgstab"]) / statistics.median(r["us_per_iteration"]["pcg"])
                        for r in recs]
            ratio = us["bicgstab"]["median"] / us["pcg"]["median"]
            model = model_ratio(w, nrhs)
            per_it.append({"stencil": st, "n": n, "nrhs": nrhs, "slots_per_row": w, "us_per_iteration": us,
                           "bicgstab_time_over_pcg": ratio, "bicgstab_time_over_pcg_per_process": per_proc,
                           "model_ratio": model, "rate_over_model": model / ratio,
                           "uniform_m_bitwise": all(r["uniform_m_bitwise"] for r in recs)})
        else:
            eps = float(cfg[5])
            recs = [r for r in raw if r["kind"] == "time_to_solution" and r["eps"] == eps]
            runs = {}
            for name, last in recs[-1]["runs"].items():
                runs[name] = {k: v for k, v in last.items() if k != "seconds"}
                runs[name]["seconds"] = summary([v for r in recs for v in r["runs"][name]["seconds"]])
            tts.append({"n": recs[0]["n"], "eps": eps, "runs": runs,
                        "uniform_m_bitwise": all(r["uniform_m_bitwise"] for r in recs)})
    doc = {"per_iteration": per_it, "time_to_solution": tts, "raw": raw}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in per_it:
        print(f"{r['stencil']}-pt {r['n']}^3 x{r['nrhs']}: pcg {r['us_per_iteration']['pcg']['median']:.1f} us, bicgstab "
              f"{r['us_per_iteration']['bicgstab']['median']:.1f} us per iteration, ratio {r['bicgstab_time_over_pcg']:.3f} "
              f"(per process {['%.3f' % v for v in r['bicgstab_time_over_pcg_per_process']]}), model {r['model_ratio']:.3f}, "
              f"rate over model {r['rate_over_model']:.3f}")
    for t in tts:
        bi, cg = t["runs"]["bicgstab"], t["runs"]["pcg"]
        print(f"convect {t['n']}^3 eps {t['eps']}: bicgstab {bi['niters']} iterations, {bi['seconds']['median']:.4f} s, "
              f"normr/normr0 {bi['normr_over_normr0']:.3e}, max |x - 1| {bi['max_abs_x_minus_xexact']:.3e}; pcg "
              f"{cg['niters']} iterations, normr/normr0 {cg['normr_over_normr0']:.3e}")
    bad = [r for r in per_it + tts if not r["uniform_m_bitwise"]]
    bad += [t for t in tts if not t["runs"]["bicgstab"]["reached"] or t["runs"]["bicgstab"]["max_abs_x_minus_xexact"] > 1e-4]
    for r in bad:
        print(f"CHECK FAILED: {json.dumps(r)}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
