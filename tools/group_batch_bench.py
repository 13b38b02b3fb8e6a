#!/usr/bin/env python3
"""Batched multi-right-hand-side CG over an in-process rank group against the
same columns solved one after the other by the group solve, on the same members
in one process (same allocations, so the per-process placement spread does not
enter).

The group: --members z-slab ranks of a local nx x ny x nz grid, all on one GPU
(default 2 x 200x200x100, 27-point). The batch
(hpccg_hip_group_batch_solve_device) and the baseline (nrhs sequential
hpccg_hip_group_solve calls) both run max_iter 500 at tolerance 0 on the same
device columns; after a warm-up of each, the two alternate `--reps` times.
Reported: RHS-iterations per second both ways (median, min, max) and their
ratio. Every member's x, niters and the residual trace of every column of the
batch are compared bitwise with the sequential solves'; a mismatch ends the run
with exit status 1.

usage: tools/group_batch_bench.py [--members 2] [--grid 200x200x100] [--stencil 27] [--nrhs 4]
                                  [--reps 5] [--out profiles/batch/group_batch_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_pkg  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(hp, torch, P, grid, stencil, nrhs, reps, max_iter):
    dev = torch.device("cuda:0")
    nx, ny, nz = grid
    Ms = hp.group_generate(nx, ny, nz, P, use_7pt=stencil == 7)
    rows = nx * ny * nz
    try:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        Bs = [torch.rand((nrhs, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0 for _ in Ms]
        # column 0: b = A 1 by the group SpMM (small integers: exact)
        ones = [torch.ones((1, rows), dtype=torch.float64, device=dev) for _ in Ms]
        hp.group_sparsemv_batch(Ms, ones, [b[:1] for b in Bs])
        Xs = [torch.zeros((nrhs, rows), dtype=torch.float64, device=dev) for _ in Ms]
        Xb = [torch.zeros((nrhs, rows), dtype=torch.float64, device=dev) for _ in Ms]
        seq_tr, seq_it = [None] * nrhs, [0] * nrhs

        def sequential():
            for x in Xs:
                x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c in range(nrhs):
                _, it, _, _ = hp.group_HPCCG(Ms, [b[c] for b in Bs], [x[c] for x in Xs], max_iter=max_iter,
                                             tolerance=0.0)
                seq_it[c] = it
                seq_tr[c] = Ms[0].last_trace().tobytes()
            return sum(seq_it) / (time.perf_counter() - t0)

        def batch():
            for x in Xb:
                x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its, _, _ = hp.group_HPCCG_batch(Ms, Bs, Xb, max_iter=max_iter, tolerance=0.0)
            return int(its.sum()) / (time.perf_counter() - t0), its

        sequential()  # warm-up of both paths (graph capture, workspace growth)
        batch()
        rs, rb = [], []
        for _ in range(reps):
            rs.append(sequential())
            r, its = batch()
            rb.append(r)
        same = all(int(its[c]) == seq_it[c] and hp.group_last_trace_batch(Ms, c).tobytes() == seq_tr[c]
                   for c in range(nrhs)) and all(bool(torch.equal(a, b)) for a, b in zip(Xb, Xs))
        rec = {"members": P, "grid": [nx, ny, nz], "stencil": stencil, "rows_per_member": rows, "nrhs": nrhs,
               "max_iter": max_iter, "reps": reps, "iters_per_column": seq_it[0],
               "batch_rhs_it_per_s": summary(rb), "sequential_rhs_it_per_s": summary(rs),
               "ratio_of_medians": statistics.median(rb) / statistics.median(rs),
               "batch_workspace_bytes": [M.batch_workspace_bytes() for M in Ms], "bitwise_equal": same}
        print(json.dumps(rec), flush=True)
        return rec
    finally:
        for M in Ms:
            M.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--grid", default="200x200x100", help="every member's local nx x ny x nz")
    ap.add_argument("--stencil", type=int, default=27, choices=(27, 7))
    ap.add_argument("--nrhs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "group_batch_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5 alternations")
    if args.nrhs < 2 or args.members < 2:
        ap.error("at least two members and two columns (one of either is forwarded to another path)")
    import torch
    hp = load_pkg()
    hp.set_device(0)
    grid = tuple(int(v) for v in args.grid.split("x"))
    rec = run(hp, torch, args.members, grid, args.stencil, args.nrhs, args.reps, args.max_iter)
    doc = {"device": hp.device_name()[0], "results": [rec]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not rec["bitwise_equal"]:
        print("MISMATCH: the group batch is not bitwise the sequential group solves", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
