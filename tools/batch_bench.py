#!/usr/bin/env python3
"""Batched multi-right-hand-side CG against the same columns solved one after
the other, on one matrix in one process (same allocations, so the per-process
placement spread does not enter).

Per size and column count: the batch (hpccg_hip_batch_solve_device) and the
baseline (nrhs sequential hpccg_hip_solve_device calls) both run max_iter 500
at tolerance 0 on the same device columns; after a warm-up of each, the two
alternate `--reps` times. Reported: RHS-iterations per second (median, min,
max), their ratio, and the byte model's prediction (bytes per row
per column per iteration, batch 88 + 8 W / R against 64 + 8 W for the single
solve; W slots per row, R columns per SpMM launch). The batch's x and residual
traces are compared bitwise with the sequential solves' at the timed size; a
mismatch ends the run with exit status 1.

usage: tools/batch_bench.py [--sizes 27:200,27:100,7:256] [--nrhs 1,2,4,8]
                            [--reps 5] [--out profiles/batch/batch_bench.json]
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

MAX_R = 4  # columns per SpMM launch (the widest instantiation)


def model_ratio(width, nrhs):
    """Predicted batch / sequential rate from the byte model."""
    if nrhs == 1:
        return 1.0  # forwarded to the single solve
    launches = (nrhs + MAX_R - 1) // MAX_R if nrhs > 2 else 1
    passes_per_col = launches / nrhs  # matrix passes per column and iteration
    return (64 + 8 * width) / (88 + 8 * width * passes_per_col)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_size(hp, torch, stencil, n, nrhs_list, reps, max_iter):
    dev = torch.device("cuda:0")
    M = hp.Matrix.generate(n, n, n, use_7pt=stencil == 7)
    rows = n ** 3
    out = []
    try:
        kmax = max(nrhs_list)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        B = torch.rand((kmax, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        # column 0: the generated right-hand side (b = A 1, exact: bitwise the generator's)
        hp.HPC_sparsemv(M, torch.ones(rows, dtype=torch.float64, device=dev), B[0])
        for nrhs in nrhs_list:
            Xs = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)
            Xb = torch.zeros((nrhs, rows), dtype=torch.float64, device=dev)
            seq_tr, seq_it = [None] * nrhs, [0] * nrhs

            def sequential():
                Xs.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in range(nrhs):
                    _, it, _, _ = hp.HPCCG(M, B[c], Xs[c], max_iter=max_iter, tolerance=0.0, device=True)
                    seq_it[c] = it
                    seq_tr[c] = M.last_trace().tobytes()
                return sum(seq_it) / (time.perf_counter() - t0)

            def batch():
                Xb.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, its, _, _ = hp.HPCCG_batch(M, B[:nrhs], Xb, max_iter=max_iter, tolerance=0.0, device=True)
                return int(its.sum()) / (time.perf_counter() - t0), its

            sequential()  # warm-up of both paths (graph capture, workspace growth)
            batch()
            rs, rb = [], []
            for _ in range(reps):
                rs.append(sequential())
                r, its = batch()
                rb.append(r)
            same = all(int(its[c]) == seq_it[c] and M.last_trace_batch(c).tobytes() == seq_tr[c]
                       for c in range(nrhs)) and bool(torch.equal(Xb, Xs))
            width = int(M.get_option("a_width")) or stencil
            rec = {"stencil": stencil, "n": n, "rows": rows, "nrhs": nrhs, "max_iter": max_iter, "reps": reps,
                   "iters_per_column": seq_it[0],
                   "batch_rhs_it_per_s": summary(rb), "sequential_rhs_it_per_s": summary(rs),
                   "ratio_of_medians": statistics.median(rb) / statistics.median(rs),
                   "model_ratio": model_ratio(width, nrhs), "slots_per_row": width,
                   "bitwise_equal": same}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            M.batch_release()
    finally:
        M.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="27:200,27:100,7:256", help="stencil:n, comma separated")
    ap.add_argument("--nrhs", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "batch_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5 alternations")
    import torch
    hp = load_pkg()
    hp.set_device(0)
    recs = []
    for sz in args.sizes.split(","):
        st, n = (int(v) for v in sz.split(":"))
        recs += run_size(hp, torch, st, n, [int(v) for v in args.nrhs.split(",")], args.reps, args.max_iter)
    doc = {"device": hp.device_name()[0], "results": recs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in recs if not r["bitwise_equal"]]
    for r in bad:
        print(f"MISMATCH: {r['stencil']}-pt {r['n']}^3 nrhs {r['nrhs']}: the batch is not bitwise the sequential "
              "solves", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
