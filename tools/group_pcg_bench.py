#!/usr/bin/env python3
"""Diagonally preconditioned CG over an in-process rank group
(hpccg_hip_group_pcg_solve_device): what it costs per iteration against the
group batch, and what the halo kernel buys against the halo by copies. One group
per size in one process (same allocations, so the per-process placement spread
does not enter), all members on one GPU.

Per size (--sizes, members x the local grid of every member, 27-point) and
column count, three runs on the same device columns, max_iter 500 at
tolerance 0:
  (a) group_HPCCG_pcg with Jacobi, the halo by k_pcg_group_halo (one launch per
      member and iteration);
  (b) the same with the halo by copies (halo_copies=True: one copy per column
      and side, the group batch's way);
  (c) group_HPCCG_batch (one column: the group solve it forwards to).
After a warm-up of each, the three alternate `--reps` times. Reported:
RHS-iterations per second (median, min, max), the ratios a/c and a/b of the
medians with the smallest and the largest ratio of one alternation, and the
byte model's a/c (tools/pcg_bench.py: 88 + (8 W + 16) / R against 88 + 8 W / R
bytes per row, column and iteration). Before the timing, (a) with m = 1 is
compared bitwise with (c) -- every member's x, niters and the traces; a mismatch
ends the run with exit status 1.

usage: tools/group_pcg_bench.py [--sizes 2:200x200x100,2:100x100x50] [--nrhs 4,1] [--reps 5]
                                [--out profiles/pcg/group_pcg_bench.json]
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
from pcg_bench import model_ratio  # noqa: E402  (tools/ is the script's directory)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def ratios(num, den):
    r = [a / b for a, b in zip(num, den)]
    return {"of_medians": statistics.median(num) / statistics.median(den), "min": min(r), "max": max(r)}


def run_size(hp, torch, P, grid, nrhs_list, reps, max_iter):
    dev = torch.device("cuda:0")
    nx, ny, nz = grid
    Ms = hp.group_generate(nx, ny, nz, P)
    rows = nx * ny * nz
    out = []
    try:
        kmax = max(max(nrhs_list), 2)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        Bs = [torch.rand((kmax, rows), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0 for _ in Ms]
        # column 0: b = A 1 by the group SpMM (small integers: exact)
        one2 = [torch.ones((2, rows), dtype=torch.float64, device=dev) for _ in Ms]
        y2 = [torch.zeros((2, rows), dtype=torch.float64, device=dev) for _ in Ms]
        hp.group_sparsemv_batch(Ms, one2, y2)
        for b, y in zip(Bs, y2):
            b[0].copy_(y[0])
        ones = [torch.ones(rows, dtype=torch.float64, device=dev) for _ in Ms]
        for nrhs in nrhs_list:
            Bn = [b[:nrhs] for b in Bs]
            Xp = [torch.zeros((nrhs, rows), dtype=torch.float64, device=dev) for _ in Ms]
            Xb = [torch.zeros((nrhs, rows), dtype=torch.float64, device=dev) for _ in Ms]

            def batch():
                for x in Xb:
                    x.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                its, _, _ = hp.group_HPCCG_batch(Ms, Bn, Xb, max_iter=max_iter, tolerance=0.0)
                return int(its.sum()) / (time.perf_counter() - t0), its

            def pcg(minvs=None, copies=False):
                for x in Xp:
                    x.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                its, _, _ = hp.group_HPCCG_pcg(Ms, Bn, Xp, max_iter=max_iter, tolerance=0.0, minvs=minvs,
                                               halo_copies=copies)
                return int(its.sum()) / (time.perf_counter() - t0), its

            # warm-up of the three paths, and the bitwise check: m = 1 is the group batch
            _, itb = batch()
            trb = [hp.group_last_trace_batch(Ms, c).tobytes() for c in range(nrhs)]
            _, itp = pcg(ones)
            same = all(int(itp[c]) == int(itb[c]) and hp.group_last_trace_pcg(Ms, c).tobytes() == trb[c]
                       for c in range(nrhs)) and all(bool(torch.equal(a, b)) for a, b in zip(Xp, Xb))
            pcg()
            pcg(copies=True)
            ra, rb, rc = [], [], []
            for _ in range(reps):
                rc.append(batch()[0])
                r, its = pcg()
                ra.append(r)
                rb.append(pcg(copies=True)[0])
            width = int(Ms[0].get_option("a_width")) or 27
            rec = {"members": P, "grid": [nx, ny, nz], "stencil": 27, "rows_per_member": rows, "nrhs": nrhs,
                   "max_iter": max_iter, "reps": reps, "iters_per_column": int(its[0]),
                   "a_pcg_halo_kernel_rhs_it_per_s": summary(ra), "b_pcg_halo_copies_rhs_it_per_s": summary(rb),
                   "c_group_batch_rhs_it_per_s": summary(rc),
                   "ratio_a_over_c": ratios(ra, rc), "ratio_a_over_b": ratios(ra, rb),
                   "model_ratio_a_over_c": model_ratio(width, nrhs), "slots_per_row": width,
                   "group_pcg_workspace_bytes": [hp.group_pcg_workspace_bytes(M) for M in Ms],
                   "unit_m_bitwise_equal_to_group_batch": same}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            for M in Ms:
                M.batch_release()
                hp.group_pcg_release(M)
    finally:
        for M in Ms:
            M.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2:200x200x100,2:100x100x50",
                    help="members:nx x ny x nz of every member, comma separated")
    ap.add_argument("--nrhs", default="4,1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg", "group_pcg_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5 alternations")
    import torch
    hp = load_pkg()
    hp.set_device(0)
    recs = []
    for sz in [v for v in args.sizes.split(",") if v]:
        P, grid = sz.split(":")
        recs += run_size(hp, torch, int(P), tuple(int(v) for v in grid.split("x")),
                         [int(v) for v in args.nrhs.split(",")], args.reps, args.max_iter)
    doc = {"device": hp.device_name()[0], "results": recs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in recs if not r["unit_m_bitwise_equal_to_group_batch"]]
    for r in bad:
        print(f"MISMATCH: {r['members']} x {r['grid']} nrhs {r['nrhs']}: the group preconditioned solve with m = 1 is "
              "not bitwise the group batch", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
