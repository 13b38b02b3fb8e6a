#!/usr/bin/env python3
"""Workload for a rocprofv3 --kernel-trace --stats run of the BiCGStab solve:
one matrix, a warm-up and one timed Jacobi solve of nrhs columns (default:
27-pt 200^3, one column, 100 iterations), then the same columns through the
preconditioned CG for the kernels it is measured against.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \\
        python tools/bicgstab_profile.py [--n 200] [--stencil 27] [--nrhs 1] [--max-iter 100]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--stencil", type=int, default=27)
    ap.add_argument("--nrhs", type=int, default=1)
    ap.add_argument("--max-iter", type=int, default=100)
    args = ap.parse_args()
    import torch
    hp = load_pkg()
    hp.set_device(0)
    dev = torch.device("cuda:0")
    M = hp.Matrix.generate(args.n, args.n, args.n, use_7pt=args.stencil == 7)
    try:
        rows = args.n ** 3
        B = torch.rand((args.nrhs, rows), dtype=torch.float64, device=dev) * 2.0 - 1.0
        X = torch.zeros_like(B)
        for name, solve in (("bicgstab", hp.HPCCG_bicgstab), ("pcg", hp.HPCCG_pcg)):
            X.zero_()
            solve(M, B, X, max_iter=4, device=True)
            X.zero_()
            _, its, _, times = solve(M, B, X, max_iter=args.max_iter, device=True)
            print(f"{name}: {args.stencil}-pt {args.n}^3 nrhs {args.nrhs}: {int(its.sum())} RHS-iterations in "
                  f"{times[0]:.4f} s")
    finally:
        M.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
