#!/usr/bin/env python3
"""A search over gamma as lanes of one CG on BASELINE config 2's shape: dense data, 100k points x 256
features, fp64, for the rbf and the laplacian kernel.

learn_gammas on K = 4 and 8 gammas (a log grid from 0.1 / d to 10 / d) against what exists without the feature: the
same gammas one after another, each as a fresh context (setup, tiles stored on the first K.p) plus learn(). The two
protocols alternate --rounds times: medians and the spread (max - min). Every lane must take the iterations of its
sequential solve, and its alpha must be the same bits.

Writes profiles/gamma_grid_dense_100k.json (--out; an existing file keeps the kernels this run does not time) and
prints it. One GPU; --points / --features / --imax shrink the problem for a quick look.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import plssvm_sparse_fp22_amd as pm  # noqa: E402
from bench_multiclass import class_blobs  # noqa: E402


def param(kernel, X, y, gamma, eps):
    p = pm.Parameter(kernel, gamma=float(gamma), cost=1.0, epsilon=eps, real_type=np.float64)
    p.data, p.labels = X, y
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--kernels", default="rbf,laplacian")
    ap.add_argument("--sizes", default="4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--imax", type=int, default=-1, help="CG iteration cap of both protocols (-1: the number of features)")
    ap.add_argument("--std", type=float, default=8.0, help="blob sigma (two overlapping classes)")
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gamma_grid_dense_100k.json"))
    args = ap.parse_args()
    n, d = args.points, args.features
    imax = d if args.imax < 0 else args.imax
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res["config"] = f"dense {n} x {d} fp64 (BASELINE config 2's shape); two blobs, sigma {args.std}, eps = {args.eps}"
    res.setdefault("kernels", {})
    X, lab = class_blobs(n, d, 2, args.std)
    y = np.where(lab == 0, 1.0, -1.0)
    for kernel in args.kernels.split(","):
        out = res["kernels"][kernel] = {"imax": imax, "grids": {}}
        with pm.CSVM(param(kernel, X, y, 1.0 / d, args.eps), kp_cache=False) as svm:  # the grid stores no tiles
            svm.setup_data_on_device()
            svm.learn_gammas([1.0 / d, 2.0 / d], imax=2)  # warm-up: code objects, the lane pool
            for k in (int(v) for v in args.sizes.split(",")):
                gammas = np.geomspace(0.1 / d, 10.0 / d, k)
                seq, grid, same = [], [], True
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    its, alphas = [], []
                    for g in gammas:  # what users do today: one context per gamma
                        with pm.CSVM(param(kernel, X, y, g, args.eps)) as one:
                            one.learn(imax)
                            its.append(int(one.iters))
                            alphas.append(one.alpha)
                    seq.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    svm.learn_gammas(gammas, imax=imax)
                    grid.append(time.perf_counter() - t0)
                    it_grid = [int(v) for v in svm.iters_multi]
                    same = same and its == it_grid and all(np.array_equal(a, b) for a, b in zip(alphas, svm.alphas))
                assert same, (its, it_grid)
                out["grids"][f"K{k}"] = {
                    "gammas": [float(g) for g in gammas], "iterations_per_gamma": it_grid, "lanes_bitwise_sequential": same,
                    "sequential_s": seq, "grid_s": grid,
                    "sequential_median_s": statistics.median(seq), "grid_median_s": statistics.median(grid),
                    "sequential_spread_s": max(seq) - min(seq), "grid_spread_s": max(grid) - min(grid),
                    "speedup_of_medians": statistics.median(seq) / statistics.median(grid),
                    "multi_width": svm.info()["multi_width"],
                }
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
