#!/usr/bin/env python3
"""A search over C as lanes of one CG on BASELINE config 2's shape: dense RBF, 100k points x 256
features, fp64, kernel-matrix tiles stored.

learn_costs on K = 4 and 8 costs (a log grid around C = 1) against the same costs through set_cost + learn() one after
another on the same context: the sequential calls are the baseline (they exist without this feature), alternating
three times each: medians and the spread (max - min) of the three. Every lane must take the iterations of its
sequential solve, and its alpha must be the same bits.

Writes profiles/cost_grid_dense_rbf_100k.json (--out) and prints it. One GPU; --points / --features shrink the problem
for a quick look.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--std", type=float, default=8.0, help="blob sigma (two overlapping classes)")
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_grid_dense_rbf_100k.json"))
    args = ap.parse_args()
    n, d = args.points, args.features
    res = {"config": f"dense RBF {n} x {d} fp64, gamma = 1/d (BASELINE config 2's shape), tiles stored",
           "learn_config": f"two blobs, sigma {args.std}, eps = {args.eps}, imax = {d}", "grids": {}}
    X, lab = class_blobs(n, d, 2, args.std)
    p = pm.Parameter("rbf", gamma=1.0 / d, cost=1.0, epsilon=args.eps, real_type=np.float64)
    p.data, p.labels = X, np.where(lab == 0, 1.0, -1.0)
    with pm.CSVM(p, kp_cache=True) as svm:
        svm.learn()  # stores the tiles; not timed
        for k in (4, 8):
            costs = np.logspace(-1.5, 1.5, k)  # 0.03 .. 30 around C = 1
            seq, grid, it_seq, it_grid, same = [], [], None, None, True
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                its, alphas = [], []
                for c in costs:
                    svm.set_cost(c)
                    svm.learn()
                    its.append(int(svm.iters))
                    alphas.append(svm.alpha)
                seq.append(time.perf_counter() - t0)
                svm.set_cost(1.0)
                t0 = time.perf_counter()
                svm.learn_costs(costs)
                grid.append(time.perf_counter() - t0)
                it_seq, it_grid = its, [int(v) for v in svm.iters_multi]
                same = same and all(np.array_equal(a, b) for a, b in zip(alphas, svm.alphas))
            assert it_seq == it_grid and same, (it_seq, it_grid, same)
            info = svm.info()
            res["grids"][f"K{k}"] = {
                "costs": [float(c) for c in costs], "iterations_per_cost": it_grid, "lanes_bitwise_sequential": same,
                "sequential_s": seq, "grid_s": grid,
                "sequential_median_s": statistics.median(seq), "grid_median_s": statistics.median(grid),
                "sequential_spread_s": max(seq) - min(seq), "grid_spread_s": max(grid) - min(grid),
                "speedup_of_medians": statistics.median(seq) / statistics.median(grid),
                "multi_width": info["multi_width"], "kp_cache_tiles": info["kp_cache_tiles"],
                "tiles_local": info["tiles_local"],
            }
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
