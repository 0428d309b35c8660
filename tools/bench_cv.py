#!/usr/bin/env python3
"""k-fold cross-validation as masked lanes of one CG on BASELINE config 2's shape: dense RBF, 100k
points x 256 features, fp64, kernel-matrix tiles stored.

CSVM.cross_validate (5 folds x {1, 4} costs) against the route a user has without it: per fold a fresh context on the
fold's training subset, learn_costs there, and predict_values on the held-out fifth. The two routes alternate, three
rounds each: medians and the spread (max - min) of the three. Both must give the same held-out predictions; the
iterations of every lane are recorded. No ratio is fixed in advance: a group of 8 lanes streams the stored tiles once
per iteration, where the subset route streams 0.64 of them per lane and pays one setup per fold.

Writes profiles/cv_dense_rbf_100k.json (--out) and prints it. One GPU; --points / --features shrink the problem for a
quick look.
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


def subset_route(X, y, folds, nfold, costs, gamma, eps):
    """Held-out decision values [costs][n] through one fresh context per fold, and the iterations [costs][nfold]."""
    n = y.size
    held = np.empty((len(costs), n))
    iters = np.zeros((len(costs), nfold), dtype=np.int64)
    for f in range(nfold):
        out = folds == f
        p = pm.Parameter("rbf", gamma=gamma, cost=1.0, epsilon=eps, real_type=np.float64)
        p.data, p.labels = np.ascontiguousarray(X[~out]), y[~out]
        with pm.CSVM(p, kp_cache=True) as sub:
            sub.learn_costs(costs)
            Z = np.ascontiguousarray(X[out])
            for c in range(len(costs)):
                held[c, out] = sub.predict_values(Z, sub.alphas[c], sub.biases[c])
                iters[c, f] = sub.iters_multi[c]
    return held, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--std", type=float, default=8.0, help="blob sigma (two overlapping classes)")
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cv_dense_rbf_100k.json"))
    args = ap.parse_args()
    n, d, nfold = args.points, args.features, args.folds
    res = {"config": f"dense RBF {n} x {d} fp64, gamma = 1/d (BASELINE config 2's shape), tiles stored",
           "learn_config": f"two blobs, sigma {args.std}, eps = {args.eps}, imax = {d}, {nfold} stratified folds", "grids": {}}
    X, lab = class_blobs(n, d, 2, args.std)
    y = np.where(lab == 0, 1.0, -1.0)
    p = pm.Parameter("rbf", gamma=1.0 / d, cost=1.0, epsilon=args.eps, real_type=np.float64)
    p.data, p.labels = X, y
    with pm.CSVM(p, kp_cache=True) as svm:
        svm.learn()  # stores the tiles; not timed (the subset route's setups are: a user pays them per fold)
        for k in (1, 4):
            costs = np.array([1.0]) if k == 1 else np.logspace(-1.5, 1.5, k)
            lanes_s, subset_s = [], []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                acc, held, folds = svm.cross_validate(nfold, costs)
                lanes_s.append(time.perf_counter() - t0)
                it_lanes = np.asarray(svm.cv_iters).reshape(k, nfold)
                t0 = time.perf_counter()
                held_sub, it_sub = subset_route(X, y, folds, nfold, costs, 1.0 / d, args.eps)
                subset_s.append(time.perf_counter() - t0)
            same_sign = bool(np.array_equal(held > 0, held_sub > 0))
            info = svm.info()
            res["grids"][f"K{k}"] = {
                "costs": [float(c) for c in costs], "accuracy": [float(a) for a in acc],
                "iterations_per_lane": it_lanes.tolist(), "iterations_subset_route": it_sub.tolist(),
                "same_held_out_predictions": same_sign,
                "held_out_values_max_abs_difference": float(np.abs(held - held_sub).max()),
                "smallest_abs_value": float(np.abs(held_sub).min()),
                "cross_validate_s": lanes_s, "subset_route_s": subset_s,
                "cross_validate_median_s": statistics.median(lanes_s), "subset_route_median_s": statistics.median(subset_s),
                "cross_validate_spread_s": max(lanes_s) - min(lanes_s), "subset_route_spread_s": max(subset_s) - min(subset_s),
                "speedup_of_medians": statistics.median(subset_s) / statistics.median(lanes_s),
                "multi_width": info["multi_width"], "kp_cache_tiles": info["kp_cache_tiles"], "tiles_local": info["tiles_local"],
            }
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
