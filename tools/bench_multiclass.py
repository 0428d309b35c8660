#!/usr/bin/env python3
"""Measurements of the multi-right-hand-side path on BASELINE config 2's shape: dense RBF,
100k points x 256 features, fp64, with K-class labels from K blob centres.

  * K·P time against R: time_kp_multi(R) for R = 1, 2, 4, 8 beside R x time_kp, with the kernel-matrix tiles stored
    and with kp_cache=False (every tile recomputed);
  * learn_multi against K sequential learn() calls on the same context (tiles stored), K = 4 and 8, alternating
    three times each: medians and the spread (max - min) of the three;
  * the device memory of a lane and the width chosen.

Writes profiles/multiclass_dense_rbf_100k.json (--out) and prints it. One GPU; --points / --features shrink the
problem for a quick look.
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


def class_blobs(n, d, k, std, seed=2):
    """k Gaussian blobs (centres ~ U(-10, 10)^d, sigma std, equal classes, shuffled), features min-max scaled to
    [-1, 1]: datagen.blobs with k centres and the class index as the label (sigma 1 separates the classes so well
    that CG stops after 2 iterations; the default sigma here makes them overlap)."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-10.0, 10.0, size=(k, d))
    lab = rng.permutation(np.arange(n) % k)
    X = rng.normal(size=(n, d)) * std + centers[lab]
    lo, hi = X.min(axis=0), X.max(axis=0)
    X = (X - lo) / np.where(hi > lo, hi - lo, 1.0) * 2.0 - 1.0
    return np.ascontiguousarray(X), lab


def context(X, cache, cost=1.0, eps=1e-3):
    p = pm.Parameter("rbf", gamma=1.0 / X.shape[1], cost=cost, epsilon=eps, real_type=np.float64)
    p.data = X
    svm = pm.CSVM(p, kp_cache=cache)
    svm.setup_data_on_device()
    svm.generate_q()
    return svm


def kp_times(X, cache, reps):
    out = {}
    with context(X, cache) as svm:
        svm.time_kp(1)  # the first product of the setup (stores the tiles when the cache is on)
        single = svm.time_kp(reps)[0]
        out["time_kp_ms"] = single
        for r in (1, 2, 4, 8):
            t = svm.time_kp_multi(r, reps)
            out[f"R{r}"] = {"time_kp_multi_ms": t, "R_x_time_kp_ms": r * single, "ratio_to_single": t / single}
        info = svm.info()
        out["kp_cache_tiles"] = info["kp_cache_tiles"]
        out["multi_width"] = info["multi_width"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--std", type=float, default=8.0, help="blob sigma of the learn comparison")
    ap.add_argument("--cost", type=float, default=10.0)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiclass_dense_rbf_100k.json"))
    args = ap.parse_args()
    n, d = args.points, args.features
    res = {"config": f"dense RBF {n} x {d} fp64, gamma = 1/d (BASELINE config 2's shape)", "reps": args.reps,
           "learn_config": f"blob sigma {args.std}, C = {args.cost}, eps = {args.eps}, imax = {d}"}

    X, _ = class_blobs(n, d, 8, 1.0)
    res["kp_stored_tiles"] = kp_times(X, True, args.reps)
    res["kp_implicit"] = kp_times(X, False, max(2, args.reps // 3))

    res["learn"] = {}
    for k in (4, 8):
        X, lab = class_blobs(n, d, k, args.std)
        classes, Y = pm.one_vs_all(lab)
        with context(X, True, args.cost, args.eps) as svm:
            before = svm.info()["device_bytes"]
            svm.params.labels = Y[0]
            svm.learn()  # stores the tiles; not timed
            seq, multi, it_seq, it_multi = [], [], None, None
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                its = []
                for c in range(k):
                    svm.params.labels = Y[c]
                    svm.learn()
                    its.append(int(svm.iters))
                seq.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                svm.learn_multi(lab)
                multi.append(time.perf_counter() - t0)
                it_seq, it_multi = its, [int(v) for v in svm.iters_multi]
            info = svm.info()
            assert it_seq == it_multi, (it_seq, it_multi)
            itemsize = 8
            res["learn"][f"K{k}"] = {
                "iterations_per_class": it_multi,
                "sequential_s": seq, "multi_s": multi,
                "sequential_median_s": statistics.median(seq), "multi_median_s": statistics.median(multi),
                "sequential_spread_s": max(seq) - min(seq), "multi_spread_s": max(multi) - min(multi),
                "speedup_of_medians": statistics.median(seq) / statistics.median(multi),
                "multi_width": info["multi_width"],
                "lane_bytes_formula": (6 * info["n_pad"] + info["tiles_local"] * 256 + 4096) * itemsize,
                "lanes_device_bytes": info["device_bytes"] - before,
                "kp_cache_tiles": info["kp_cache_tiles"], "tiles_local": info["tiles_local"],
            }
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
