#!/usr/bin/env python3
"""Scoring a gamma grid in one call on BASELINE config 2's shape: a dense 100k x 256 fp64 model and
100k points, for the rbf and the laplacian kernel, K = 4 and 8 gammas of the log grid 0.1 / d .. 10 / d.

lanes:       one predict_values_gammas call on the context that holds the data (what learn_gammas leaves);
sequential:  what exists without it: per gamma a fresh context, setup_data_on_device and predict_values.

Every measurement runs in a fresh process of its own (--side; the parent never opens the GPU), after a small warm-up
through the same code paths; the two sides alternate --rounds times: medians and the spread (max - min). Both sides
hash their decision values: the lanes must give the sequential bits.

Writes profiles/predict_gamma_lanes.json (--out) and prints it. One GPU; --points / --features shrink the problem.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def param(pm, kernel, X, gamma):
    p = pm.Parameter(kernel, gamma=float(gamma), real_type=np.float64)
    p.data = X
    return p


def one_side(args):
    """Child process: time one side once, print {"s": seconds, "sha1": of the values [np][K]}."""
    import plssvm_sparse_fp22_amd as pm
    from bench_multiclass import class_blobs

    n, d, k = args.points, args.features, args.k
    X, _ = class_blobs(n, d, 2, args.std)
    Z, _ = class_blobs(n, d, 2, args.std, seed=11)
    rng = np.random.default_rng(3)
    A, b = rng.standard_normal((k, n)), rng.standard_normal(k)
    gammas = np.geomspace(0.1 / d, 10.0 / d, k)
    with pm.CSVM(param(pm, args.kernel, X[:300], 1.0 / d)) as warm:  # code objects of both sides
        warm.predict_values_gammas(Z[:200], gammas[:2], A[:2, :300], b[:2])
        warm.predict_values(Z[:200], A[0, :300], b[0])
    if args.side == "lanes":
        with pm.CSVM(param(pm, args.kernel, X, 1.0 / d), kp_cache=False) as svm:
            svm.setup_data_on_device()
            t0 = time.perf_counter()
            V = svm.predict_values_gammas(Z, gammas, A, b)
            dt = time.perf_counter() - t0
    else:
        cols, t0 = [], time.perf_counter()
        for l, g in enumerate(gammas):
            with pm.CSVM(param(pm, args.kernel, X, g), kp_cache=False) as one:
                one.setup_data_on_device()
                cols.append(one.predict_values(Z, A[l], b[l]))
        dt = time.perf_counter() - t0
        V = np.stack(cols, axis=1)
    print(json.dumps({"s": dt, "sha1": hashlib.sha1(np.ascontiguousarray(V).tobytes()).hexdigest()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--kernels", default="rbf,laplacian")
    ap.add_argument("--sizes", default="4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--std", type=float, default=8.0, help="blob sigma (two overlapping classes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_gamma_lanes.json"))
    ap.add_argument("--side", choices=["lanes", "sequential"], help="(child) time this side once")
    ap.add_argument("--kernel", help="(child)")
    ap.add_argument("--k", type=int, help="(child)")
    args = ap.parse_args()
    if args.side:
        return one_side(args)
    n, d = args.points, args.features
    res = {"config": f"dense {n} x {d} fp64 model, {n} points (BASELINE config 2's shape); a fresh process per measurement",
           "kernels": {}}
    for kernel in args.kernels.split(","):
        out = res["kernels"][kernel] = {}
        for k in (int(v) for v in args.sizes.split(",")):
            t = {"sequential": [], "lanes": []}
            sha = set()
            for _ in range(args.rounds):
                for side in ("sequential", "lanes"):
                    cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--kernel", kernel, "--k", str(k),
                           "--points", str(n), "--features", str(d), "--std", str(args.std)]
                    r = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.splitlines()[-1])
                    t[side].append(r["s"])
                    sha.add(r["sha1"])
            assert len(sha) == 1, "the lanes do not give the sequential bits"
            seq, lan = t["sequential"], t["lanes"]
            out[f"K{k}"] = {"gammas": [float(g) for g in np.geomspace(0.1 / d, 10.0 / d, k)], "lanes_bitwise_sequential": True,
                            "sequential_s": seq, "lanes_s": lan,
                            "sequential_median_s": statistics.median(seq), "lanes_median_s": statistics.median(lan),
                            "sequential_spread_s": max(seq) - min(seq), "lanes_spread_s": max(lan) - min(lan),
                            "speedup_of_medians": statistics.median(seq) / statistics.median(lan)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
