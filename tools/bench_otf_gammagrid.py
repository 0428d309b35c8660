#!/usr/bin/env python3
"""Gamma lanes on the sparse on-the-fly path: fp32 RBF on tools/bench_otf_multi.py's CSR data,
sparse_algo="onthefly", log grids of R = 4 and 8 gammas from 0.1 / d to 10 / d. One process per shape:

  python tools/bench_otf_gammagrid.py --points 100000 --features 20000 --density 0.02
  python tools/bench_otf_gammagrid.py --points 200000 --features 50000 --density 0.001

Per round, alternating the protocols (host wall time around the call; every call returns synchronised):

  (a) K.P: one run_device_kernel_gammas of R (gamma, p) lanes on one context, against
        `singles`: R run_device_kernel calls, one on each of R fresh on-the-fly contexts (what exists without the feature;
                   their setups are not timed here), and
        `floor`:   one run_device_kernel_multi of the R vectors at one gamma on the same context: the same walk with one
                   exponential per pair instead of R;
  (b) learn: learn_gammas against R x (fresh context + learn()), --imax iterations at most on both sides, the iteration
      counts asserted equal (--imax 0 skips it).

--rounds rounds; medians and the spread (max - min) per figure, every round kept. Results go to --out
(profiles/otf_gamma_lanes_ab.json) under the shape's name, beside the shapes already there. One GPU.
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
from plssvm_sparse_fp22_amd import _abi  # noqa: E402
from bench_otf_multi import random_csr, summary  # noqa: E402


def context(csr, y, gamma, args, width=None):
    p = pm.Parameter("rbf", gamma=float(gamma), cost=args.cost, epsilon=args.eps, real_type=np.float32)
    p.csr, p.labels = csr, y
    svm = pm.CSVM(p, sparse_algo="onthefly", **({} if width is None else {"multi_width": width}))
    svm.setup_data_on_device()
    svm.generate_q()
    assert svm.info()["sparse_algo"] == _abi.SPARSE_ONTHEFLY
    return svm


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=20_000)
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--sizes", default="4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--imax", type=int, default=10, help="CG iterations per learn at most; 0: K.P only")
    ap.add_argument("--cost", type=float, default=10.0)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "otf_gamma_lanes_ab.json"))
    args = ap.parse_args()
    n, d = args.points, args.features
    per_row = max(1, round(d * args.density))
    name = f"{n}x{d}@{100 * args.density:g}%"
    csr = random_csr(n, d, per_row)
    y = np.where(np.random.default_rng(5).uniform(size=n) < 0.5, -1.0, 1.0).astype(np.float32)
    m = n - 1
    res = {"config": f"sparse fp32 RBF {n} x {d}, {per_row} entries per row, on the fly; log grid 0.1/d .. 10/d",
           "learn_config": f"C = {args.cost}, eps = {args.eps}, imax = {args.imax}", "timer": "host wall time per call, seconds",
           "grids": {}}
    with context(csr, y, 1.0 / d, args) as svm:
        res["multi_width"] = svm.info()["multi_width"]
        for R in (int(v) for v in args.sizes.split(",")):
            gammas = np.geomspace(0.1 / d, 10.0 / d, R)
            P = np.random.default_rng(R).uniform(-1, 2, (R, m)).astype(np.float32)
            fresh = [context(csr, y, g, args, width=1) for g in gammas]
            try:
                forms = [bool(c.info()["rbf_factored"]) for c in fresh]
                # warm-up: code objects, the lane pool and its gamma buffers
                svm.run_device_kernel_gammas(gammas, np.zeros_like(P), P, 1.0)
                svm.run_device_kernel_multi(None, np.zeros_like(P), P, 1.0)
                kp = {"singles": [], "floor": [], "gammas": []}
                for rnd in range(args.rounds):
                    print(f"{name}: R = {R}, K.P round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
                    kp["singles"].append(timed(lambda: [c.run_device_kernel(None, np.zeros(m, np.float32), p, 1.0) for c, p in zip(fresh, P)]))
                    kp["floor"].append(timed(lambda: svm.run_device_kernel_multi(None, np.zeros_like(P), P, 1.0)))
                    kp["gammas"].append(timed(lambda: svm.run_device_kernel_gammas(gammas, np.zeros_like(P), P, 1.0)))
            finally:
                for c in fresh:
                    c.close()
            out = {"gammas": [float(g) for g in gammas], "factored_per_gamma": forms, "kp_s": {k: summary(v) for k, v in kp.items()}}
            med = {k: out["kp_s"][k]["median"] for k in kp}
            out["kp_singles_over_gammas"] = med["singles"] / med["gammas"]
            out["kp_gammas_over_floor"] = med["gammas"] / med["floor"]
            out["kp_faster_by_more_than_the_spread"] = min(kp["singles"]) - max(kp["gammas"]) > 0
            if args.imax > 0:
                seq, grid = [], []
                for rnd in range(args.rounds):
                    print(f"{name}: R = {R}, learn round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
                    its = []

                    def sequential():
                        for g in gammas:  # what users do today: one context per gamma
                            with context(csr, y, g, args, width=1) as one:
                                one.learn(args.imax)
                                its.append(int(one.iters))
                    seq.append(timed(sequential))
                    grid.append(timed(lambda: svm.learn_gammas(gammas, imax=args.imax)))
                    assert its == [int(v) for v in svm.iters_multi], (its, svm.iters_multi)
                out["learn_s"] = {"sequential": summary(seq), "gammas": summary(grid), "iterations_per_gamma": its,
                                  "speedup_of_medians": statistics.median(seq) / statistics.median(grid)}
            res["grids"][f"R{R}"] = out
    print(json.dumps(res, indent=1))
    if args.out:
        allres = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                allres = json.load(f)
        allres[name] = res
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(allres, indent=1) + "\n")


if __name__ == "__main__":
    main()
