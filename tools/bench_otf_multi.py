#!/usr/bin/env python3
"""Measurements of the lanes on the sparse on-the-fly path: fp32 RBF, gamma = 1/d, CSR data with
density * d distinct uniform columns per row and values in [-1, 1] (tools/density_1pct.py's), sparse_algo="onthefly".

Two contexts on the same data in one process: `seq` with multi_width=1 (every right-hand side through the single-vector
kernel, one after another) and `lanes` (one pass over the pairs per group). Per round, alternating the two:

  * K·P: time_kp_multi(R) on each, R = 2, 4, 8 (on `seq` that is R single products);
  * learn: R sequential learn() calls on `seq` against learn_multi on `lanes`, R one-vs-all classes, --imax iterations
    at most (0 skips the learn comparison); the iteration counts must agree.

--rounds rounds; medians and the spread (max - min) per figure; every round is written to --out
(profiles/otf_lanes_ab.json) under the configuration's name, beside the configurations already there. One GPU.

  python tools/bench_otf_multi.py --points 100000 --features 20000 --density 0.02
  python tools/bench_otf_multi.py --points 200000 --features 50000 --density 0.01
  python tools/bench_otf_multi.py --points 200000 --features 50000 --density 0.001
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


def random_csr(n, d, k, seed=3):
    rng = np.random.default_rng(seed)
    col = np.empty((n, k), np.int32)
    for i in range(n):
        col[i] = np.sort(rng.choice(d, k, replace=False, shuffle=False))
    val = rng.uniform(-1.0, 1.0, (n, k)).astype(np.float32)
    return np.arange(0, (n + 1) * k, k, dtype=np.int64), col.reshape(-1), val.reshape(-1), n, d


def context(csr, width, cost, eps):
    p = pm.Parameter("rbf", gamma=1.0 / csr[4], cost=cost, epsilon=eps, real_type=np.float32)
    p.csr = csr
    svm = pm.CSVM(p, sparse_algo="onthefly", **({} if width is None else {"multi_width": width}))
    svm.setup_data_on_device()
    svm.generate_q()
    assert svm.info()["sparse_algo"] == _abi.SPARSE_ONTHEFLY
    return svm


def summary(v):
    return {"rounds": v, "median": statistics.median(v), "spread": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=20_000)
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=1, help="products per timed K·P window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--imax", type=int, default=10, help="CG iterations per learn at most; 0: K·P only")
    ap.add_argument("--cost", type=float, default=10.0)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "otf_lanes_ab.json"))
    args = ap.parse_args()
    n, d = args.points, args.features
    per_row = max(1, round(d * args.density))
    name = f"{n}x{d}@{100 * args.density:g}%"
    csr = random_csr(n, d, per_row)
    res = {"config": f"sparse fp32 RBF {n} x {d}, {per_row} entries per row, gamma = 1/d, on the fly", "reps": args.reps,
           "learn_config": f"R one-vs-all classes, C = {args.cost}, eps = {args.eps}, imax = {args.imax}", "kp_ms": {},
           "learn_s": {}}
    with context(csr, 1, args.cost, args.eps) as seq, context(csr, None, args.cost, args.eps) as lanes:
        assert seq.info()["multi_width"] == 1
        res["multi_width"] = lanes.info()["multi_width"]
        kp = {r: {"sequential": [], "lanes": []} for r in (2, 4, 8)}
        ln = {r: {"sequential": [], "lanes": [], "iterations": None} for r in (2, 4, 8)} if args.imax > 0 else {}
        labs = {r: np.random.default_rng(r).integers(0, r, n) for r in ln}
        for rnd in range(args.rounds):
            print(f"{name}: round {rnd + 1} of {args.rounds}", file=sys.stderr, flush=True)
            for r in kp:
                kp[r]["sequential"].append(seq.time_kp_multi(r, args.reps))
                kp[r]["lanes"].append(lanes.time_kp_multi(r, args.reps))
            for r in ln:
                its = []
                t0 = time.perf_counter()
                for y in pm.one_vs_all(labs[r], seq.dtype)[1]:
                    seq.params.labels = y
                    seq.learn(args.imax)
                    its.append(int(seq.iters))
                ln[r]["sequential"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                lanes.learn_multi(labs[r], args.imax)
                ln[r]["lanes"].append(time.perf_counter() - t0)
                assert its == [int(v) for v in lanes.iters_multi], (its, lanes.iters_multi)
                ln[r]["iterations"] = its
        for r in kp:
            s, l = summary(kp[r]["sequential"]), summary(kp[r]["lanes"])
            res["kp_ms"][f"R{r}"] = {"sequential": s, "lanes": l, "speedup_of_medians": s["median"] / l["median"]}
        for r in ln:
            s, l = summary(ln[r]["sequential"]), summary(ln[r]["lanes"])
            res["learn_s"][f"R{r}"] = {"sequential": s, "lanes": l, "speedup_of_medians": s["median"] / l["median"],
                                       "iterations_per_class": ln[r]["iterations"]}
    print(json.dumps(res, indent=1))
    if args.out:
        allres = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                allres = json.load(f)
        allres[name] = res
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(allres, indent=1) + "\n")


if __name__ == "__main__":
    main()
