#!/usr/bin/env python3
"""Dense Laplacian K.p beside dense RBF at config 2's shape (100k x 256 blobs): run on the GPU box.

Per kernel and real type, `--runs` times in alternation (laplacian, rbf, laplacian, ...), each on a fresh context:
* first_kp_ms      the first K.p of the setup, wall clock around plssvm_mi_kp: every tile formed (Laplacian: the VALU
                   L1 loop, RBF: MFMA) and stored in the tile cache; includes the 0.8 MB host copies of p and the result;
* implicit_ms      the tile kernel alone over all tiles, nothing stored (plssvm_mi_time_kp's dominant-kernel time,
                   hipEvents, L2 / Infinity Cache evicted before each launch);
* streamed_kp_ms   a later K.p: the stored tiles streamed (plssvm_mi_time_kp's K.p time, hipEvents);
* cg_iters_per_s   forced CG iterations on the streamed tiles (wall clock over `--steps` iterations after a warm-up);
* tiles            the record forms of the stored fp64 tiles: raw / 7-byte / narrow.
For the Laplacian rows the fp64 VALU floor is reported too: tiles x 16384 pairs x d features x 2 operations over the
vector non-FMA issue rate (39.3 T lane-operations/s fp64 by the data sheet: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz; the
fp32 rate without packed instructions is the same). Prints one JSON document; --out writes it to a file as well.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plssvm_sparse_fp22_amd as pm  # noqa: E402
from plssvm_sparse_fp22_amd import datagen  # noqa: E402

VALU_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def one_run(kernel, dtype, X, y, steps, kp_reps):
    n, d = X.shape
    p = pm.Parameter(kernel, gamma=1.0 / d, real_type=dtype)
    p.data, p.labels = X, y
    m = n - 1
    with pm.CSVM(p) as svm:
        svm.setup_data_on_device()
        q = svm.generate_q()
        v = np.linspace(1.0, 2.0, m).astype(dtype)
        ret = np.zeros(m, dtype=dtype)
        t0 = time.perf_counter()
        svm.run_device_kernel(None, ret, v, 1.0)
        first = time.perf_counter() - t0
        ms_kp, ms_dom = svm.time_kp(kp_reps)
        b = (y[:m] - y[m]).astype(dtype)
        svm.cg_begin(b, eps=1e-30)
        svm.cg_step(3, force=True)
        t0 = time.perf_counter()
        svm.cg_step(steps, force=True)
        cg = time.perf_counter() - t0
        info = svm.info()
    tiles = info["tiles_local"]
    row = {"first_kp_ms": first * 1e3, "implicit_ms": ms_dom, "streamed_kp_ms": ms_kp, "cg_iters_per_s": steps / cg,
           "tiles": {"all": tiles, "cached": info["kp_cache_tiles"],
                     "raw": info["kp_cache_tiles"] - info["kp_cache_packed_tiles"],
                     "7-byte": info["kp_cache_packed_tiles"] - info["kp_cache_narrow_tiles"],
                     "narrow": info["kp_cache_narrow_tiles"]},
           "kp_cache_bytes": info["kp_cache_bytes"], "checksum": float(np.abs(ret).sum()), "q0": float(q[0])}
    if kernel == "laplacian":
        floor = tiles * 128 * 128 * info["d_pad"] * 2 / VALU_LANE_OPS_PER_S * 1e3
        row["valu_floor_ms"] = floor
        row["implicit_frac_of_floor"] = floor / ms_dom
        row["first_kp_frac_of_floor"] = floor / (first * 1e3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kp-reps", type=int, default=3)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"points": args.points, "features": args.features, "runs": args.runs, "protocol": "alternating, fresh context per run"}
    for name in args.dtypes.split(","):
        dtype = {"f64": np.float64, "f32": np.float32}[name]
        X, y = datagen.blobs(args.points, args.features, seed=2, dtype=dtype)
        rows = {"laplacian": [], "rbf": []}
        for _ in range(args.runs):
            for kernel in ("laplacian", "rbf"):
                rows[kernel].append(one_run(kernel, dtype, X, y, args.steps, args.kp_reps))
                print(name, kernel, json.dumps(rows[kernel][-1]), file=sys.stderr, flush=True)
        res[name] = {k: {"runs": v, "median": {f: float(np.median([r[f] for r in v]))
                                                for f in ("first_kp_ms", "implicit_ms", "streamed_kp_ms", "cg_iters_per_s")}}
                     for k, v in rows.items()}
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
