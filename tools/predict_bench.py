#!/usr/bin/env python3
"""predict / update_w throughput on BASELINE-shaped models (SURVEY §8(f)2 measurement; run on the GPU box).

* dense RBF, config 2's model: 100k support vectors x 256 fp64, 100k predict points: the fused MFMA tile
  kernel (csrc/predict_tiles.hip), 2 d n np FLOP whatever the number of classes; reported against the fp64
  MFMA peak. --classes K[,K...] runs only this row, once per K, through predict_values_multi (K one-vs-all
  classes in one call); --gemm sets PLSSVM_MI_PRED_GEMM=1 (rocBLAS G = X Z^T + the kernel/alpha epilogue,
  once per class: the A/B baseline). The kernel's share of the seconds comes from a kernel trace of this
  command (rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py --classes 8; tools/top_kernels.py);
* sparse RBF, config 3-RBF's model: 1M support vectors x 50k CSR fp32 (5e7 entries), 4096 CSR points:
  through the kernel expansion (the model's column moments once, then per point its features' moment
  sums and the support vectors sharing two or more features with it), beside the brute-force kernel
  (every support vector entry gathered per 64 points, PLSSVM_MI_PRED_BRUTE);
* linear update_w on config 3 (the SELL CSC pass, w = sum alpha_i x_i);
* --sparse-classes K[,K...] runs only the sparse rows, once per K, through predict_values_multi: config 3-RBF's model
  through the expansion and through the brute-force sweep, and config 3's linear model (w_c . z). The points are
  prepared once and up to 8 classes share each pass over the support vectors; PLSSVM_MI_PRED_SEQ=1 in the
  environment runs the classes one after another (the A/B baseline of the shared pass).
Times include the host transfers of the points and results (the C ABI takes host buffers); alpha is
random (the model's alphas do not change the work). Prints one JSON line.
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


def timed(fn, reps=3):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


ALGO = {v: k for k, v in vars(pm._abi).items() if k.startswith("PREDICT_") and k != "PREDICT_SEG_TILES"}


def sparse_classes(res, rng, ks, reps):
    """config 3-RBF's model (expansion, brute force) and config 3's linear model with K classes per call"""
    n, d, k, npts = 1_000_000, 50_000, 50, 4096
    csr, y = datagen.sparse_csr(n, d, k, seed=3, dtype=np.float32)
    zc, _ = datagen.sparse_csr(npts, d, k, seed=11, dtype=np.float32)
    A = rng.standard_normal((max(ks), n)).astype(np.float32)
    b = rng.standard_normal(max(ks)).astype(np.float32)
    seq = os.environ.get("PLSSVM_MI_PRED_SEQ", "0") != "0"
    for kern, rows in (("rbf", (("csr_rbf_1m_expansion", False, reps), ("csr_rbf_1m_brute", True, 1))),
                       ("linear", (("csr_linear_1m", False, 1),))):
        p = pm.Parameter(kern, gamma=1.0 / d, real_type=np.float32)
        p.csr, p.labels = csr, y
        with pm.CSVM(p) as svm:
            svm.setup_data_on_device()
            for name, brute, r in rows:
                if brute:
                    os.environ["PLSSVM_MI_PRED_BRUTE"] = "1"
                row = {"support_vectors": n, "d": d, "points": npts, "dtype": "f32", "reps": r, "sequential": seq}
                for K in ks:
                    s, _ = timed(lambda: svm.predict_values_multi(zc, alphas=A[:K], biases=b[:K]), r)
                    row[f"K{K}"] = {"seconds": s, "seconds_per_class": s / K,
                                    "predict_algo": ALGO[svm.info()["predict_algo"]]}
                    if hasattr(svm, "predict_stats"):
                        row[f"K{K}"]["predict_stats"] = svm.predict_stats()
                os.environ.pop("PLSSVM_MI_PRED_BRUTE", None)
                res[name] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default=None, metavar="K[,K...]",
                    help="only the dense row, with K one-vs-all classes per predict_values_multi call")
    ap.add_argument("--gemm", action="store_true", help="PLSSVM_MI_PRED_GEMM=1: rocBLAS + epilogue, once per class")
    ap.add_argument("--sparse-classes", default=None, metavar="K[,K...]",
                    help="only the sparse rows (expansion, brute force, linear), K classes per predict_values_multi call")
    ap.add_argument("--points", type=int, default=100_000, help="support vectors and predict points of the dense row")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel", choices=["rbf", "laplacian"], default="rbf",
                    help="kernel of the dense row; laplacian: the VALU L1-distance tile kernel, always the fused path")
    args = ap.parse_args()
    if args.gemm:
        os.environ["PLSSVM_MI_PRED_GEMM"] = "1"
    res = {}
    rng = np.random.default_rng(7)
    if args.sparse_classes is not None:
        sparse_classes(res, rng, [int(v) for v in args.sparse_classes.split(",")], args.reps)
        print(json.dumps(res), flush=True)
        return
    # dense RBF (config 2 model)
    n, d, npts = args.points, 256, args.points
    X, y = datagen.blobs(n, d, seed=2)
    Z, _ = datagen.blobs(npts, d, seed=9)
    p = pm.Parameter(args.kernel, gamma=1.0 / d, real_type=np.float64)
    p.data, p.labels = X, y
    flop = 2.0 * d * n * npts  # rbf: MFMA FLOP; laplacian: the same count of VALU operations (subtract, add |.|)
    dense_row = f"dense_{args.kernel}_100k"
    with pm.CSVM(p) as svm:
        svm.setup_data_on_device()
        alpha = rng.standard_normal(n)
        if args.classes is None:
            s, _ = timed(lambda: svm.predict_values(Z, alpha=alpha, bias=0.1), args.reps)
            res[dense_row] = {"support_vectors": n, "d": d, "points": npts, "dtype": "f64", "seconds": s,
                                     "points_per_s": npts / s, "TFLOPs_on_2dnnp": flop / s / 1e12,
                                     "frac_of_fp64_mfma_peak": flop / s / 78.6e12,
                                     "predict_algo": ALGO[svm.info()["predict_algo"]]}
        else:
            row = {"support_vectors": n, "d": d, "points": npts, "dtype": "f64", "reps": args.reps}
            for k in (int(v) for v in args.classes.split(",")):
                A = rng.standard_normal((k, n))
                b = rng.standard_normal(k)
                s, _ = timed(lambda: svm.predict_values_multi(Z, alphas=A, biases=b), args.reps)
                row[f"K{k}"] = {"seconds": s, "seconds_per_class": s / k, "TFLOPs_on_2dnnp": flop / s / 1e12,
                                "frac_of_fp64_mfma_peak": flop / s / 78.6e12,
                                "predict_algo": ALGO[svm.info()["predict_algo"]]}
            res[dense_row] = row
    if args.classes is not None:
        print(json.dumps(res), flush=True)
        return
    # sparse RBF (config 3-RBF model) and linear update_w (config 3)
    n, d, k, npts = 1_000_000, 50_000, 50, 4096
    csr, y = datagen.sparse_csr(n, d, k, seed=3, dtype=np.float32)
    zc, _ = datagen.sparse_csr(npts, d, k, seed=11, dtype=np.float32)
    for kern in ("rbf", "linear"):
        p = pm.Parameter(kern, gamma=1.0 / d, real_type=np.float32)
        p.csr, p.labels = csr, y
        with pm.CSVM(p) as svm:
            svm.setup_data_on_device()
            alpha = rng.standard_normal(n).astype(np.float32)
            if kern == "rbf":
                s, _ = timed(lambda: svm.predict_values(zc, alpha=alpha, bias=0.1), reps=3)
                os.environ["PLSSVM_MI_PRED_BRUTE"] = "1"
                sb, _ = timed(lambda: svm.predict_values(zc, alpha=alpha, bias=0.1), reps=1)
                del os.environ["PLSSVM_MI_PRED_BRUTE"]
                nnz = int(csr[0][-1])
                res["csr_rbf_1m"] = {"support_vectors": n, "d": d, "nnz": nnz, "points": npts, "dtype": "f32",
                                     "path": "kernel expansion (moments + multi-feature partners per point)",
                                     "seconds": s, "points_per_s": npts / s,
                                     "brute_force_seconds": sb, "brute_force_points_per_s": npts / sb}
            else:
                s, _ = timed(lambda: svm.update_w(alpha), reps=5)
                nnz = int(csr[0][-1])
                res["csr_linear_1m_update_w"] = {"nnz": nnz, "seconds": s, "GBps_incl_host_copies": nnz * 6.0 / s / 1e9}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
