"""The sparse K.p and predict paths against a high-precision reference, off [-1, 1] data and with signed vectors
(DESIGN.md §5.5).

Every other accuracy check of a sparse path draws features in [-1, 1], multiplies by p ~ U(1, 2) and compares with the
C oracle, which rounds like the code under test. Here the reference is written in this file, in np.longdouble (LD of
test_gpu_kernel_envelope), from the inputs already rounded to the context's type (FP22: packed and decoded): the CSR is
densified, k_ij comes from direct differences (RBF) or an integer power (polynomial, linear), Q~ p is formed as in
check_kp's definition, K p + (QA - q) sum(p) - q.p + p / cost, with q and QA from the reference, and the decision
values are sum_j alpha_j k(z, x_j) + b. The reference is checked once against the oracle on the CPU.

Shapes: m = 2100 (+ the last point): one row past a 2048-row Gram cell, past an on-the-fly partner window (1024 fp64 /
2048 fp32 partners) and past 32 SELL-64 slices; d = 40 with 6 entries per row (most overlapping pairs share two or
more features); 131 predict points (one on a support vector, one on the last point, one empty).

Vectors per case: (0) U(1, 2); (1) N(0, 1) on a 2^-10 grid with the last entry set so that the sum is exactly zero in
either type; (2) sign 10^U(-6, 0); unit vectors at rows 0, 63, 64, 2047, 2048 and m - 1 (a column of Q~ each). The three
general vectors run through run_device_kernel (vector 1 with add = -1), all nine through run_device_kernel_multi.

Paths per case: auto, sparse_algo = expansion (where the restated rule of DESIGN §5.1 makes it eligible), pattern,
onthefly and dense, rbf_form = 1 (RBF), generate_q and QA_cost on each of them; the linear kernel through the factored
SELL SpMV, kp_mode = "pairwise" and pairwise on the fly. On rbf_control, rbf_cancel, rbf_ladder_K2 and rbf_tiny the
expansion also runs with PLSSVM_MI_EXP_ROWS = index / flags / pairs, PLSSVM_MI_EXP_HFMT = full and PLSSVM_MI_CTR = 0.
The storage rule of DESIGN §5.1.2 is restated (_hratio): in fp32 rbf_ladder_K2 and rbf_tiny store H as bfloat16
(exp_hbytes 2, exp_layout 1 / 2 / 4 for index / flags / pairs, 4 bytes and layout 1 with HFMT = full), rbf_control and
rbf_cancel keep H in the real type (|H| / k up to 1e-2 and 8e2 against 2^-16), where the row index is the only layout;
centered is 0 with CTR = 0 and 1 otherwise. Predict: predict_values_multi with K = 3 and with 8 unit-vector
classes through the default route (the expansion predict where it applies), PLSSVM_MI_PRED_BRUTE = 1 and
PLSSVM_MI_PRED_SEQ = 1; predict_values of class 0 is column 0 bit for bit. predict_algo must be the route of the
restated rule (_predict_rule: brute force only where the expansion is off, a point exceeds the model's largest |x| or
meets more than 4096 repeat sightings: the ragged, heavy-column and beyond-16 cases) and predict_stats must show the
classes sharing a pass ([3, 1]) or, with PRED_SEQ, running one by one ([1, 3]).

Bounds. K.p, q and QA_cost: 1e-12 (fp64) / 1e-4 (fp32), for the positive vector (0) of max|ref| as everywhere else in
the suite, and for every vector of the term-wise scale

    S = max_i [ sum_j (|k_ij| + |QA| + |q_i| + |q_j|) |p_j| + |p_i| / cost ]

taken from the reference: the bound of a Q~ p formed term by term, which a signed p does not shrink. Both constants
exceed m eps_T, the worst-case growth of an m-term sum. On the CPU,
test_cpu_reference_is_finite_and_scale_does_not_loosen_the_old_contract shows S within a factor 8 of max|ref| for
vector (0). Decision values: 1e-10 / 1e-4 of max_p sum_j |alpha_j| |k(z_p, x_j)| + |b|.
Single kernel values (RBF and polynomial; column k of the unit-vector classes is k(z_p, x_{j_k})):

    |got - ref| <= C eps_T (1 + gamma (|a|^2 + |b|^2 + 2 |a.b|)) |ref| + tiny_T

with C per kernel function and route from a numpy model in the context's type of the arithmetic DESIGN documents:
"brute" is the sparse fma dot product, the fma norms and kval of predict.hip; "expansion" is exp_pred_point_kernel's
e_z (S + J_z + w_j H_jz) with the moments rounded to the type, the Horner sum in the type's fma and H in fp64.
test_cpu_model_sets_C evaluates both over every case (never the GPU's output); C_BOUND is 4x the model's largest ratio
for the summation order. Where a polynomial value cancels (gamma s + coef0 near 0 at degree 5 and 16 on the x30 data)
the expansion's sum of binomial terms has no relative accuracy and neither has its model: that C (3.4e46) bounds
nothing, so the unit-vector classes are also held to the decision values' bound, 1e-10 / 1e-4 of the class's largest
value. The linear kernel has no single-value bound of this form (its w path is covered by the decision values).

Cases: rbf / poly / linear control (datagen.sparse_csr, gamma = 1/d); tiny (x 1e-3: small-argument expm1, centred
finalize); the RBF Taylor ladder K = 2, 4, 5, 8, 9, 16 at 0.98 of each degree's largest 2 gamma max x^2 and one step
beyond 16 (auto: Gram pattern; forcing the expansion raises); 2 gamma max|s| at 0.995 / 1.005 (factored form) and at
0.99 / 1.01 of the small-argument bound of the type; cancelling pairs (odd rows below m / 2 copy their neighbour with the
largest feature's sign flipped, odd rows above are exact duplicates, 2 gamma a near the K = 16 edge); ragged rows (empty,
single-feature, one with all d features) with the last point empty and with the last point the row of largest norm;
a heavy column (feature 0 in every row at 8 U(0.1, 1), vector (0) times 1e3) for rbf, polynomial and linear; the
polynomial kernel on values x 30 with degree 1, 2, 5, 16, coef0 0, 1, -0.7 and gamma 1/d, 2 (degree 16 with gamma = 2 in
fp32 is dropped: the reference's kernel values, 1e64, exceed float's range, test_cpu_dropped_cases_overflow_the_type); FP22 control and cancelling pairs for rbf and
linear (fp32 contexts: FP22 is a storage format of float); linear on values x 1e3.

MEASURED on an MI355X (worst over the cases of a group, all paths and vectors; fp64 / fp32, as a fraction of S for
K.p, of max|q| and QA for q and QA_cost, of sum |alpha k| + |b| for the decision values):

    group                          K.p               q, QA_cost        decision values
    control (rbf, poly, linear)    4.1e-16 / 1.7e-7  4.3e-16 / 2.4e-7  5.5e-17 / 3.4e-8
    tiny                           2.1e-16 / 5.3e-8  5.6e-17 / 4.1e-8  2.5e-17 / 8.9e-9
    Taylor ladder, beyond 16       3.1e-16 / 1.4e-7  1.8e-16 / 2.1e-7  2.9e-17 / 1.6e-8
    Gram thresholds                2.7e-16 / 1.1e-7  1.6e-16 / 9.7e-8  2.7e-17 / 1.3e-8
    cancelling pairs               2.8e-16 / 1.7e-7  1.8e-16 / 2.1e-7  1.6e-17 / 8.2e-9
    ragged (rbf, poly)             2.8e-16 / 1.3e-7  3.8e-16 / 2.0e-7  2.9e-17 / 1.4e-8
    heavy column (rbf, poly, lin)  1.2e-15 / 8.1e-7  3.7e-16 / 2.2e-7  2.7e-17 / 1.3e-8
    poly x 30, degree 1, 2         6.1e-16 / 2.3e-7  2.5e-16 / 1.3e-7  5.8e-17 / 2.6e-8
    poly x 30, degree 5            4.0e-15 / 6.2e-7  4.9e-16 / 3.0e-7  2.1e-16 / 1.2e-7
    poly x 30, degree 16           3.4e-15 / 1.8e-6  1.4e-15 / 1.1e-6  1.4e-15 / 7.5e-7
    FP22 (fp32)                    1.6e-7            2.7e-7            4.2e-8
    linear x 1e3                   3.6e-16 / 1.1e-7  8.5e-17 / 6.3e-8  5.6e-17 / 2.8e-8

The positive vector against max|ref|, the old contract: at most 1.9e-15 / 1.4e-6 (linear heavy column). Single kernel
values need C = 1.26 (rbf, brute; bound 5), 5.15 (rbf, expansion, K = 16 in fp32; bound 15), 26.3 (polynomial, brute,
degree 16; fp32: 16.3; bound 106) and 3.2e46 (polynomial, expansion; fp32: 2.7e44), and stay within 3.8e-15 / 1.1e-6 of
the class's largest value. Found and fixed on the way: the Gram pattern's polynomial K.p of degree 16 on the unit vectors at rows
64 and 2047 missed 1e-12 of S by up to 9.6e-11 in all six fp64 cases, because the fixed-point quantum of a cell came
from the cell's largest |s| alone; with the bound per row it is 3.4e-15. And rbf_tiny in fp64 predicted by brute
force although its points lie inside the model's range: expansion_predict compared max|z| with sqrt(umax / 2 gamma),
which rounds either way when max|z| = max|x|; it now compares 2 gamma max z^2 with umax. No case is an xfail.
"""
import functools
import math
import os
from typing import NamedTuple

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen
from test_gpu_kernel_envelope import DEC_TOL, DTYPES, KP_TOL, LD

gpu = pytest.mark.gpu

M = 2100  # rows of Q~; the last point is row M of the data
N = M + 1
D = 40
NNZ = 6
NPTS = 131
UNIT_ROWS = (0, 63, 64, 2047, 2048, M - 1)  # unit vectors of the K.p
PRED_ROWS = (0, 1, 63, 64, 2047, 2048, M - 1, M)  # unit-vector classes of the predict
NGEN = 3  # general vectors; classes of the summed predict
EXP_KMAX = 16
SMALL_BOUND = {"f64": 0.0017, "f32": 0.007}  # expm1's short polynomial (sparse.hip expm1_small_bound)
FACT_RANGE = {"f64": 300.0, "f32": 40.0}  # gamma max|x_i|^2 of the factored rbf form
ALGO = {"expansion": _abi.SPARSE_EXPANSION, "pattern": _abi.SPARSE_PATTERN, "dense": _abi.SPARSE_DENSE,
        "onthefly": _abi.SPARSE_ONTHEFLY}
# the model's largest ratio per (kernel function, route), test_cpu_model_sets_C, and 4x over it
C_MODEL = {("rbf", "brute"): 1.24, ("rbf", "expansion"): 3.74, ("polynomial", "brute"): 26.3,
           ("polynomial", "expansion"): 3.41e46}
C_BOUND = {("rbf", "brute"): 5.0, ("rbf", "expansion"): 15.0, ("polynomial", "brute"): 106.0,
           ("polynomial", "expansion"): 1.4e47}


class Case(NamedTuple):
    name: str
    kernel: str
    data: str
    # a number, or per type: ("edge", K, f): 2 gamma max x^2 = f times the largest value of Taylor degree K;
    # ("s", x): 2 gamma max|s_ij| = x; ("small", f): 2 gamma max|s_ij| = f times the small-argument bound
    gamma: object = 1.0 / D
    degree: int = 3
    coef0: float = 0.0
    dtypes: tuple = ("f64", "f32")
    fp22: bool = False
    pscale: float = 1.0  # vector (0) is U(1, 2) times this
    claims: tuple = ()  # what the case is there for: (key of _rules, value), checked on the CPU and on the GPU
    variants: bool = False  # also run the expansion's layout / storage / finalize variants


# ---- the setup rules of DESIGN §5.1 / §5.2, restated ------------------------------------------------------------------
def taylor_degree(umax, dt):
    """The smallest K >= 1 with umax^K e^(2 umax) / (K + 1)! <= 2^-27 (fp32) / 2^-56 (fp64); 17: none up to 16."""
    tol = 2.0 ** -27 if dt == "f32" else 2.0 ** -56
    K, fact = 1, 2.0
    while K <= EXP_KMAX and umax ** K * math.exp(2.0 * umax) / fact > tol:
        K += 1
        fact *= K + 1
    return K


def taylor_edge(K, dt):
    """The largest umax that still gives a degree <= K (bisection)."""
    lo, hi = 0.0, 16.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if taylor_degree(mid, dt) <= K else (lo, mid)
    return lo


def _ladder(K):
    return Case(f"rbf_ladder_K{K}", "rbf", "control", ("edge", K, 0.98), claims=(("K", K), ("auto", "expansion")),
                variants=K == 2)


CASES = [
    Case("rbf_control", "rbf", "control", claims=(("auto", "expansion"),), variants=True),
    Case("poly_control", "polynomial", "control", coef0=1.0, claims=(("auto", "expansion"), ("K", 3))),
    Case("linear_control", "linear", "control"),
    Case("rbf_tiny", "rbf", "tiny", claims=(("small", 1), ("factored", 1), ("auto", "expansion")), variants=True),
    *[_ladder(K) for K in (2, 4, 5, 8, 9, 16)],
    Case("rbf_ladder_beyond16", "rbf", "control", ("edge", 16, 1.03), claims=(("K", 17), ("auto", "pattern"))),
    Case("rbf_gram_factored_under", "rbf", "control", ("s", 0.995), claims=(("factored", 1), ("small", 0))),
    Case("rbf_gram_factored_over", "rbf", "control", ("s", 1.005), claims=(("factored", 0), ("small", 0))),
    Case("rbf_gram_small_under", "rbf", "control", ("small", 0.99), claims=(("factored", 1), ("small", 1))),
    Case("rbf_gram_small_over", "rbf", "control", ("small", 1.01), claims=(("factored", 1), ("small", 0))),
    Case("rbf_cancel", "rbf", "cancel", ("edge", 16, 0.98), claims=(("K", 16), ("auto", "expansion")), variants=True),
    Case("rbf_ragged_empty_last", "rbf", "ragged_empty"),
    Case("rbf_ragged_big_last", "rbf", "ragged_big"),
    Case("rbf_heavy_column", "rbf", "heavy", pscale=1e3, claims=(("auto", "pattern"), ("factored", 0))),
    Case("poly_heavy_column", "polynomial", "heavy", coef0=1.0, pscale=1e3, claims=(("auto", "expansion"),)),
    Case("poly_ragged_big_last", "polynomial", "ragged_big", coef0=1.0),
    Case("rbf_fp22_control", "rbf", "control", dtypes=("f32",), fp22=True),
    Case("rbf_fp22_cancel", "rbf", "cancel", ("edge", 16, 0.98), dtypes=("f32",), fp22=True, claims=(("K", 16),)),
    Case("linear_fp22_control", "linear", "control", dtypes=("f32",), fp22=True),
    Case("linear_fp22_cancel", "linear", "cancel", dtypes=("f32",), fp22=True),
    Case("linear_x1e3", "linear", "x1e3"),
    Case("linear_heavy_column", "linear", "heavy", pscale=1e3),
]
POLY_OFF = [Case(f"poly_x30_degree{deg}_coef{c0:g}_gamma{'2' if g == 2.0 else 'inv_d'}", "polynomial", "x30", g, degree=deg,
                 coef0=c0, claims=(("K", deg), ("auto", "expansion")))
            for deg in (1, 2, 5, EXP_KMAX) for c0 in (0.0, 1.0, -0.7) for g in (1.0 / D, 2.0)]


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _ragged(rng, n, last):
    X = np.zeros((n, D))
    for i in range(n):
        k = 0 if i % 97 == 0 else (1 if i % 5 == 1 else (D if i == 5 else int(rng.integers(2, 13))))
        cols = rng.choice(D, size=k, replace=False)
        X[i, cols] = rng.uniform(-1, 1, k)
    if last == "big":  # the last point: every feature, the largest norm of the set
        X[n - 1] = rng.choice([-1.0, 1.0], D) * rng.uniform(0.8, 1.0, D)
    elif last == "empty":
        X[n - 1] = 0.0
    return X


@functools.lru_cache(maxsize=None)
def _master(data):
    """X [N][D] and Z [NPTS][D], densified, in float64 before the rounding to the context's type; zeros are absent."""
    X = datagen.densify(datagen.sparse_csr(N, D, NNZ, seed=2027, dtype=np.float64)[0])
    Z = datagen.densify(datagen.sparse_csr(NPTS, D, NNZ, seed=2028, dtype=np.float64)[0])
    rng = np.random.default_rng(2029)
    if data == "tiny":
        X, Z = 1e-3 * X, 1e-3 * Z
    elif data == "x30":
        X, Z = 30.0 * X, 30.0 * Z
    elif data == "x1e3":
        X, Z = 1e3 * X, 1e3 * Z
    elif data == "cancel":
        # rows 2j + 1 < M / 2: row 2j with the sign of its largest feature flipped (products +a and -a in one s_ij);
        # rows 2j + 1 >= M / 2: exact duplicates of row 2j (s = |x|^2, k = 1)
        for i in range(1, M, 2):
            X[i] = X[i - 1]
            if i < M // 2:
                f = np.argmax(np.abs(X[i]))
                X[i, f] = -X[i, f]
    elif data in ("ragged_empty", "ragged_big"):
        X = _ragged(rng, N, data[7:])
        Z = _ragged(rng, NPTS, "none")
    elif data == "heavy":
        # one feature in every row at 8x the scale of the rest, all of one sign; the last point at the lower end, so
        # that Q~_ij = k_ij - q_i - q_j + QA (linear: (x_i - x_m).(x_j - x_m)) keeps one sign and S stays near max|ref|
        X[:, 0] = 8.0 * rng.uniform(0.1, 1.0, N)
        X[M, 0] = 0.8
        Z[:, 0] = 8.0 * rng.uniform(0.1, 1.0, NPTS)
    else:
        assert data == "control"
    Z[0] = X[5]  # a predict point on a support vector
    Z[1] = X[M]  # one on the last point
    Z[2] = 0.0  # an empty one
    X.setflags(write=False)
    Z.setflags(write=False)
    return X, Z


def _csr(Xr, mask, words=None):
    """The CSR tuple of the rounded dense rows Xr with the master's pattern; words: pack the values (FP22)."""
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
    col = np.nonzero(mask)[1].astype(np.int32)
    val = Xr[mask]
    return rowptr, col, (words(val) if words else val), Xr.shape[0], Xr.shape[1]


@functools.lru_cache(maxsize=None)
def _data(data, dt, fp22):
    """The features as the context sees them: rounded to the type, FP22 packed and decoded."""
    T = DTYPES[dt]
    Xm, Zm = _master(data)
    X, Z = Xm.astype(T), Zm.astype(T)
    if fp22:
        from oracle import pyoracle

        pyoracle.build()
        X = pyoracle.fp22_unpack(pyoracle.fp22_pack(X.ravel()), X.size).reshape(X.shape).astype(T)
        Z = pyoracle.fp22_unpack(pyoracle.fp22_pack(Z.ravel()), Z.size).reshape(Z.shape).astype(T)
    X.setflags(write=False)
    Z.setflags(write=False)
    return X, Z


@functools.lru_cache(maxsize=None)
def _maxima(data, dt, fp22):
    """max x^2 and max |x_i|^2 over the rows of Q~ (the setup's amax, nmax), max |s_ij| over i != j < M, and
    max |s| over all pairs with the last point and the predict points; float64 from the rounded values."""
    X, Z = _data(data, dt, fp22)
    X64, Z64 = X.astype(np.float64), Z.astype(np.float64)
    G = X64[:M] @ X64[:M].T
    nmax = float(np.diag(G).max())
    np.fill_diagonal(G, 0.0)
    sall = max(float(np.abs(X64 @ X64.T).max()), float(np.abs(Z64 @ X64.T).max()))
    return float((X64[:M] ** 2).max()), nmax, float(np.abs(G).max()), sall


def _gamma(case, dt):
    """The case's gamma as the context holds it (rounded to the type)."""
    T = DTYPES[dt]
    g = case.gamma
    if isinstance(g, tuple):
        amax, _, smax, _ = _maxima(case.data, dt, case.fp22)
        if g[0] == "edge":  # 2 gamma max x^2 at a fraction of the largest umax of Taylor degree g[1]
            g = g[2] * taylor_edge(g[1], dt) / (2.0 * amax)
        elif g[0] == "s":
            g = g[1] / (2.0 * smax)
        else:
            assert g[0] == "small"
            g = g[1] * SMALL_BOUND[dt] / (2.0 * smax)
    return float(T(g))


def _rules(case, dt):
    """What the setup must decide on this case (the expansion's Taylor degree and eligibility; §5.2: the
    Gram pattern's factored rbf form and its small-argument polynomial)."""
    amax, nmax, smax, _ = _maxima(case.data, dt, case.fp22)
    g = _gamma(case, dt)
    r = dict(umax=2.0 * abs(g) * amax, us=2.0 * abs(g) * smax)
    if case.kernel == "rbf":
        r["fact_ok"] = int(abs(g) * nmax <= FACT_RANGE[dt])
        r["K"] = taylor_degree(r["umax"], dt)
        r["eligible"] = bool(r["fact_ok"] and r["K"] <= EXP_KMAX)
        r["factored"] = int(r["us"] <= 1.0)
        r["small"] = int(r["us"] < SMALL_BOUND[dt])
    elif case.kernel == "polynomial":
        r["K"] = case.degree
        r["eligible"] = 0 <= case.degree <= EXP_KMAX
    else:
        return r
    r["auto"] = "expansion" if r["eligible"] else "pattern"
    return r


def _hratio(case, dt):
    """DESIGN §5.1.2, restated for rbf: the largest |H_ij| / (1 + E(s_ij)) over the pairs i != j < M that share two or
    more features, H_ij = E(s_ij) - sum_f E(x_if x_jf), E(a) = expm1(2 gamma a). In a float context H is stored as
    bfloat16 while this is at most 2^-16 (and the row layouts index / flags / pairs exist only then)."""
    X = _data(case.data, dt, case.fp22)[0][:M].astype(np.float64)
    g2 = 2.0 * _gamma(case, dt)
    s, sphi, shared = X @ X.T, np.zeros((M, M)), np.zeros((M, M), dtype=int)
    for f in range(D):
        r = np.nonzero(X[:, f])[0]
        sphi[np.ix_(r, r)] += np.expm1(g2 * X[r, f, None] * X[None, r, f])
        shared[np.ix_(r, r)] += 1
    ratio = np.abs(np.expm1(g2 * s) - sphi) / (1.0 + np.expm1(g2 * s))
    np.fill_diagonal(shared, 0)
    return float(ratio[shared >= 2].max())


def _predict_rule(case, dt):
    """The route predict must take without PLSSVM_MI_PRED_BRUTE (expansion_predict): the expansion where
    the context runs it, max z^2 <= max x^2 of the model (rbf: the Taylor degree covers every 2 gamma x z), gamma
    max|z|^2 within the factored form's range (rbf), and no point with more than 4096 repeat sightings of support vectors
    (a row sharing k features with the point is seen k - 1 times again); brute force otherwise."""
    if case.kernel == "linear":
        return _abi.PREDICT_LINEAR
    X, Z = (a.astype(np.float64) for a in _data(case.data, dt, case.fp22))
    g = abs(_gamma(case, dt))
    ok = _rules(case, dt)["eligible"]
    if case.kernel == "rbf":
        ok = ok and 2.0 * g * (Z ** 2).max() <= _rules(case, dt)["umax"] and g * (Z ** 2).sum(1).max() <= FACT_RANGE[dt]
    shared = (Z != 0).astype(int) @ (X[:M] != 0).astype(int).T
    ok = ok and np.maximum(shared - 1, 0).sum(1).max() <= 4096
    return _abi.PREDICT_EXPANSION if ok else _abi.PREDICT_BRUTE


# dropped: the reference itself (kernel values of 1e64) exceeds float's range, test_cpu_dropped_cases_overflow_the_type
DROPPED = {(f"poly_x30_degree16_coef{c0}_gamma2", "f32") for c0 in ("0", "1", "-0.7")}
CASES += [c._replace(dtypes=tuple(dt for dt in c.dtypes if (c.name, dt) not in DROPPED)) for c in POLY_OFF]
RUNS = [(c, dt) for c in CASES for dt in c.dtypes]
IDS = [f"{c.name}-{dt}" for c, dt in RUNS]
CONTROL = [(c, dt) for c, dt in RUNS if c.name in ("rbf_control", "poly_control", "linear_control", "rbf_fp22_control")]
VARIANTS = [(c, dt) for c, dt in RUNS if c.variants]
KERNEL_VALUE_RUNS = [(c, dt) for c, dt in RUNS if c.kernel != "linear"]


@functools.lru_cache(maxsize=None)
def _inputs(case, dt):
    T = DTYPES[dt]
    X, Z = _data(case.data, dt, case.fp22)
    Xm, Zm = _master(case.data)
    words = None
    if case.fp22:
        from oracle import pyoracle

        words = pyoracle.fp22_pack
    rng = np.random.default_rng(11)
    P = np.zeros((NGEN + len(UNIT_ROWS), M))
    P[0] = case.pscale * rng.uniform(1.0, 2.0, M)
    P[1] = np.round(rng.standard_normal(M) * 1024.0) / 1024.0
    P[1, -1] -= P[1].sum()  # every value a multiple of 2^-10 below 2^13: the sum is exactly zero in any order and type
    P[2] = rng.choice([-1.0, 1.0], M) * 10.0 ** rng.uniform(-6.0, 0.0, M)
    P[NGEN + np.arange(len(UNIT_ROWS)), UNIT_ROWS] = 1.0
    UA = np.zeros((len(PRED_ROWS), N))
    UA[np.arange(len(PRED_ROWS)), PRED_ROWS] = 1.0
    out = dict(X=X, Z=Z, csr=_csr(X, Xm != 0, words), zcsr=_csr(Z, Zm != 0), P=P.astype(T),
               A=rng.standard_normal((NGEN, N)).astype(T), b=rng.standard_normal(NGEN).astype(T), UA=UA.astype(T))
    assert out["P"][1].astype(LD).sum() == 0
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the reference ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _geometry(data, dt, fp22, what):
    """what = "gram": a.b, "dist": |a - b|^2 by direct differences, for a in [X; Z] and b in X; LD from the rounded
    inputs. Shared by the cases of one data set (the cases of a data set are neighbours in RUNS)."""
    X, Z = _data(data, dt, fp22)
    a, b = np.vstack([X, Z]).astype(LD), X.astype(LD)
    t = np.zeros((a.shape[0], b.shape[0]), dtype=LD)
    for k in range(D):  # only where a feature is present: an absent one contributes 0 (gram) or the other's square, exactly
        ra, rb = np.nonzero(a[:, k])[0], np.nonzero(b[:, k])[0]
        if what == "gram":
            t[np.ix_(ra, rb)] += a[ra, k, None] * b[None, rb, k]
        else:
            diff = a[ra, k, None] - b[None, :, k]
            t[ra] += diff * diff
            t[np.ix_(np.nonzero(a[:, k] == 0)[0], rb)] += (b[rb, k] * b[rb, k])[None, :]
    t.setflags(write=False)
    return t


def _kernel_matrix(case, dt):
    """k(a, x_j) in LD for a in [X; Z]: [N + NPTS][N]."""
    T = DTYPES[dt]
    gamma, coef0 = LD(T(_gamma(case, dt))), LD(T(case.coef0))
    if case.kernel == "rbf":
        return np.exp(-gamma * _geometry(case.data, dt, case.fp22, "dist"))
    G = _geometry(case.data, dt, case.fp22, "gram")
    if case.kernel == "linear":
        return G
    base = gamma * G + coef0
    r = np.ones_like(base)
    for _ in range(case.degree):
        r = r * base
    return r


def _reference_values(case, dt):
    inp = _inputs(case, dt)
    Kall = _kernel_matrix(case, dt)
    K, q, QA, KZ = Kall[:M, :M], Kall[:M, M], Kall[M, M] + LD(1), Kall[N:, :]  # + 1 / cost, cost = 1
    P, A, b = inp["P"].astype(LD), inp["A"].astype(LD), inp["b"].astype(LD)
    aP = np.abs(P)
    kp = (K @ P.T).T + (QA - q)[None, :] * P.sum(1)[:, None] - (P @ q)[:, None] + P  # [vectors][M]
    terms = (np.abs(K) @ aP.T).T + (abs(QA) + np.abs(q))[None, :] * aP.sum(1)[:, None] + (aP @ np.abs(q))[:, None] + aP
    G = _geometry(case.data, dt, case.fp22, "gram")
    nx, nz = np.diag(G)[list(PRED_ROWS)], np.einsum("ij,ij->i", inp["Z"].astype(LD), inp["Z"].astype(LD))
    rows = list(PRED_ROWS)
    return dict(q=q.copy(), QA=QA, kp=kp, S=terms.max(1), dec=KZ @ A.T + b,
                dec_scale=(np.abs(KZ) @ np.abs(A).T).max(0) + np.abs(b), vals=KZ[:, rows].copy(),
                cond=nz[:, None] + nx[None, :] + 2 * np.abs(G[N:, rows]))


def _in_range(ref, dt):
    """Every value the code under test has to return is finite and within the type's range."""
    top = LD(np.finfo(DTYPES[dt]).max)
    return all(np.isfinite(np.asarray(ref[k], dtype=LD)).all() and (np.abs(ref[k]) <= top).all()
               for k in ("q", "QA", "kp", "dec", "vals"))


@functools.lru_cache(maxsize=None)
def _reference(case, dt):
    """Everything the tests compare with, without the kernel matrix itself (70 MB per case)."""
    ref = _reference_values(case, dt)
    for k, v in ref.items():
        assert np.isfinite(np.asarray(v, dtype=LD)).all(), (case.name, dt, k)  # a non-finite reference is a bad case
    assert _in_range(ref, dt), (case.name, dt)
    return ref


def _envelope(case, dt):
    """eps_T (1 + gamma (|z|^2 + |x|^2 + 2 |z.x|)) |ref| for the unit-vector classes' values; C = 1, no floor."""
    T = DTYPES[dt]
    ref = _reference(case, dt)
    return LD(np.finfo(T).eps) * (1 + LD(T(abs(_gamma(case, dt)))) * ref["cond"]) * np.abs(ref["vals"])


def _ratio(got, case, dt):
    """The largest (|got - ref| - tiny_T) / envelope: the C that this result needs."""
    T = DTYPES[dt]
    err = np.abs(np.asarray(got).astype(LD) - _reference(case, dt)["vals"]) - LD(np.finfo(T).tiny)
    env = _envelope(case, dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / env, 0)
    return float(r.max())


# ---- the CPU model of the predict arithmetic (sets C; never the GPU's output) ----------------------------------------
def _fma(a, b, c, T):
    wide = np.float64 if T == np.float32 else LD
    return (np.asarray(a).astype(wide) * np.asarray(b).astype(wide) + np.asarray(c).astype(wide)).astype(T)


def _model_chains(case, dt):
    """x_j . z_p and the squared norms as sequential fma chains in T in column order (zeros add nothing, exactly)."""
    T = DTYPES[dt]
    inp = _inputs(case, dt)
    X, Z = inp["X"][list(PRED_ROWS)], inp["Z"]
    g = np.zeros((NPTS, len(PRED_ROWS)), dtype=T)
    nz, nx = np.zeros(NPTS, dtype=T), np.zeros(len(PRED_ROWS), dtype=T)
    for k in range(D):
        g = _fma(np.broadcast_to(Z[:, k, None], g.shape), np.broadcast_to(X[None, :, k], g.shape), g, T)
        nz, nx = _fma(Z[:, k], Z[:, k], nz, T), _fma(X[:, k], X[:, k], nx, T)
    return g, nz, nx


def _model_kval(case, dt, g, nz, nx):
    """kval of predict.hip in T."""
    T = DTYPES[dt]
    gamma, coef0 = T(_gamma(case, dt)), T(case.coef0)
    if case.kernel == "rbf":
        dist = (nx[None, :] + nz[:, None]).astype(T) - T(2) * g
        return np.exp(-gamma * np.maximum(dist, T(0))).astype(T)
    base = _fma(np.full_like(g, gamma), g, np.full_like(g, coef0), T)
    r = np.ones_like(base)
    for _ in range(case.degree):
        r = (r * base).astype(T)
    return r


def model_brute(case, dt):
    return _model_kval(case, dt, *_model_chains(case, dt))


def _phi_coefs(case, dt):
    """phi(a) = sum_k coef[k] a^k, k = 1 .. K, in float64 as expansion_eligible / make_phi form them."""
    g = float(DTYPES[dt](_gamma(case, dt)))
    if case.kernel == "rbf":
        K = _rules(case, dt)["K"]
        coef, c = [0.0], 1.0
        for k in range(1, K + 1):
            c = c * 2.0 * g / k
            coef.append(c)
        return coef
    coef, binom = [0.0], 1.0
    c0 = float(DTYPES[dt](case.coef0))
    for k in range(1, case.degree + 1):
        binom = binom * (case.degree - k + 1) / k
        coef.append(binom * c0 ** (case.degree - k) * g ** k)
    return coef


def model_expansion(case, dt):
    """exp_pred_point_kernel for a unit-vector class at row j < M: e_z (S + J_z + w_j H_jz) (rbf) / kappa S + J_z +
    H_jz (polynomial), w_j = e_j in T, S = w_j, the moments M_k(f) = coef_k x_jf^k w_j rounded to T, J_z by Horner in
    T's fma over z's entries (summed in float64), H_jz = phi(s) - sum_f phi(x_jf z_f) in float64 where two or more
    features are shared; the last point's class is the brute-force value."""
    T = DTYPES[dt]
    inp = _inputs(case, dt)
    X, Z = inp["X"][list(PRED_ROWS)], inp["Z"]
    g, nz, nx = _model_chains(case, dt)
    brute = _model_kval(case, dt, g, nz, nx)
    gamma = T(_gamma(case, dt))
    coef = _phi_coefs(case, dt)
    K = len(coef) - 1
    rbf = case.kernel == "rbf"
    w = np.exp(-gamma * nx).astype(T) if rbf else np.ones(len(PRED_ROWS), dtype=T)
    w64, X64, Z64 = w.astype(np.float64), X.astype(np.float64), Z.astype(np.float64)

    def phi(a):
        if rbf:
            return np.expm1(2.0 * float(gamma) * a)
        r = np.zeros_like(a)
        for k in range(K, 0, -1):
            r = (r + coef[k]) * a
        return r

    J = np.zeros((NPTS, len(PRED_ROWS)))
    sdot, sphi, shared = np.zeros_like(J), np.zeros_like(J), np.zeros(J.shape, dtype=int)
    for f in range(D):
        both = (Z64[:, f, None] != 0) & (X64[None, :, f] != 0)
        if K >= 1:
            Mk = [(coef[k] * (X64[:, f] ** k * w64)).astype(T) for k in range(1, K + 1)]  # M_k(f) per class, in T
            zf = np.broadcast_to(Z[:, f, None], J.shape)
            h = np.broadcast_to(Mk[K - 1][None, :], J.shape).astype(T)
            for k in range(K - 2, -1, -1):
                h = _fma(h, zf, np.broadcast_to(Mk[k][None, :], J.shape), T)
            J += (h * zf).astype(T).astype(np.float64)
        a = Z64[:, f, None] * X64[None, :, f]
        sdot += a
        sphi += np.where(both, phi(a), 0.0)
        shared += both
    H = np.where(shared >= 2, phi(sdot) - sphi, 0.0)
    if rbf:
        ez = np.exp(-float(gamma) * nz.astype(np.float64))
        v = ez[:, None] * (w64[None, :] + J + w64[None, :] * H)
    else:
        kappa = T(1)
        for _ in range(case.degree):
            kappa = T(kappa * T(case.coef0))
        v = float(kappa) * w64[None, :] + J + H
    out = v.astype(T)
    out[:, -1] = brute[:, -1]
    return out


def test_cpu_model_sets_C():
    """The derivation of C_BOUND, rerun: the model's largest ratio per kernel function and route is the recorded one."""
    worst = {k: (0.0, None) for k in C_MODEL}
    for case, dt in KERNEL_VALUE_RUNS:
        if dt == "f64" and LD is np.float64:
            continue  # no wider type to emulate the fp64 fma with
        routes = [("brute", model_brute)] + ([("expansion", model_expansion)] if _rules(case, dt)["eligible"] else [])
        for route, model in routes:
            r = _ratio(model(case, dt), case, dt)
            if r > worst[case.kernel, route][0]:
                worst[case.kernel, route] = (r, f"{case.name}-{dt}")
    print("model ratios:", worst)
    for key, (r, _) in worst.items():
        assert 0.5 * C_MODEL[key] <= r <= 1.01 * C_MODEL[key], worst
        assert C_BOUND[key] >= 4 * C_MODEL[key]


# ---- CPU tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dt", CONTROL, ids=[f"{c.name}-{dt}" for c, dt in CONTROL])
def test_reference_agrees_with_the_oracle(oracle, case, dt):
    """At the oracle's own contract, the constants of the GPU tests: 1e-12 / 1e-4 for q and K.p (of S; the positive
    vector also of max|ref|), 1e-10 / 1e-4 for the decision values."""
    T = DTYPES[dt]
    inp, ref = _inputs(case, dt), _reference(case, dt)
    args = dict(degree=case.degree, gamma=T(_gamma(case, dt)), coef0=T(case.coef0))
    data = oracle.Data(inp["X"], dtype=T)
    q = oracle.generate_q(case.kernel, data, **args)
    assert np.abs(q - ref["q"]).max() <= KP_TOL[dt] * np.abs(ref["q"]).max()
    for v, add in ((0, 1.0), (1, -1.0), (2, 1.0), (NGEN + 3, 1.0)):
        got = oracle.kp(case.kernel, data, ref["q"].astype(T), T(ref["QA"]), T(1.0), add, inp["P"][v], **args)
        err = np.abs(got - LD(add) * ref["kp"][v]).max()
        assert err <= KP_TOL[dt] * (np.abs(ref["kp"][v]).max() if v == 0 else ref["S"][v]), (v, err)
    for k in range(NGEN):
        got = oracle.predict(case.kernel, inp["X"], inp["A"][k], -inp["b"][k], inp["Z"], **args)
        assert np.abs(got - ref["dec"][:, k]).max() <= DEC_TOL[dt] * ref["dec_scale"][k]


@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_cpu_case_sits_where_it_claims(case, dt):
    """Every threshold case is on its side of the restated rule, by more than the rounding of gamma and of s."""
    r = _rules(case, dt)
    for key, want in case.claims:
        assert r[key] == want, (key, r)
    g = case.gamma
    if isinstance(g, tuple) and g[0] == "edge":
        assert r["umax"] == pytest.approx(g[2] * taylor_edge(g[1], dt), rel=1e-6)
        assert taylor_degree(r["umax"] * (1 - 1e-4), dt) == r["K"] == taylor_degree(r["umax"] * (1 + 1e-4), dt)
    elif isinstance(g, tuple):
        edge = 1.0 if g[0] == "s" else SMALL_BOUND[dt]
        assert r["us"] == pytest.approx(g[1] * edge, rel=1e-6) and abs(r["us"] / edge - 1) > 1e-3
    if isinstance(g, tuple):  # the largest x^2 is in a row of Q~: the rule does not hinge on the last point
        assert _maxima(case.data, dt, case.fp22)[0] == float((_inputs(case, dt)["X"].astype(np.float64) ** 2).max())


def test_cpu_dropped_cases_overflow_the_type():
    """The only combinations left out: degree 16 with gamma = 2 in fp32, whose reference exceeds float's range."""
    dropped = [(c, dt) for c in POLY_OFF for dt in ("f64", "f32") if (c.name, dt) in DROPPED]
    assert len(dropped) == len(DROPPED) == 3
    for case, dt in dropped:
        assert not _in_range(_reference_values(case, dt), dt), case.name
    assert {(c.name, dt) for c, dt in RUNS} >= {(c.name, dt) for c in POLY_OFF for dt in ("f64", "f32")} - DROPPED


@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_cpu_reference_is_finite_and_scale_does_not_loosen_the_old_contract(case, dt):
    """_reference asserts that every value is finite and in the type's range. For the positive vector the term-wise
    scale S lies within a factor 8 of max|ref|: asserting the same constant against S is no looser there."""
    ref = _reference(case, dt)
    top = np.abs(ref["kp"][0]).max()
    assert top <= ref["S"][0] <= 8 * top, (float(ref["S"][0]), float(top))
    for v in range(1, ref["kp"].shape[0]):
        assert np.abs(ref["kp"][v]).max() <= ref["S"][v]


# ---- the GPU runs of a case, once ------------------------------------------------------------------------------------
class _env:
    """Set (or, with None, unset) environment variables for a block and put the old values back."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


DEFAULT_ENV = dict(PLSSVM_MI_EXP_ROWS=None, PLSSVM_MI_EXP_HFMT=None, PLSSVM_MI_CTR=None, PLSSVM_MI_PRED_BRUTE=None,
                   PLSSVM_MI_PRED_SEQ=None)


def _make(case, dt, **kw):
    inp = _inputs(case, dt)
    p = pm.Parameter(case.kernel, degree=case.degree, gamma=_gamma(case, dt), coef0=case.coef0, cost=1.0,
                     real_type=DTYPES[dt])
    p.csr = inp["csr"]
    if case.fp22:
        p.val_fmt = _abi.VAL_FP22
    svm = pm.CSVM(p, **kw)
    svm.setup_data_on_device()
    return svm


def _kp_runs(svm, case, dt):
    T = DTYPES[dt]
    P = _inputs(case, dt)["P"]
    out = dict(q=svm.generate_q().copy(), QA=svm.QA_cost)
    out["single"] = [svm.run_device_kernel(None, np.zeros(M, T), P[v], add).copy() for v, add in ((0, 1.0), (1, -1.0), (2, 1.0))]
    out["multi"] = svm.run_device_kernel_multi(None, np.zeros(P.shape, T), P, 1.0).copy()
    out["info"] = svm.info()
    return out


def _paths(case, dt):
    if case.kernel == "linear":
        return {"factored": {}, "pairwise": dict(kp_mode="pairwise"),
                "pairwise_onthefly": dict(kp_mode="pairwise", sparse_algo="onthefly")}
    paths = {"auto": {}}
    if _rules(case, dt)["eligible"]:
        paths["expansion"] = dict(sparse_algo="expansion")
    paths.update(pattern=dict(sparse_algo="pattern"), onthefly=dict(sparse_algo="onthefly"), dense=dict(sparse_algo="dense"))
    if case.kernel == "rbf":
        paths["direct"] = dict(rbf_form=1)
    return paths


@functools.lru_cache(maxsize=None)
def _gpu(case, dt):
    inp = _inputs(case, dt)
    out = {"kp": {}, "predict": {}}
    with _env(**DEFAULT_ENV):
        for name, kw in _paths(case, dt).items():
            with _make(case, dt, **kw) as svm:
                out["kp"][name] = _kp_runs(svm, case, dt)
        zeros = np.zeros(len(PRED_ROWS))
        with _make(case, dt) as svm:  # auto: the expansion predict where the expansion is on
            for route, env in (("default", {}), ("brute", dict(PLSSVM_MI_PRED_BRUTE="1")), ("seq", dict(PLSSVM_MI_PRED_SEQ="1"))):
                with _env(**env):
                    r = dict(dec=svm.predict_values_multi(inp["zcsr"], alphas=inp["A"], biases=inp["b"]))
                    r["algo"], r["stats"] = svm.info()["predict_algo"], svm.predict_stats()
                    r["vals"] = svm.predict_values_multi(inp["zcsr"], alphas=inp["UA"], biases=zeros)
                    assert svm.info()["predict_algo"] == r["algo"]
                    r["one"] = svm.predict_values(inp["zcsr"], alpha=inp["A"][0], bias=inp["b"][0]).copy()
                    out["predict"][route] = r
    return out


@functools.lru_cache(maxsize=None)
def _gpu_variants(case, dt):
    out = {}
    settings = dict(default={}, rows_index=dict(PLSSVM_MI_EXP_ROWS="index"), rows_flags=dict(PLSSVM_MI_EXP_ROWS="flags"),
                    rows_pairs=dict(PLSSVM_MI_EXP_ROWS="pairs"), hfmt_full=dict(PLSSVM_MI_EXP_HFMT="full"),
                    ctr_off=dict(PLSSVM_MI_CTR="0"))
    for name, env in settings.items():
        with _env(**{**DEFAULT_ENV, **env}):
            with _make(case, dt, sparse_algo="expansion") as svm:
                out[name] = _kp_runs(svm, case, dt)
    return out


def _check(got, want, tol, scales, what, failures):
    """|got - want| <= tol * scale for every (name, scale); prints the error as a fraction of each scale."""
    got = np.asarray(got)
    assert got.shape == np.shape(want), what
    assert np.isfinite(got).all(), (what, "not finite")
    err = np.abs(got.astype(LD) - want).max()
    rel = {k: float(err / max(s, LD(1e-30))) for k, s in scales.items()}  # check_kp's floor
    print(f"  {what}: " + ", ".join(f"{r:.3e} of {k}" for k, r in rel.items()) + f" (tolerance {tol:g})")
    for k, r in rel.items():
        if not r <= tol:
            failures.append(f"{what}: {r:.3e} of {k} > {tol:g}")
    return rel


def _check_kp(run, case, dt, what, failures):
    ref = _reference(case, dt)
    for v, g in enumerate(run["single"]):
        add = LD(-1.0 if v == 1 else 1.0)
        scales = {"S": ref["S"][v], **({"max|ref|": np.abs(ref["kp"][v]).max()} if v == 0 else {})}
        _check(g, add * ref["kp"][v], KP_TOL[dt], scales, f"K.p {what} vector {v}", failures)
    for v in range(ref["kp"].shape[0]):
        scales = {"S": ref["S"][v], **({"max|ref|": np.abs(ref["kp"][v]).max()} if v == 0 else {})}
        _check(run["multi"][v], ref["kp"][v], KP_TOL[dt], scales, f"K.P {what} vector {v}", failures)


# ---- the GPU tests ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_setup_follows_the_restated_rules(case, dt):
    """info() of every path against _rules: the algorithm auto picks, the Taylor degree, the Gram pattern's factored
    form and small-argument polynomial, the centred finalize (on exactly where the expansion runs)."""
    runs, r = _gpu(case, dt)["kp"], _rules(case, dt)
    for name, run in runs.items():
        info = run["info"]
        print(f"  {name}: " + ", ".join(f"{k}={info[k]}" for k in ("sparse_algo", "exp_terms", "rbf_factored", "rbf_small_args",
                                                                    "exp_hbytes", "exp_layout", "centered", "pairs")))
        assert info["is_sparse"] == 1
        assert info["val_fmt"] == (_abi.VAL_FP22 if case.fp22 else _abi.VAL_REAL)
        if case.kernel == "linear":
            assert info["centered"] == 0
            continue
        want = ALGO[r["auto"]] if name in ("auto", "direct") else ALGO[name]
        if name == "direct":
            want = ALGO["pattern"]  # the direct rbf form is the Gram pattern's
        assert info["sparse_algo"] == want, (name, info["sparse_algo"])
        on = want == _abi.SPARSE_EXPANSION
        assert info["exp_terms"] == (r["K"] if on else 0), (name, info["exp_terms"], r["K"])
        assert info["centered"] == (1 if on else 0), name
        if case.kernel == "rbf" and want == _abi.SPARSE_PATTERN:
            assert info["rbf_factored"] == (0 if name == "direct" else r["factored"]), (name, r["us"])
            if name != "direct":
                assert info["rbf_small_args"] == r["small"], (name, r["us"])
        if case.kernel == "rbf" and name == "onthefly":
            assert info["rbf_factored"] == r["fact_ok"]


@gpu
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_forcing_the_expansion_beyond_degree_16_raises(dt):
    case = next(c for c in CASES if c.name == "rbf_ladder_beyond16")
    with pytest.raises(pm.BackendError, match="the kernel expansion cannot represent this kernel on this data"):
        _make(case, dt, sparse_algo="expansion")


@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_q_and_QA_cost(case, dt):
    print(f"\n[q_and_QA_cost {case.name}-{dt}]")
    ref, failures = _reference(case, dt), []
    for name, run in _gpu(case, dt)["kp"].items():
        _check(run["q"], ref["q"], KP_TOL[dt], {"max|q|": np.abs(ref["q"]).max()}, f"q {name}", failures)
        _check(np.array([run["QA"]]), np.array([ref["QA"]]), KP_TOL[dt], {"QA": abs(ref["QA"])}, f"QA_cost {name}", failures)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_kp_on_every_path_and_vector(case, dt):
    print(f"\n[kp_on_every_path_and_vector {case.name}-{dt}]")
    failures = []
    for name, run in _gpu(case, dt)["kp"].items():
        _check_kp(run, case, dt, name, failures)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", VARIANTS, ids=[f"{c.name}-{dt}" for c, dt in VARIANTS])
def test_expansion_variants(case, dt):
    """Row index / chunk flags / pair flags, H in the real type, the plain finalize: each ran (exp_layout, exp_hbytes,
    centered) and each keeps the bounds."""
    print(f"\n[expansion_variants {case.name}-{dt}]")
    runs, failures = _gpu_variants(case, dt), []
    size = np.dtype(DTYPES[dt]).itemsize
    for name, run in runs.items():
        info = run["info"]
        print(f"  {name}: exp_hbytes={info['exp_hbytes']} exp_layout={info['exp_layout']} centered={info['centered']}")
        assert info["sparse_algo"] == _abi.SPARSE_EXPANSION
        _check_kp(run, case, dt, name, failures)
    hratio = _hratio(case, dt)
    print(f"  largest |H| / k of a stored pair: {hratio:.3g} (bfloat16 H up to 2^-16 = {2.0 ** -16:.3g})")
    assert not 0.5 < hratio / 2.0 ** -16 < 2  # the case is clear of the storage bound
    bf16 = dt == "f32" and hratio <= 2.0 ** -16
    if case.name in ("rbf_tiny", "rbf_ladder_K2"):
        assert bf16 == (dt == "f32")  # these two are the cases that store bfloat16 H; the others keep the real type
    layouts = {name: runs[name]["info"]["exp_layout"] for name in ("default", "rows_index", "rows_flags", "rows_pairs")}
    hbytes = {name: run["info"]["exp_hbytes"] for name, run in runs.items()}
    assert hbytes.pop("hfmt_full") == size
    assert set(hbytes.values()) == {2 if bf16 else size}, hbytes
    if bf16:
        assert (layouts["rows_index"], layouts["rows_flags"], layouts["rows_pairs"]) == (1, 2, 4), layouts
        assert layouts["default"] in (2, 4)
        assert runs["hfmt_full"]["info"]["exp_layout"] == 1
    else:  # H in the real type: the row index is the only layout
        assert set(layouts.values()) == {1}, layouts
    assert runs["ctr_off"]["info"]["centered"] == 0
    assert all(run["info"]["centered"] == 1 for name, run in runs.items() if name != "ctr_off")
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_decision_values(case, dt):
    print(f"\n[decision_values {case.name}-{dt}]")
    got, ref, failures = _gpu(case, dt)["predict"], _reference(case, dt), []
    want = _predict_rule(case, dt)
    for route, run in got.items():
        print(f"  {route}: predict_algo {run['algo']}, predict_stats {run['stats']}")
        brute = route == "brute" and case.kernel != "linear"
        assert run["algo"] == (_abi.PREDICT_BRUTE if brute else want), (route, run["algo"], want)
        assert run["stats"] == ([1, NGEN] if route == "seq" else [NGEN, 1]), (route, run["stats"])
        for k in range(NGEN):
            _check(run["dec"][:, k], ref["dec"][:, k], DEC_TOL[dt], {"sum |alpha k| + |b|": ref["dec_scale"][k]},
                   f"decision values {route} class {k}", failures)
        assert np.array_equal(run["one"], run["dec"][:, 0]), route  # predict_values is column 0
    assert np.array_equal(got["seq"]["dec"], got["default"]["dec"])  # the classes one after another: the same bits
    if case.name in ("rbf_control", "poly_control"):
        assert got["default"]["algo"] == _abi.PREDICT_EXPANSION
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", KERNEL_VALUE_RUNS, ids=[f"{c.name}-{dt}" for c, dt in KERNEL_VALUE_RUNS])
def test_single_kernel_values(case, dt):
    print(f"\n[single_kernel_values {case.name}-{dt}]")
    got, failures = _gpu(case, dt)["predict"], []
    for route, run in got.items():
        v = run["vals"]
        assert v.shape == (NPTS, len(PRED_ROWS)) and np.isfinite(v).all(), route
        key = (case.kernel, "expansion" if run["algo"] == _abi.PREDICT_EXPANSION else "brute")
        r = _ratio(v, case, dt)
        print(f"  kernel values {route} ({key[1]}): needs C = {r:.3g} (C = {C_BOUND[key]:g})")
        if not r <= C_BOUND[key]:
            failures.append(f"kernel values {route} ({key[1]}): C {r:.3g} > {C_BOUND[key]:g}")
        # ... and, as a class's decision values, of the largest value of the class (where a value cancels, gamma s +
        # coef0 near 0, the bound above is relative to almost nothing and C is large: this one is not)
        ref = _reference(case, dt)["vals"]
        for k in range(len(PRED_ROWS)):
            _check(v[:, k], ref[:, k], DEC_TOL[dt], {"max|k|": np.abs(ref[:, k]).max()}, f"kernel values {route} class {k}",
                   failures)
    ref = _reference(case, dt)["vals"]
    if case.kernel == "rbf":  # a point on a support vector and one on the last point: the reference is exactly 1
        assert ref[1, -1] == 1
    assert not failures, failures
