"""The dense MFMA paths against a high-precision reference, off the unit cube.

Every other GPU test of the dense tile kernels draws features of order 1 with gamma = 1/d, degree 3, and compares
either with another path of this library or with the C oracle, which rounds like the code under test. Here the
reference is written in this file, in np.longdouble (80-bit on x86; float64 where longdouble is a double), from the
inputs already rounded to the context's type: k_ij by direct differences (RBF), by an integer power of
gamma a.b + coef0 (polynomial) or from the sum of |a - b| (Laplacian), the full Q~ p of run_device_kernel with q and
QA_cost formed by the reference too, and the decision values sum_j alpha_j k(z, x_j) + b. The reference is checked once
against the oracle on the CPU; the oracle does not know the Laplacian kernel, whose reference is checked against
test_gpu_laplacian's float64 numpy and an example by hand instead (test_laplacian_reference_anchor).

Paths, per case and real type (the contexts of a case are built once and shared by its tests):
  (a) implicit K.p (kp_cache=False)                      (e) fused predict, K = 3 classes
  (b) the filling K.p of a cached context                (f) rocBLAS predict (PLSSVM_MI_PRED_GEMM=1)
  (c) K.p streamed from stored tiles (fp64 RBF: packed   (g) generate_q and QA_cost
      and raw records)                                   (h) single kernel values: 8 unit-vector classes through
  (d) run_device_kernel_multi, R = 3                         (e) and (f), column k is k(z_p, x_{j_k})
  (i) single values of kp_tile_kernel: kp_part(e_j, "kernel") for the unit-vector rows j < m is K[:, j] (fma(kv, 1, 0)
      and exact zeros), computed and streamed from every record form (the same bits), X against X in the envelope,
      K[i, j] == K[j, i] on the rows x rows sub-matrix
The Laplacian kernel has no rocBLAS predict: its (f) round asserts the tile kernel and the bits of (e). Its fp64 cases run
(b) - (d) with packed and with raw records like the RBF cases, each bitwise the implicit K.p.

Shapes: m = 130 (+ the last point) is three tiles with a ragged last tile row, d = 24 (d = 257 once per kernel),
131 predict points; one RBF case is test_gpu_kp_pack's mixed data at m = 300 (packed and raw tiles in one cache).

Tolerances. The summed results keep the project's contract relative to max|ref| of the vector: K.p and q 1e-12
(fp64) / 1e-4 (fp32), decision values 1e-10 / 1e-4. Single kernel values are bound by

    |got - ref| <= C eps_T (1 + gamma (|a|^2 + |b|^2 + 2 |a.b|)) |ref| + tiny_T

with the norms of the data as the kernel sees it (shifted by the context's column means where info()["rbf_shift"]
says so). C comes from a numpy model of the arithmetic (norm trick, sequential fma dot product and norms in T, in
forward and in reversed feature order; never the GPU's output), evaluated for every case by test_cpu_model_sets_C:
the largest ratio of the model's error to the bound with C = 1 is 2.33 over the RBF cases (fp64, mixed data at
gamma = 40, shift subtracted; 2.22 for fp32 at offset 1000 as given) and 916 over the polynomial cases (fp32, degree 5, coef0 = 0, gamma = 1/d: an
element whose base gamma a.b is small against its terms); 4x over that for the summation order of a d-term dot
product on MFMA gives C = 9.5 (RBF) and C = 3700 (polynomial). One C per kernel function, each no larger than the
single C over all cases would be. (Measured on an MI355X afterwards, for the record: the results need C = 3.3
for RBF, on the mixed data in fp64, and C = 1780 for the polynomial kernel, degree 5, coef0 = 0, gamma = 1/d, fp64.)

The Laplacian envelope is eps_T (1 + gamma |a - b|_1) |ref| + tiny_T: no norms, L1 differences do not cancel. Its model
(D += |a - b| feature by feature in T, exp(T(-gamma D)), both feature orders) has its largest ratio, 3.39, at d = 257 in
fp64 (2.68 in fp32), and the device's sum order is the model's, so the 4x, C = 13.6, covers the device's exp against
numpy's. (Measured on an MI355X afterwards: the predict kernel's values need C = 3.03, d = 257, fp64; kp_tile_kernel's,
path (i), C = 3.6, d = 257, fp32. On path (i) the RBF values need C = 2.56, d = 257, fp64, and the polynomial ones that
pass C = 3590, degree 4, coef0 = 0, gamma = 1/d, fp32.) What holds exactly for this kernel is asserted with ==: equal
points give 1 (predict, q, the K.p tile values, QA_cost = 1 + 1 / cost), and at gamma = 1e8 K is the identity, so
kp_part returns a signed p bit for bit.

Three K.p cases miss the summed contract and are strict xfails with their measured errors (KP_XFAIL). On path (i) five
polynomial runs with coef0 = 0, gamma = 1/d miss the envelope through one element whose dot product cancels by 1e5
(KVAL_XFAIL: the CPU model needs the same C), and eight fp64 RBF runs are not bitwise symmetric inside a diagonal tile
(KSYM_XFAIL: the one-fma form of the fast exp's argument treats n_i and n_j differently; one ulp).
"""
import functools
import os
from typing import NamedTuple

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi

gpu = pytest.mark.gpu

LD = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
DTYPES = {"f64": np.float64, "f32": np.float32}
KP_TOL = {"f64": 1e-12, "f32": 1e-4}
DEC_TOL = {"f64": 1e-10, "f32": 1e-4}
C_MODEL = {"rbf": 2.33, "polynomial": 916.0, "laplacian": 3.39}  # the largest model ratio, test_cpu_model_sets_C
C_BOUND = {"rbf": 9.5, "polynomial": 3700.0, "laplacian": 13.6}  # 4x over it
TILE = 128
NPTS = 131
R = 3  # vectors of the multi K.p, classes of the summed predict


class Case(NamedTuple):
    name: str
    kernel: str
    data: str
    gamma: float
    d: int = 24
    degree: int = 3
    coef0: float = 0.0
    m: int = 130
    dtypes: tuple = ("f64", "f32")
    packed: str = "any"  # fp64 RBF, kp_pack on: "all" tiles packed, "some", or whatever the values allow


CASES = [
    Case("rbf_control", "rbf", "unit", 1.0 / 24, packed="all"),
    Case("rbf_offset100", "rbf", "off100", 1.0 / 24),
    Case("rbf_offset1000", "rbf", "off1000", 1.0 / 24),
    Case("rbf_column1e4", "rbf", "col1e4", 1.0 / 24),
    Case("rbf_scale100", "rbf", "scale100", 1.0 / (24 * 1e4)),
    Case("rbf_duplicates", "rbf", "dups", 1.0 / 24),
    Case("rbf_d257", "rbf", "unit", 1.0 / 257, d=257),
    Case("rbf_mixed_gamma40", "rbf", "mixed", 40.0, d=20, m=300, packed="some"),
    # gamma |x_i - x_j|^2 over 250 ... 1400 (|x_i - x_j|^2 = 16 +- 4): about a tenth of the pairs in 700 ... 760,
    # where the fp64 result is denormal; fp32: 35 ... 190 around the 80 ... 110 of its denormals
    Case("rbf_underflow", "rbf", "unit", 45.0, dtypes=("f64",)),
    Case("rbf_underflow", "rbf", "unit", 6.0, dtypes=("f32",)),
    Case("rbf_gamma1e8", "rbf", "unit", 1e8, dtypes=("f64",)),  # |y| > 2^31 in exp_scaled_f64
    Case("poly_offset100_degree2", "polynomial", "off100", 1.0 / 24, degree=2, coef0=1.0),
    Case("poly_d257", "polynomial", "unit", 1.0 / 257, d=257, degree=3, coef0=1.0),
]
CASES += [Case(f"poly_degree{deg}_coef{c0:g}_gamma{'2' if g == 2.0 else 'inv_d'}", "polynomial", "unit", g, degree=deg,
               coef0=c0)
          for deg in (1, 2, 4, 5) for c0 in (-1.0, 0.0, 2.5) for g in (1.0 / 24, 2.0)]
# The Laplacian kernel exp(-gamma |a - b|_1): the RBF cases' data (L1 differences do not cancel: no shift), d on both sides
# of the K loop's chunk depth of 16 (1, 17, 24, 257 = 16 chunks and one feature), values from 1 down to e^-24 and through
# the subnormals to 0 (|x_i - x_j|_1 = 16 +- 2 at d = 24), and a gamma at which K is exactly the identity
CASES += [
    Case("lap_control", "laplacian", "unit", 1.0 / 24),
    Case("lap_offset100", "laplacian", "off100", 1.0 / 24),
    Case("lap_offset1000", "laplacian", "off1000", 1.0 / 24),
    Case("lap_column1e4", "laplacian", "col1e4", 1.0 / 24),
    Case("lap_scale100", "laplacian", "scale100", 1.0 / 2400),
    Case("lap_duplicates", "laplacian", "dups", 1.0 / 24),
    Case("lap_d257", "laplacian", "unit", 1.0 / 257, d=257),
    Case("lap_d1", "laplacian", "unit", 1.0, d=1),
    Case("lap_d17", "laplacian", "unit", 1.0 / 17, d=17),
    Case("lap_gamma1", "laplacian", "unit", 1.0),
    Case("lap_underflow", "laplacian", "unit", 45.0, dtypes=("f64",)),
    Case("lap_underflow", "laplacian", "unit", 6.0, dtypes=("f32",)),
    Case("lap_gamma1e8", "laplacian", "unit", 1e8),
]
RUNS = [(c, dt) for c in CASES for dt in c.dtypes]
IDS = [f"{c.name}-{dt}" for c, dt in RUNS]
# K.p results that miss the contract, measured on an MI355X (every K.p path of the case alike)
KP_XFAIL = {
    "rbf_gamma1e8-f64": "4.3e-9 of max|K.p| against 1e-12: the diagonal k_ii = exp(-gamma (2 |x_i|^2 - 2 x_i.x_i)) comes from "
                        "the norm trick like every other value, and its rounding, eps |x_i|^2, is multiplied by gamma = 1e8",
    "poly_offset100_degree2-f64": "1.2e-11 against 1e-12: k_ij is 1e8 and Q~ p 1.8e6, k_ij + QA_cost - q_i - q_j cancels; "
                                  "the C oracle, the reference's formula in fp64, misses by 8.4e-12 itself",
    "poly_offset100_degree2-f32": "5.8e-3 against 1e-4: the same cancellation; the C oracle in fp32 misses by 4.0e-3 itself",
}
KP_RUNS = [pytest.param(c, dt, id=i, marks=[pytest.mark.xfail(strict=True, reason=KP_XFAIL[i])] if i in KP_XFAIL else [])
           for (c, dt), i in zip(RUNS, IDS)]
# single values of kp_tile_kernel that miss their envelope, measured on an MI355X, with the C they need and the cause
_SMALL_BASE = ("one element: x_26 . x_63 = -5.5e-5 against sum_k |x_26k x_63k| = 5.5, the base gamma a.b + 0 cancels by 1e5 and the "
               "envelope carries no 1 / |a.b|; the numpy model of the arithmetic (sequential fma, forward order) needs the "
               "same C on this value set (test_cpu_model_on_the_kp_values): the envelope's conditioning, not the kernel")
KVAL_XFAIL = {f"poly_degree{deg}_coef0_gammainv_d-{dt}": f"C = {c} against 3700, degree {deg}, {dt}; " + _SMALL_BASE
              for deg, dt, c in ((1, "f64", "6.77e3"), (2, "f64", "1.35e4"), (4, "f64", "2.71e4"), (5, "f64", "3.39e4"),
                                 (5, "f32", "4.49e3"))}
KVAL_RUNS = [pytest.param(c, dt, id=i, marks=[pytest.mark.xfail(strict=True, reason=KVAL_XFAIL[i])] if i in KVAL_XFAIL else [])
             for (c, dt), i in zip(RUNS, IDS)]
# K[i, j] != K[j, i] inside a diagonal tile, measured on an MI355X: the largest |K_ij - K_ji| of the rows x rows sub-matrix
_FAST_EXP = ("the fp64 RBF epilogue of kp_tile_kernel (FAST_EXP) starts the accumulator of column j at -n_j / 2 and forms "
             "y_ij = 2 g KEXP (x_i.x_j - n_j / 2) - g KEXP n_i in one fma: n_i and n_j enter at different roundings, so the two "
             "halves of a diagonal tile differ in the last bit; one ulp of a value inside its envelope, the price of one "
             "fma per element in the hot epilogue, left as it is")
KSYM_XFAIL = {f"rbf_{name}-f64": f"max |K_ij - K_ji| = {a}: " + _FAST_EXP
              for name, a in (("control", "1.1e-16"), ("offset100", "1.1e-16"), ("offset1000", "5.6e-17"),
                              ("scale100", "1.1e-16"), ("duplicates", "1.1e-16"), ("d257", "1.1e-16"),
                              ("mixed_gamma40", "2.2e-16"), ("underflow", "2.8e-256"))}
KSYM_RUNS = [pytest.param(c, dt, id=i, marks=[pytest.mark.xfail(strict=True, reason=KSYM_XFAIL[i])] if i in KSYM_XFAIL else [])
             for (c, dt), i in zip(RUNS, IDS)]
CONTROL = [(c, dt) for c, dt in RUNS if c.name in ("rbf_control", "poly_degree4_coef2.5_gammainv_d")]


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _master(data, d, m):
    """X [m + 1][d] and Z [NPTS][d] in float64, before the rounding to the context's type."""
    rng = np.random.default_rng(2024 + d + m)
    if data == "mixed":
        from test_gpu_kp_pack import _mixed

        X = np.array(_mixed(m)[0])
        Z = rng.uniform(-1, 1, (NPTS, d))
        Z[:40] = X[0] + 1e-3 * rng.standard_normal((40, d))  # next to the cluster: values near 1
        return X, Z
    X = rng.uniform(-1, 1, (m + 1, d))
    Z = rng.uniform(-1, 1, (NPTS, d))
    if data == "off100":
        X, Z = X + 100.0, Z + 100.0
    elif data == "off1000":
        X, Z = X + 1000.0, Z + 1000.0
    elif data == "col1e4":
        X[:, 3] += 1e4
        Z[:, 3] += 1e4
    elif data == "scale100":
        X, Z = 100.0 * X, 100.0 * Z
    elif data == "dups":
        X[1::2] = X[0:-1:2]  # rows equal in pairs
        X[m] = X[m - 2]  # ... and the last point equal to rows m - 2 and m - 1
        Z[0] = X[5]  # a predict point on a support vector
        Z[1] = X[m]  # and one on the last point
    else:
        assert data == "unit"
    return X, Z


@functools.lru_cache(maxsize=None)
def _inputs(case, dt):
    T = DTYPES[dt]
    X, Z = _master(case.data, case.d, case.m)
    rng = np.random.default_rng(7)
    n = case.m + 1
    out = dict(X=np.ascontiguousarray(X, dtype=T), Z=np.ascontiguousarray(Z, dtype=T),
               P=rng.uniform(1.0, 2.0, (R, case.m)).astype(T), A=rng.standard_normal((R, n)).astype(T),
               b=rng.standard_normal(R).astype(T))
    # unit-vector classes: first and last row of a tile, rows 127 / 128, the last (ragged) row, the last point
    rows = [0, 1, 63, 64, 127, 128, case.m - 1, case.m] if case.m == 130 else [0, 127, 128, 255, 256, 257, case.m - 1, case.m]
    U = np.zeros((len(rows), n), dtype=T)
    U[np.arange(len(rows)), rows] = 1
    out["rows"], out["U"] = rows, U
    out["krows"] = [j for j in rows if j < case.m]  # the unit vectors of a K.p: row k of U without the last point
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the reference ---------------------------------------------------------------------------------------------------
def l1_distances(a, b):
    """|a_i - b_j|_1 for every row pair, in LD."""
    a, b = np.asarray(a).astype(LD), np.asarray(b).astype(LD)
    D = np.zeros((a.shape[0], b.shape[0]), dtype=LD)
    for k in range(a.shape[1]):
        D += np.abs(a[:, k, None] - b[None, :, k])
    return D


def ref_kernel_matrix(case, T, A, B):
    """k(a_i, b_j) in LD from inputs already in T: direct differences (RBF), integer power (polynomial), the sum of
    |a - b| over the features (Laplacian)."""
    a, b = np.asarray(A, dtype=T).astype(LD), np.asarray(B, dtype=T).astype(LD)
    gamma, coef0 = LD(T(case.gamma)), LD(T(case.coef0))
    t = np.zeros((a.shape[0], b.shape[0]), dtype=LD)
    if case.kernel == "laplacian":
        return np.exp(-gamma * l1_distances(a, b))
    if case.kernel == "rbf":
        for k in range(a.shape[1]):
            diff = a[:, k, None] - b[None, :, k]
            t += diff * diff
        return np.exp(-gamma * t)
    for k in range(a.shape[1]):
        t += a[:, k, None] * b[None, :, k]
    base = gamma * t + coef0
    r = np.ones_like(base)
    for _ in range(case.degree):
        r = r * base
    return r


@functools.lru_cache(maxsize=None)
def _reference(case, dt):
    T = DTYPES[dt]
    inp = _inputs(case, dt)
    X, Z, m = inp["X"], inp["Z"], case.m
    K = ref_kernel_matrix(case, T, X[:m], X[:m])
    q = ref_kernel_matrix(case, T, X[:m], X[m:])[:, 0]
    QA = ref_kernel_matrix(case, T, X[m:], X[m:])[0, 0] + LD(1)  # + 1 / cost, cost = 1
    KZ = ref_kernel_matrix(case, T, Z, X)  # [NPTS][n]

    def qp(p, add):
        """add * Q~ p, Q~_ij = k_ij + QA_cost - q_i - q_j + delta_ij / cost (check_kp's definition)."""
        p = p.astype(LD)
        return LD(add) * (K @ p + (QA - q) * p.sum() - q @ p + p)

    ref = dict(K=K, q=q, QA=QA, KZ=KZ, kp=[qp(inp["P"][0], 1.0), qp(inp["P"][1], -1.0)],
               multi=np.stack([qp(p, 1.0) for p in inp["P"]]),
               dec=KZ @ inp["A"].astype(LD).T + inp["b"].astype(LD), vals=KZ[:, inp["rows"]], kvals=K[:, inp["krows"]])
    for k, v in ref.items():
        assert np.isfinite(np.asarray(v, dtype=LD)).all(), (case.name, k)  # a non-finite reference is a bad case
    return ref


def _sides(case, dt, shift=None, kp=False):
    """The two row sets of the single kernel values and the reference's name for them: the predict points Z against
    the unit-vector classes' rows of X, or (kp) the first m rows of X against those of the rows below m."""
    T = DTYPES[dt]
    inp = _inputs(case, dt)
    X, Z = inp["X"], inp["Z"]
    if shift is not None:  # the data as the kernel sees it: x - c in T
        X, Z = (X - shift).astype(T), (Z - shift).astype(T)
    return (X[:case.m], X[inp["krows"]], "kvals") if kp else (Z, X[inp["rows"]], "vals")


def _envelope(case, dt, shift=None, kp=False):
    """eps_T (1 + gamma (|z|^2 + |x|^2 + 2 |z.x|)) |ref|, Laplacian: eps_T (1 + gamma |z - x|_1) |ref|, for the values
    of the unit-vector classes (kp: for the columns K[:, j] of the unit-vector K.p, X against X); C = 1, no floor."""
    T = DTYPES[dt]
    left, right, name = _sides(case, dt, shift, kp)
    x, z = right.astype(LD), left.astype(LD)
    if case.kernel == "laplacian":
        cond = l1_distances(z, x)
    else:
        cond = (z * z).sum(1)[:, None] + (x * x).sum(1)[None, :] + 2 * np.abs(z @ x.T)
    return LD(np.finfo(T).eps) * (1 + LD(T(case.gamma)) * cond) * np.abs(_reference(case, dt)[name])


def column_means(X, T):
    """The shift of a dense RBF context: column means accumulated in fp64 in row order, rounded to T."""
    c = np.zeros(X.shape[1], dtype=np.float64)
    for row in X[:-1].astype(np.float64):
        c += row
    return (c / max(X.shape[0] - 1, 1)).astype(T)


def _ratio(got, case, dt, shift=None, kp=False):
    """The largest (|got - ref| - tiny_T) / envelope: the C that this result needs."""
    T = DTYPES[dt]
    err = np.abs(got.astype(LD) - _reference(case, dt)["kvals" if kp else "vals"]) - LD(np.finfo(T).tiny)
    env = _envelope(case, dt, shift, kp)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / env, 0)
    return float(r.max())


# ---- the CPU model of the arithmetic (sets C; never the GPU's output) ------------------------------------------------
def _fma(a, b, c, T):
    wide = np.float64 if T == np.float32 else LD
    return (a.astype(wide) * b.astype(wide) + c.astype(wide)).astype(T)


def model_values(case, dt, reverse, shift=None, kp=False):
    """The unit-vector classes' kernel values by the device's formulas in T: sequential fma chains for the dot product
    and the norms, |a|^2 + |b|^2 - 2 a.b clamped at 0, exp; fma(gamma, a.b, coef0) and the power loop; Laplacian
    (q_dense_kernel, l1_acc, kernel_apply): D += |a - b| feature by feature, the difference and the sum each rounded
    to T, then exp(T(-gamma D))."""
    T = DTYPES[dt]
    Z, X, _ = _sides(case, dt, shift, kp)
    order = range(case.d - 1, -1, -1) if reverse else range(case.d)
    if case.kernel == "laplacian":
        D = np.zeros((Z.shape[0], X.shape[0]), dtype=T)
        for k in order:
            D = (D + np.abs((Z[:, k, None] - X[None, :, k]).astype(T))).astype(T)
        return np.exp((-T(case.gamma) * D).astype(T)).astype(T)
    g = np.zeros((Z.shape[0], X.shape[0]), dtype=T)
    nz, nx = np.zeros(Z.shape[0], dtype=T), np.zeros(X.shape[0], dtype=T)
    for k in order:
        g = _fma(np.broadcast_to(Z[:, k, None], g.shape), np.broadcast_to(X[None, :, k], g.shape), g, T)
        nz, nx = _fma(Z[:, k], Z[:, k], nz, T), _fma(X[:, k], X[:, k], nx, T)
    gamma, coef0 = T(case.gamma), T(case.coef0)
    if case.kernel == "rbf":
        dist = (nz[:, None] + nx[None, :]).astype(T) - T(2) * g
        return np.exp(-gamma * np.maximum(dist, T(0))).astype(T)
    base = _fma(np.full_like(g, gamma), g, np.full_like(g, coef0), T)
    r = np.ones_like(base)
    for _ in range(case.degree):
        r = (r * base).astype(T)
    return r


def test_cpu_model_sets_C():
    """The derivation of C_BOUND, rerun: the model's largest ratio per kernel function is the recorded one. RBF cases
    are modelled on the features as given and with the context's shift subtracted, in both feature orders."""
    worst = {"rbf": (0.0, None), "polynomial": (0.0, None), "laplacian": (0.0, None)}
    for case, dt in RUNS:
        if dt == "f64" and LD is np.float64:
            continue  # no wider type to emulate the fp64 fma with
        shifts = [None, column_means(_inputs(case, dt)["X"], DTYPES[dt])] if case.kernel == "rbf" else [None]
        for shift in shifts:
            for reverse in (False, True):
                r = _ratio(model_values(case, dt, reverse, shift), case, dt, shift)
                if r > worst[case.kernel][0]:
                    worst[case.kernel] = (r, f"{case.name}-{dt}")
    print("model ratios:", worst)
    for kernel, (r, _) in worst.items():
        assert 0.5 * C_MODEL[kernel] <= r <= 1.01 * C_MODEL[kernel], worst
        assert C_BOUND[kernel] >= 4 * C_MODEL[kernel]


def test_cpu_model_on_the_kp_values():
    """The cause of KVAL_XFAIL, without a GPU: on the unit-vector K.p's values (X against X) the model of the arithmetic in
    forward feature order needs the C recorded for the GPU's values, to its three digits. The miss is the envelope's."""
    for name, reason in KVAL_XFAIL.items():
        case, dt = next((c, t) for (c, t), i in zip(RUNS, IDS) if i == name)
        if dt == "f64" and LD is np.float64:
            continue
        r = _ratio(model_values(case, dt, False, kp=True), case, dt, kp=True)
        recorded = float(reason.split()[2])
        print(f"{name}: model {r:.4g}, recorded for the GPU {recorded:g}")
        assert abs(r - recorded) <= 0.01 * recorded and r > C_BOUND[case.kernel]


# ---- the reference against the oracle, on the CPU --------------------------------------------------------------------
@pytest.mark.parametrize("case,dt", CONTROL, ids=[f"{c.name}-{dt}" for c, dt in CONTROL])
def test_reference_agrees_with_the_oracle(oracle, case, dt):
    """To the oracle's own precision: it sums n terms sequentially in T, each a kernel value from a d-term chain, so
    its error is at most about (n + d + 10) eps_T of the sum of the terms' magnitudes."""
    T = DTYPES[dt]
    inp, ref = _inputs(case, dt), _reference(case, dt)
    X, m, n = inp["X"], case.m, case.m + 1
    args = dict(degree=case.degree, gamma=T(case.gamma), coef0=T(case.coef0))
    tol = LD((n + case.d + 10) * np.finfo(T).eps)
    data = oracle.Data(X, dtype=T)
    q = oracle.generate_q(case.kernel, data, **args)
    assert np.abs(q - ref["q"]).max() <= tol * np.abs(ref["q"]).max()
    Qabs = np.abs(ref["K"] + ref["QA"] - ref["q"][:, None] - ref["q"][None, :])
    for (p, add), want in zip(((inp["P"][0], 1.0), (inp["P"][1], -1.0)), ref["kp"]):
        got = oracle.kp(case.kernel, data, ref["q"].astype(T), T(ref["QA"]), T(1.0), add, p, **args)
        mag = Qabs @ np.abs(p).astype(LD) + np.abs(p)
        assert (np.abs(got - want) <= tol * mag).all(), np.abs(got - want).max()
    for k in range(R):
        got = oracle.predict(case.kernel, X, inp["A"][k], -inp["b"][k], inp["Z"], **args)
        mag = np.abs(ref["KZ"]) @ np.abs(inp["A"][k]).astype(LD) + abs(LD(inp["b"][k]))
        assert (np.abs(got - ref["dec"][:, k]) <= tol * mag).all(), np.abs(got - ref["dec"][:, k]).max()


# ---- the Laplacian reference and the conditions of its cases, on the CPU (the C oracle does not know the kernel) -------
def _case(name, dt):
    return next(c for c, t in RUNS if c.name == name and t == dt)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_laplacian_reference_anchor(dt):
    """The long-double reference against test_gpu_laplacian's float64 numpy on the control case, to float64's precision
    (a d-term sum, the product with gamma and exp: (d + 10) eps_f64 relative), and on a d = 2 example by hand whose
    differences are binary fractions: distances 3.5, 0 and 0.75 at gamma = 1/2."""
    from test_gpu_laplacian import l1_kernel

    T = DTYPES[dt]
    case = _case("lap_control", dt)
    X, Z = _inputs(case, dt)["X"], _inputs(case, dt)["Z"]
    for A, B in ((X, X), (Z, X)):
        ref, f64 = ref_kernel_matrix(case, T, A, B), l1_kernel(A, B, float(T(case.gamma)))
        assert ref.shape == f64.shape and (ref > 0).all()
        assert (np.abs(f64 - ref) <= (case.d + 10) * np.finfo(np.float64).eps * ref).all(), np.abs(f64 / ref - 1).max()
    hand = Case("by_hand", "laplacian", "unit", 0.5, d=2)
    got = ref_kernel_matrix(hand, T, [[0.5, -1.25]], [[0.25, 2.0], [0.5, -1.25], [1.0, -1.5]])
    want = [LD("0.1737739434504451266807172586663710160147"), LD(1),  # e^-1.75, e^0, e^-0.375
            LD("0.6872892787909721985452023391465135904347")]
    assert got.shape == (1, 3) and got[0, 1] == 1
    assert (np.abs(got[0] - np.array(want, dtype=LD)) <= 2 * np.finfo(LD).eps * np.array(want, dtype=LD)).all(), got


def _denormal_counts(v, T):
    tiny = np.finfo(T).tiny
    return int(((v != 0) & (np.abs(v) < tiny)).sum()), int((np.abs(v) >= tiny).sum()), int((v == 0).sum())


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_laplacian_underflow_case_reaches_the_subnormals(dt):
    """Of the unit-vector classes' 131 x 8 reference values rounded to T, at least a hundred each are subnormal, normal
    and zero (with these seeds 138 / 413 / 497 in fp64 at gamma = 45 and 448 / 226 / 374 in fp32 at gamma = 6)."""
    T = DTYPES[dt]
    with np.errstate(under="ignore"):
        counts = _denormal_counts(_reference(_case("lap_underflow", dt), dt)["vals"].astype(T), T)
    print("subnormal / normal / zero:", counts)
    assert sum(counts) == NPTS * 8 and min(counts) >= 100, counts


def _min_scaled_distance(case, dt):
    """The smallest gamma |x_i - x_j|_1 over the distinct pairs of the case's n points, in LD."""
    D = l1_distances(_inputs(case, dt)["X"], _inputs(case, dt)["X"])
    D[np.diag_indices_from(D)] = np.inf
    return LD(DTYPES[dt](case.gamma)) * D.min()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_laplacian_gamma1e8_case_is_the_identity(dt):
    """Every off-diagonal exponent lies below the last subnormal's (-745 in fp64, -104 in fp32): K is exactly I."""
    case, T = _case("lap_gamma1e8", dt), DTYPES[dt]
    assert _min_scaled_distance(case, dt) > {"f64": 745, "f32": 104}[dt]
    with np.errstate(under="ignore"):
        K = _reference(case, dt)["K"].astype(T)
    assert np.array_equal(K, np.eye(case.m, dtype=T))


# ---- the GPU runs of a case, once ------------------------------------------------------------------------------------
def _tiles(m):
    nb = -(-m // TILE)
    return nb * (nb + 1) // 2


@functools.lru_cache(maxsize=None)
def _gpu(case, dt):
    T = DTYPES[dt]
    inp = _inputs(case, dt)
    m, P = case.m, inp["P"]
    out = {}

    def make(**kw):
        p = pm.Parameter(case.kernel, degree=case.degree, gamma=case.gamma, coef0=case.coef0, cost=1.0, real_type=T)
        p.data = inp["X"]
        svm = pm.CSVM(p, **kw)
        svm.setup_data_on_device()
        return svm

    def kp(svm, c, add):
        return svm.run_device_kernel(None, np.zeros(m, T), P[c], add).copy()

    def kvals(svm):  # (i): column k is K[:, j_k], each element one value of kp_tile_kernel (fma(kv, 1, 0) and exact zeros)
        return np.stack([svm.kp_part(inp["U"][k, :m], "kernel").copy() for k in range(len(inp["krows"]))], axis=1)

    with make(kp_cache=False) as svm:  # (a), (g), (d)
        out["q"], out["QA"] = svm.generate_q().copy(), svm.QA_cost
        out["implicit"] = [kp(svm, 0, 1.0), kp(svm, 1, -1.0)]
        out["implicit_multi"] = svm.run_device_kernel_multi(None, np.zeros((R, m), T), P, 1.0).copy()
        out["kvals_implicit"] = kvals(svm)
        info = svm.info()
        assert info["kp_cache_tiles"] == 0 and info["kp_cache_packed_tiles"] == 0
        out["shift"] = info.get("rbf_shift", 0)
    packs = (True, False) if (case.kernel in ("rbf", "laplacian") and dt == "f64") else (None,)
    tiles_only = case.kernel == "laplacian"  # no rocBLAS predict: PLSSVM_MI_PRED_GEMM has no meaning for this kernel
    for pack in packs:
        tag = {True: "packed", False: "raw", None: "cached"}[pack]
        with make(**({} if pack is None else {"kp_pack": pack})) as svm:
            svm.generate_q()
            assert svm.info()["kp_cache_tiles"] == _tiles(m) and svm.info()["kp_cache_packed_tiles"] == 0
            out[tag + "_fill"] = [kp(svm, 0, 1.0)]  # (b)
            packed = svm.info()["kp_cache_packed_tiles"]
            if pack and case.packed == "all":
                assert packed == _tiles(m)
            elif pack and case.packed == "some":
                assert 0 < packed < _tiles(m)
            elif pack is False or dt == "f32":
                assert packed == 0
            out[tag + "_stream"] = [kp(svm, 0, 1.0), kp(svm, 1, -1.0)]  # (c)
            out[tag + "_multi"] = svm.run_device_kernel_multi(None, np.zeros((R, m), T), P, 1.0).copy()  # (d)
            out[tag + "_kvals"] = kvals(svm)  # (i), streamed
            assert svm.info()["kp_cache_tiles"] == _tiles(m) and svm.info()["kp_cache_packed_tiles"] == packed
            if pack is False:
                continue
            saved = os.environ.pop("PLSSVM_MI_PRED_GEMM", None)
            try:
                for name, algo in (("tiles", _abi.PREDICT_TILES),
                                   ("gemm", _abi.PREDICT_TILES if tiles_only else _abi.PREDICT_GEMM)):
                    if name == "gemm":
                        os.environ["PLSSVM_MI_PRED_GEMM"] = "1"
                    out["dec_" + name] = svm.predict_values_multi(inp["Z"], alphas=inp["A"], biases=inp["b"])  # (e), (f)
                    assert svm.info()["predict_algo"] == algo
                    out["vals_" + name] = svm.predict_values_multi(inp["Z"], alphas=inp["U"],
                                                                   biases=np.zeros(len(inp["rows"])))  # (h)
                    assert svm.info()["predict_algo"] == algo
                    Z = inp["Z"]  # the same points as CSR: densified per chunk on the host, shifted like dense points
                    csr = (np.arange(NPTS + 1, dtype=np.int64) * case.d, np.tile(np.arange(case.d, dtype=np.int32), NPTS),
                           Z.ravel(), NPTS, case.d)
                    out["dec_csr_" + name] = svm.predict_values_multi(csr, alphas=inp["A"], biases=inp["b"])
                    assert svm.info()["predict_algo"] == algo
            finally:
                os.environ.pop("PLSSVM_MI_PRED_GEMM", None)
                if saved is not None:
                    os.environ["PLSSVM_MI_PRED_GEMM"] = saved
    return out


def _summed(got, want, tol, what, failures):
    got = np.asarray(got)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), (what, "not finite")
    err = float(np.abs(got.astype(LD) - want).max() / max(np.abs(want).max(), LD(1e-30)))  # check_kp's floor
    print(f"  {what}: err {err:.3e} of max|ref| (tolerance {tol:g})")
    if not err <= tol:
        failures.append(f"{what}: {err:.3e} > {tol:g}")


# ---- the GPU tests ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_shift_is_active_on_dense_rbf_only(case, dt):
    assert _gpu(case, dt)["shift"] == (1 if case.kernel == "rbf" else 0)


@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_q_and_QA_cost(case, dt):
    print(f"\n[q_and_QA_cost {case.name}-{dt}]")
    got, ref, failures = _gpu(case, dt), _reference(case, dt), []
    _summed(got["q"], ref["q"], KP_TOL[dt], "q", failures)
    _summed(np.array([got["QA"]]), np.array([ref["QA"]]), KP_TOL[dt], "QA_cost", failures)
    if case.kernel == "laplacian":  # k(x, x) = exp(-gamma 0) = 1: QA_cost is exactly 1 + 1 / cost
        X = _inputs(case, dt)["X"]
        assert got["QA"] == 2 and ref["QA"] == 2
        same = np.flatnonzero((X[:case.m] == X[case.m]).all(axis=1))  # rows equal to the last point
        assert same.size == (2 if case.data == "dups" else 0)
        assert (got["q"][same] == 1).all() and (ref["q"][same] == 1).all(), got["q"][same]
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", KP_RUNS)
def test_kp_on_every_path(case, dt):
    print(f"\n[kp_on_every_path {case.name}-{dt}]")
    got, ref, failures = _gpu(case, dt), _reference(case, dt), []
    for tag in ("implicit", "packed_fill", "packed_stream", "raw_fill", "raw_stream", "cached_fill", "cached_stream"):
        for k, g in enumerate(got.get(tag, ())):
            _summed(g, ref["kp"][k], KP_TOL[dt], f"K.p {tag} add={'+-'[k]}1", failures)
    for tag in ("implicit_multi", "packed_multi", "raw_multi", "cached_multi"):
        if tag in got:
            for c in range(R):
                _summed(got[tag][c], ref["multi"][c], KP_TOL[dt], f"K.P {tag} vector {c}", failures)
    assert ("cached_fill" in got) != ("packed_fill" in got and "raw_fill" in got)
    if case.kernel == "laplacian":  # stored tiles in every record form: bitwise the implicit K.p
        for tag in ("packed", "raw", "cached"):
            if tag + "_fill" in got:
                assert np.array_equal(got[tag + "_fill"][0], got["implicit"][0]), tag
                assert all(np.array_equal(g, w) for g, w in zip(got[tag + "_stream"], got["implicit"])), tag
                assert np.array_equal(got[tag + "_multi"], got["implicit_multi"]), tag
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_decision_values(case, dt):
    print(f"\n[decision_values {case.name}-{dt}]")
    got, ref, failures = _gpu(case, dt), _reference(case, dt), []
    for name in ("tiles", "gemm"):
        for k in range(R):
            _summed(got["dec_" + name][:, k], ref["dec"][:, k], DEC_TOL[dt], f"decision values {name} class {k}", failures)
        assert np.array_equal(got["dec_csr_" + name], got["dec_" + name]), name  # CSR points: the same values
    if case.kernel == "laplacian":  # PLSSVM_MI_PRED_GEMM=1 is ignored: the tile kernel both times
        assert np.array_equal(got["dec_gemm"], got["dec_tiles"])
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_single_kernel_values(case, dt):
    print(f"\n[single_kernel_values {case.name}-{dt}]")
    T = DTYPES[dt]
    got, inp, failures = _gpu(case, dt), _inputs(case, dt), []
    shift = column_means(inp["X"], T) if got["shift"] else None
    for name in ("tiles", "gemm"):
        v = got["vals_" + name]
        assert v.shape == (NPTS, len(inp["rows"])) and np.isfinite(v).all(), name
        r = _ratio(v, case, dt, shift)
        print(f"  kernel values {name}: needs C = {r:.3g} (C = {C_BOUND[case.kernel]:g})")
        if not r <= C_BOUND[case.kernel]:
            failures.append(f"kernel values {name}: C {r:.3g} > {C_BOUND[case.kernel]:g}")
    if case.data == "dups":  # a point on the last point: the reference is exactly 1
        assert _reference(case, dt)["vals"][1, -1] == 1
    if case.kernel == "laplacian":
        assert np.array_equal(got["vals_gemm"], got["vals_tiles"])  # PLSSVM_MI_PRED_GEMM=1 is ignored
        on = (inp["Z"][:, None, :] == inp["X"][inp["rows"]][None, :, :]).all(axis=2)  # a point on a support vector
        assert on.sum() == (3 if case.data == "dups" else 0)  # Z[1] = the last point = rows m - 2 and m - 1
        assert (got["vals_tiles"][on] == 1).all(), got["vals_tiles"][on]  # exp(-gamma 0), not a bound
    assert not failures, failures


@gpu
@pytest.mark.parametrize("case,dt", RUNS, ids=IDS)
def test_kp_tile_kernel_values_streamed_and_exact(case, dt):
    """(i): the values kp_tile_kernel forms, one by one. Column k of kvals is kp_part(e_j) for the k-th of the rows
    below m, i.e. K[:, j]: computed (kp_cache=False) and streamed from the stored tiles in every record form, the same
    bits. Laplacian: k(x, x) and the values of equal rows are exp(-gamma 0) = 1, not nearly 1. plssvm_mi_kp_part takes
    one vector, so the batched tile kernel's single values are not reached: its sums are (test_kp_on_every_path)."""
    got, inp = _gpu(case, dt), _inputs(case, dt)
    rows, v = inp["krows"], got["kvals_implicit"]
    assert v.shape == (case.m, len(rows)) and np.isfinite(v).all()
    streamed = [tag for tag in ("packed_kvals", "raw_kvals", "cached_kvals") if tag in got]
    assert len(streamed) == (2 if case.kernel in ("rbf", "laplacian") and dt == "f64" else 1)
    for tag in streamed:
        assert np.array_equal(got[tag], v), tag
    if case.kernel == "laplacian":
        assert (v[rows, np.arange(len(rows))] == 1).all(), v[rows, np.arange(len(rows))]
        X = inp["X"]
        same = (X[:case.m, None, :] == X[rows][None, :, :]).all(axis=2)  # equal rows
        assert same.sum() == len(rows) + (len(rows) if case.data == "dups" else 0)  # dups: every row has one twin below m
        assert (v[same] == 1).all(), v[same]


@gpu
@pytest.mark.parametrize("case,dt", KVAL_RUNS)
def test_kp_tile_kernel_values(case, dt):
    """(i) inside the envelope of the kernel function, X against X, with the C of the predict kernels' values."""
    print(f"\n[kp_tile_kernel_values {case.name}-{dt}]")
    T = DTYPES[dt]
    got, inp = _gpu(case, dt), _inputs(case, dt)
    shift = column_means(inp["X"], T) if got["shift"] else None
    r = _ratio(got["kvals_implicit"], case, dt, shift, kp=True)
    print(f"  K.p tile kernel values: needs C = {r:.3g} (C = {C_BOUND[case.kernel]:g})")
    assert r <= C_BOUND[case.kernel], f"K.p tile kernel values: C {r:.3g} > {C_BOUND[case.kernel]:g}"


@gpu
@pytest.mark.parametrize("case,dt", KSYM_RUNS)
def test_kp_tile_kernel_values_are_symmetric(case, dt):
    """(i) on the rows x rows sub-matrix: K[i, j] and K[j, i] are the same bits. Between two tile rows one tile serves
    both; a diagonal tile forms both (five of the rows share tile 0, two tile 1)."""
    got, rows = _gpu(case, dt), _inputs(case, dt)["krows"]
    sub = got["kvals_implicit"][rows, :]
    asym = np.abs(sub - sub.T).max()
    print(f"\n[kp_tile_kernel_values_are_symmetric {case.name}-{dt}] max |K_ij - K_ji| = {asym:.3g}")
    assert np.array_equal(sub, sub.T), asym


@gpu
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_laplacian_identity_at_gamma1e8(dt):
    """K = I exactly (test_laplacian_gamma1e8_case_is_the_identity): every product of K p is p_j * 0 or p_i * 1, so
    kp_part returns a signed p bit for bit, computed, while filling the cache and streamed from it."""
    case, T = _case("lap_gamma1e8", dt), DTYPES[dt]
    p = np.random.default_rng(11).uniform(-1, 2, case.m).astype(T)
    assert (p < 0).any() and (p > 0).any()
    for cache, calls in ((False, ("implicit",)), (True, ("fill", "stream"))):
        with _context(case, dt, _inputs(case, dt)["X"], kp_cache=cache) as svm:
            svm.setup_data_on_device()
            for what in calls:
                assert np.array_equal(svm.kp_part(p, "kernel"), p), what
            assert svm.info()["kp_cache_tiles"] == (_tiles(case.m) if cache else 0)


# ---- the shift itself ------------------------------------------------------------------------------------------------
def _context(case, dt, X, **kw):
    p = pm.Parameter(case.kernel, degree=case.degree, gamma=case.gamma, coef0=case.coef0, cost=1.0, real_type=DTYPES[dt])
    p.data = X
    return pm.CSVM(p, **kw)


@gpu
def test_a_second_setup_rebuilds_the_shift():
    """Offset 100, then offset 1000 on one context: the second setup's K.p is bitwise a fresh context's."""
    a, b = _case("rbf_offset100", "f64"), _case("rbf_offset1000", "f64")
    p = _inputs(a, "f64")["P"][0]

    def kp(svm):
        svm.setup_data_on_device()
        svm.generate_q()
        return svm.run_device_kernel(None, np.zeros(a.m), p, 1.0).copy()

    with _context(b, "f64", _inputs(b, "f64")["X"]) as svm:
        want = kp(svm)
    with _context(a, "f64", _inputs(a, "f64")["X"]) as svm:
        first = kp(svm)
        svm.params.data = _inputs(b, "f64")["X"]
        second = kp(svm)
        assert svm.info()["rbf_shift"] == 1
    assert np.array_equal(second, want) and not np.array_equal(first, want)
    failures = []
    _summed(second, _reference(b, "f64")["kp"][0], KP_TOL["f64"], "K.p after the second setup", failures)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("world", [2, 3])
def test_simulated_ranks_share_the_shift(world):
    """Every simulated rank holds all of X and forms the same c: the shares sum to the reference's K.p."""
    case = _case("rbf_offset1000", "f64")
    inp = _inputs(case, "f64")
    total = np.zeros(case.m)
    for r in range(world):
        with _context(case, "f64", inp["X"], sim_rank=(r, world)) as svm:
            svm.setup_data_on_device()
            svm.generate_q()
            assert svm.info()["rbf_shift"] == 1
            total += svm.run_device_kernel(None, np.zeros(case.m), inp["P"][0], 1.0)
    failures = []
    _summed(total, _reference(case, "f64")["kp"][0], KP_TOL["f64"], f"K.p summed over {world} simulated ranks", failures)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_update_w_returns_the_callers_features(dt):
    """w = sum_i alpha_i x_i on a shifted context is that of the features as given, to the rounding of the sum."""
    case, T = _case("rbf_offset100", dt), DTYPES[dt]
    inp = _inputs(case, dt)
    alpha = inp["A"][0]
    with _context(case, dt, inp["X"]) as svm:
        w = svm.update_w(alpha)
        assert svm.info()["rbf_shift"] == 1
    want = inp["X"].astype(LD).T @ alpha.astype(LD)
    mag = np.abs(inp["X"]).astype(LD).T @ np.abs(alpha).astype(LD)
    assert (np.abs(w - want) <= (case.m + 10) * np.finfo(T).eps * mag).all(), np.abs(w - want).max()
