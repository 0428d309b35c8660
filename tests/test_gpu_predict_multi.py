"""GPU tests of the fused dense predict (csrc/predict_tiles.hip) behind plssvm_mi_predict_multi_dense / _csr: every
class of a one-vs-all model in one pass over the kernel values.

1. parity with the oracle's predict per class, at the tolerances of tests/test_gpu_predict.py (1e-10 fp64 / 1e-4 fp32
   of max|ref|), on the fused kernel and on the rocBLAS path (PLSSVM_MI_PRED_GEMM=1);
2. the contract, bitwise: a decision value depends only on the model and the point — not on the number of classes,
   the class's row, the number or order of the points, the chunking (PLSSVM_MI_PRED_CHUNK), the run or the leading
   dimensions;
3. exact integer arithmetic (the MFMA fragment layout: any swapped row or column changes an integer);
4. argument errors leave the context usable;
5. sparse and linear contexts run the classes through the single-class paths, bitwise.
"""
import ctypes
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
SEG_ROWS = _abi.PREDICT_SEG_TILES * 128  # support vectors per workgroup segment
# (n, np, d, K); the last: m = n - 1 spans three segments, the third with one full and one ragged (2-row) tile
SHAPES = [(1, 3, 4, 2), (2, 1, 1, 1), (128, 129, 24, 3), (129, 128, 24, 8), (130, 300, 257, 9),
          (2 * SEG_ROWS + 131, 130, 24, 3)]
KERNELS = ["polynomial", "rbf"]
DTYPES = [np.float64, np.float32]


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def _inputs(n, npts, d, K, dtype):
    X, _ = datagen.blobs(n, d, seed=41, dtype=dtype)
    Z, _ = datagen.blobs(npts, d, seed=42, dtype=dtype)
    rng = np.random.default_rng(43)
    A = rng.standard_normal((K, n)).astype(dtype)
    b = rng.standard_normal(K).astype(dtype)
    for a in (X, Z, A, b):
        a.setflags(write=False)
    return X, Z, A, b


def _param(kernel, d, dtype):
    return pm.Parameter(kernel, gamma=1.0 / d, coef0=1.0 if kernel == "polynomial" else 0.0, real_type=dtype)


def _svm(kernel, X, dtype):
    p = _param(kernel, X.shape[1], dtype)
    p.data = X
    svm = pm.CSVM(p)
    svm.setup_data_on_device()
    return svm


@functools.lru_cache(maxsize=None)
def _reference(kernel, n, npts, d, K, dtype):
    from oracle import pyoracle

    pyoracle.build()
    X, Z, A, b = _inputs(n, npts, d, K, dtype)
    coef0 = dtype(1.0 if kernel == "polynomial" else 0.0)
    ref = np.stack([pyoracle.predict(kernel, X, A[k], -b[k], Z, gamma=dtype(1.0 / d), coef0=coef0) for k in range(K)], axis=1)
    ref.setflags(write=False)
    return ref


# ---- 1. parity with the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("gemm", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_oracle(shape, kernel, dtype, gemm, monkeypatch):
    n, npts, d, K = shape
    X, Z, A, b = _inputs(n, npts, d, K, dtype)
    ref = _reference(kernel, n, npts, d, K, dtype)
    if gemm:
        monkeypatch.setenv("PLSSVM_MI_PRED_GEMM", "1")
    with _svm(kernel, X, dtype) as svm:
        assert svm.info()["predict_algo"] == _abi.PREDICT_NONE
        V = svm.predict_values_multi(Z, alphas=A, biases=b)
        assert svm.info()["predict_algo"] == (_abi.PREDICT_GEMM if gemm else _abi.PREDICT_TILES)
    assert V.shape == (npts, K) and V.dtype == dtype
    for k in range(K):
        err = np.abs(V[:, k] - ref[:, k]).max() / np.abs(ref[:, k]).max()
        print(f"shape {shape} {kernel} {np.dtype(dtype).name} gemm={gemm} class {k}: err {err:.3e}")
        assert err <= TOL[dtype], (k, err)


# ---- 2. the contract -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_contract_bitwise(kernel, dtype, monkeypatch):
    n, npts, d, K = 130, 300, 257, 9
    X, Z, A, b = _inputs(n, npts, d, K, dtype)
    with _svm(kernel, X, dtype) as svm:
        V = svm.predict_values_multi(Z, alphas=A, biases=b)
        # the single entry point, per class
        for k in range(K):
            assert np.array_equal(V[:, k], svm.predict_values(Z, A[k], b[k])), k
        # nclass: 9 classes (two passes) against their first 8 and their last one
        assert np.array_equal(V[:, :8], svm.predict_values_multi(Z, alphas=A[:8], biases=b[:8]))
        assert np.array_equal(V[:, 8:], svm.predict_values_multi(Z, alphas=A[8:], biases=b[8:]))
        # the class's row
        order = np.array([4, 0, 8, 2, 1, 3, 7, 6, 5])
        assert np.array_equal(V[:, order], svm.predict_values_multi(Z, alphas=A[order], biases=b[order]))
        # the points' number and order
        perm = np.random.default_rng(5).permutation(npts)
        assert np.array_equal(V[perm], svm.predict_values_multi(Z[perm], alphas=A, biases=b))
        assert np.array_equal(V[:1], svm.predict_values_multi(Z[:1], alphas=A, biases=b))
        # the chunking: 128 + 128 + 44 points
        monkeypatch.setenv("PLSSVM_MI_PRED_CHUNK", "128")
        assert np.array_equal(V, svm.predict_values_multi(Z, alphas=A, biases=b))
        monkeypatch.delenv("PLSSVM_MI_PRED_CHUNK")
        # the run
        assert np.array_equal(V, svm.predict_values_multi(Z, alphas=A, biases=b))
        # the leading dimensions: NaN past n in ALPHA is never read, OUT keeps its sentinels past np
        L = _abi.lib()
        Ap = np.full((K, n + 5), np.nan, dtype=dtype)
        Ap[:, :n] = A
        out = np.full((K, npts + 3), 77.0, dtype=dtype)
        b64 = np.ascontiguousarray(b, dtype=np.float64)
        assert L.plssvm_mi_predict_multi_dense(svm._ctx, ptr(Ap), K, n + 5, ptr(b64), ptr(np.ascontiguousarray(Z)), npts, d,
                                               ptr(out), npts + 3) == 0
        assert np.array_equal(out[:, :npts].T, V)
        assert np.all(out[:, npts:] == 77.0)


def test_contract_across_segments():
    """The three-segment model: the multi call, the single calls and a one-point call agree bitwise."""
    n, npts, d, K = SHAPES[-1]
    X, Z, A, b = _inputs(n, npts, d, K, np.float64)
    with _svm("rbf", X, np.float64) as svm:
        V = svm.predict_values_multi(Z, alphas=A, biases=b)
        assert np.array_equal(V[:, 1], svm.predict_values(Z, A[1], b[1]))
        assert np.array_equal(V[129:], svm.predict_values_multi(Z[129:], alphas=A, biases=b))


# ---- 3. exact arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_integers(dtype):
    """poly, degree 2, gamma 1, coef0 1 on integer features in [-2, 2] (d = 20) and integer alphas in [-3, 3]
    (n = 300): |x . z| <= 80, (1 + x . z)^2 <= 6561, |sum| <= 300 * 3 * 6561 < 2^24 — every product and partial sum
    is an integer below 2^24, exact in both real types in any order, so the result must equal the int64 one."""
    n, npts, d, K = 300, 150, 20, 3
    rng = np.random.default_rng(9)
    X = rng.integers(-2, 3, size=(n, d))
    Z = rng.integers(-2, 3, size=(npts, d))
    A = rng.integers(-3, 4, size=(K, n))
    want = ((1 + Z @ X.T) ** 2) @ A.T  # int64 [np][K]
    p = pm.Parameter("polynomial", degree=2, gamma=1.0, coef0=1.0, real_type=dtype)
    p.data = X.astype(dtype)
    with pm.CSVM(p) as svm:
        V = svm.predict_values_multi(Z.astype(dtype), alphas=A.astype(dtype), biases=np.zeros(K))
        assert svm.info()["predict_algo"] == _abi.PREDICT_TILES
    assert np.array_equal(V.astype(np.int64), want) and np.array_equal(V, want.astype(dtype))


# ---- 4. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable():
    n, npts, d, K = 129, 128, 24, 8
    X, Z, A, b = _inputs(n, npts, d, K, np.float64)
    A, Z = np.ascontiguousarray(A), np.ascontiguousarray(Z)
    b64 = np.ascontiguousarray(b, dtype=np.float64)
    L = _abi.lib()
    rowptr = np.arange(npts + 1, dtype=np.int64)
    col = np.zeros(npts, dtype=np.int32)
    val = np.ones(npts)
    with _svm("rbf", X, np.float64) as svm:
        out = np.zeros((K, npts))
        base = dict(ctx=svm._ctx, A=ptr(A), K=K, lda=n, b=ptr(b64), Z=ptr(Z), r=ptr(rowptr), c=ptr(col), v=ptr(val),
                    fmt=_abi.VAL_REAL, np=npts, d=d, out=ptr(out), ldo=npts)

        def dense(**kw):
            a = {**base, **kw}
            return L.plssvm_mi_predict_multi_dense(*[a[k] for k in ("ctx", "A", "K", "lda", "b", "Z", "np", "d", "out", "ldo")])

        def csr(**kw):
            a = {**base, **kw}
            return L.plssvm_mi_predict_multi_csr(*[a[k] for k in ("ctx", "A", "K", "lda", "b", "r", "c", "v", "fmt", "np", "d",
                                                                  "out", "ldo")])

        for call in (dense, csr):
            assert call(K=0) == -1
            assert call(K=-1) == -1
            assert call(A=None) == -1
            assert call(b=None) == -1
            assert call(out=None) == -1
            assert call(lda=n - 1) == -1
            assert call(ldo=npts - 1) == -1
        assert dense(Z=None) == -1
        assert csr(r=None) == -1
        assert csr(c=None) == -1
        assert dense(np=0, Z=None, out=None) == 0  # no points: a no-op
        assert csr(np=0, r=None, c=None, v=None, out=None) == 0
        assert np.all(out == 0.0)
        assert dense() == 0  # the context is still usable
        want = svm.predict_values_multi(Z, alphas=A, biases=b)
        assert np.array_equal(out.T, want)
        out2 = out.copy()
        out[:] = 0
        assert csr() == 0  # CSR points on the dense context: the same kernel
        assert svm.info()["predict_algo"] == _abi.PREDICT_TILES
        Zc = np.zeros((npts, d))
        Zc[:, 0] = 1.0
        assert np.array_equal(out.T, svm.predict_values_multi(Zc, alphas=A, biases=b))
        assert not np.array_equal(out, out2)


# ---- 5. sparse and linear contexts -----------------------------------------------------------------------------------
def test_sparse_context_runs_the_classes_one_after_another():
    n, d, K = 600, 400, 3
    csr, _ = datagen.sparse_csr(n, d, 12, seed=51, dtype=np.float64)
    zc, _ = datagen.sparse_csr(70, d, 12, seed=52, dtype=np.float64)
    rng = np.random.default_rng(53)
    A, b = rng.standard_normal((K, n)), rng.standard_normal(K)
    p = pm.Parameter("rbf", gamma=1.0 / d)
    p.csr = csr
    with pm.CSVM(p) as svm:
        V = svm.predict_values_multi(zc, alphas=A, biases=b)
        algo = svm.info()["predict_algo"]
        assert algo in (_abi.PREDICT_EXPANSION, _abi.PREDICT_BRUTE)
        for k in range(K):
            assert np.array_equal(V[:, k], svm.predict_values(zc, A[k], b[k])), k
            assert svm.info()["predict_algo"] == algo
    assert V.shape == (70, K)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_context_runs_the_classes_one_after_another(dtype):
    n, npts, d, K = 130, 300, 257, 9
    X, Z, A, b = _inputs(n, npts, d, K, dtype)
    with _svm("linear", X, dtype) as svm:
        V = svm.predict_values_multi(Z, alphas=A, biases=b)
        assert svm.info()["predict_algo"] == _abi.PREDICT_LINEAR
        for k in range(K):
            assert np.array_equal(V[:, k], svm.predict_values(Z, A[k], b[k])), k
