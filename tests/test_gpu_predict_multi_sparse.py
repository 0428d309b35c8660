"""GPU tests of the shared multi-class predict on sparse data and on linear models (csrc/predict.hip predict_shared,
csrc/expand.hip exp_pred_point_kernel) behind plssvm_mi_predict_multi_dense / _csr: the points are prepared once and up
to 8 classes share every pass over the support vectors.

1. parity per class with the oracle's predict, at the tolerances of tests/test_gpu_predict.py (1e-10 fp64 / 1e-4 fp32
   of max|ref|), on the expansion, the brute-force sweep (PLSSVM_MI_PRED_BRUTE=1) and the linear w path (factored SELL
   and Gram-mode contexts), with an empty point, an empty support vector, ragged blocks and chunks, K in {1, 3, 8, 9};
2. bitwise: column k is predict_values with class k; the matrix is the one of PLSSVM_MI_PRED_SEQ=1 (the classes one
   after another); neither the points' order or number, nor the class's row, nor the number of classes matters;
3. predict_stats(): [min(K, 8), 1] shared, [1, K] sequential, predict_algo the same either way;
4. the fallbacks from the expansion to brute force are taken for all classes together;
5. the per-class sums carried across two bitmap passes of the expansion (more than 786 432 support vectors);
6. exact integer arithmetic: a swapped class or row changes an integer;
7. argument errors leave a sparse context usable.
"""
import ctypes
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen, fp22

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
DTYPES = [np.float64, np.float32]
N, D, NNZ, NP = 600, 400, 12, 70  # m = 599: three 256-row blocks, the last ragged; two 64-point chunks, the second ragged
KS = [1, 3, 8, 9]                  # 9: two class passes
# name: (kernel, PLSSVM_MI_PRED_BRUTE, CSVM arguments, predict_algo)
PATHS = {
    "rbf-expansion": ("rbf", False, dict(sparse_algo="expansion"), _abi.PREDICT_EXPANSION),
    "poly-expansion": ("polynomial", False, dict(sparse_algo="expansion"), _abi.PREDICT_EXPANSION),
    "rbf-brute": ("rbf", True, dict(sparse_algo="expansion"), _abi.PREDICT_BRUTE),
    "poly-brute": ("polynomial", True, dict(sparse_algo="expansion"), _abi.PREDICT_BRUTE),
    "linear-factored": ("linear", False, dict(kp_mode="factored"), _abi.PREDICT_LINEAR),
    "linear-gram": ("linear", False, dict(kp_mode="pairwise"), _abi.PREDICT_LINEAR),
}


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def without_row(csr, i):
    """The CSR set with row i emptied."""
    rowptr, col, val, n, d = csr
    keep = np.ones(col.size, dtype=bool)
    keep[rowptr[i]:rowptr[i + 1]] = False
    cnt = np.diff(rowptr)
    cnt[i] = 0
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), col[keep], val[keep], n, d


def rows_of(csr, idx):
    """The CSR set of the rows idx, in that order."""
    rowptr, col, val, _, d = csr
    sel = np.concatenate([np.arange(rowptr[i], rowptr[i + 1]) for i in idx]) if len(idx) else np.zeros(0, dtype=np.int64)
    cnt = np.diff(rowptr)[idx]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), col[sel], val[sel], len(idx), d


@functools.lru_cache(maxsize=None)
def _inputs(dtype):
    """The model (support vector 17 empty), the points (point 5 empty), 9 classes."""
    X, _ = datagen.sparse_csr(N, D, NNZ, seed=61, dtype=dtype)
    Zc, _ = datagen.sparse_csr(NP, D, NNZ, seed=62, dtype=dtype)
    X, Zc = without_row(X, 17), without_row(Zc, 5)
    rng = np.random.default_rng(63)
    A = rng.standard_normal((max(KS), N)).astype(dtype)
    b = rng.standard_normal(max(KS)).astype(dtype)
    for a in (*X[:3], *Zc[:3], A, b):
        a.setflags(write=False)
    return X, Zc, A, b


def _params(kernel, dtype):
    return dict(gamma=dtype(1.0 / D), coef0=dtype(0.5))


@functools.lru_cache(maxsize=None)
def _reference(kernel, dtype):
    from oracle import pyoracle

    pyoracle.build()
    X, Zc, A, b = _inputs(dtype)
    Xd, Zd = datagen.densify(X), datagen.densify(Zc)
    ref = np.stack([pyoracle.predict(kernel, Xd, A[k], -b[k], Zd, **_params(kernel, dtype)) for k in range(max(KS))], axis=1)
    ref.setflags(write=False)
    return ref


def _svm(kernel, csr, dtype, val_fmt=None, **kw):
    p = pm.Parameter(kernel, gamma=1.0 / csr[4], coef0=0.5, real_type=dtype)
    p.csr = csr
    if val_fmt is not None:
        p.val_fmt = val_fmt
    svm = pm.CSVM(p, **kw)
    svm.setup_data_on_device()
    return svm


def _path(name, monkeypatch):
    kernel, brute, kw, algo = PATHS[name]
    if brute:
        monkeypatch.setenv("PLSSVM_MI_PRED_BRUTE", "1")
    return kernel, kw, algo


# ---- 1. parity with the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", list(PATHS))
def test_parity_with_the_oracle(path, dtype, K, monkeypatch):
    kernel, kw, algo = _path(path, monkeypatch)
    X, Zc, A, b = _inputs(dtype)
    ref = _reference(kernel, dtype)
    with _svm(kernel, X, dtype, **kw) as svm:
        V = svm.predict_values_multi(Zc, alphas=A[:K], biases=b[:K])
        assert svm.info()["predict_algo"] == algo
    assert V.shape == (NP, K) and V.dtype == dtype
    for k in range(K):
        err = np.abs(V[:, k] - ref[:, k]).max() / np.abs(ref[:, k]).max()
        print(f"{path} {np.dtype(dtype).name} K={K} class {k}: err {err:.3e}")
        assert err <= TOL[dtype], (k, err)


def test_parity_fp22_points_and_model():
    from oracle import pyoracle

    pyoracle.build()
    dtype, K = np.float32, 3
    X, Zc, A, b = _inputs(dtype)
    Xd = datagen.densify((X[0], X[1], fp22.unpack(fp22.pack(X[2]), X[2].size), N, D))
    Zd = datagen.densify((Zc[0], Zc[1], fp22.unpack(fp22.pack(Zc[2]), Zc[2].size), NP, D))
    with _svm("rbf", (X[0], X[1], fp22.pack(X[2]), N, D), dtype, val_fmt=_abi.VAL_FP22) as svm:
        pts = (Zc[0], Zc[1], fp22.pack(Zc[2]), NP, D)
        V = svm.predict_values_multi(pts, val_fmt=_abi.VAL_FP22, alphas=A[:K], biases=b[:K])
        assert svm.predict_stats() == [K, 1]
        for k in range(K):
            ref = pyoracle.predict("rbf", Xd, A[k], -b[k], Zd, **_params("rbf", dtype))
            err = np.abs(V[:, k] - ref).max() / np.abs(ref).max()
            print(f"fp22 class {k}: err {err:.3e}")
            assert err <= TOL[dtype], (k, err)
            assert np.array_equal(V[:, k], svm.predict_values(pts, A[k], b[k], val_fmt=_abi.VAL_FP22)), k


# ---- 2. bitwise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", list(PATHS))
def test_bitwise(path, dtype, monkeypatch):
    kernel, kw, algo = _path(path, monkeypatch)
    X, Zc, A, b = _inputs(dtype)
    K = 9
    with _svm(kernel, X, dtype, **kw) as svm:
        V = svm.predict_values_multi(Zc, alphas=A, biases=b)
        assert svm.info()["predict_algo"] == algo
        # the single entry point and the one-class multi call, per class
        for k in range(K):
            assert np.array_equal(V[:, k], svm.predict_values(Zc, A[k], b[k])), k
            assert np.array_equal(V[:, k:k + 1], svm.predict_values_multi(Zc, alphas=A[k:k + 1], biases=b[k:k + 1])), k
        # the classes one after another
        monkeypatch.setenv("PLSSVM_MI_PRED_SEQ", "1")
        assert np.array_equal(V, svm.predict_values_multi(Zc, alphas=A, biases=b))
        monkeypatch.delenv("PLSSVM_MI_PRED_SEQ")
        # a permutation and a subset of the points (one chunk instead of two)
        perm = np.random.default_rng(7).permutation(NP)
        assert np.array_equal(V[perm], svm.predict_values_multi(rows_of(Zc, perm), alphas=A, biases=b))
        sub = np.array([66, 5, 64, 0])
        assert np.array_equal(V[sub], svm.predict_values_multi(rows_of(Zc, sub), alphas=A, biases=b))
        # the class's row (class 8 moves from the second pass into the first)
        order = np.array([4, 0, 8, 2, 1, 3, 7, 6, 5])
        assert np.array_equal(V[:, order], svm.predict_values_multi(Zc, alphas=A[order], biases=b[order]))
        # dense points on the sparse context: the same values
        assert np.array_equal(V, svm.predict_values_multi(datagen.densify(Zc), alphas=A, biases=b))


# ---- 3. predict_stats ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("path", list(PATHS))
def test_predict_stats(path, K, monkeypatch):
    kernel, kw, algo = _path(path, monkeypatch)
    X, Zc, A, b = _inputs(np.float64)
    with _svm(kernel, X, np.float64, **kw) as svm:
        assert svm.predict_stats() == [0, 0]
        svm.predict_values_multi(Zc, alphas=A[:K], biases=b[:K])
        assert svm.predict_stats() == [min(K, 8), 1]
        assert svm.info()["predict_algo"] == algo
        monkeypatch.setenv("PLSSVM_MI_PRED_SEQ", "1")
        svm.predict_values_multi(Zc, alphas=A[:K], biases=b[:K])
        assert svm.predict_stats() == [1, K]
        assert svm.info()["predict_algo"] == algo
        monkeypatch.delenv("PLSSVM_MI_PRED_SEQ")
        svm.predict_values(Zc, A[0], b[0])
        assert svm.predict_stats() == [1, 1]


# ---- 4. fallbacks, for all classes together --------------------------------------------------------------------------
def _check_fallback(X, Zc, dtype):
    K = 3
    rng = np.random.default_rng(71)
    A, b = rng.standard_normal((K, X[3])).astype(dtype), rng.standard_normal(K).astype(dtype)
    with _svm("rbf", X, dtype, sparse_algo="expansion") as svm:
        assert svm.info()["sparse_algo"] == _abi.SPARSE_EXPANSION
        V = svm.predict_values_multi(Zc, alphas=A, biases=b)
        assert svm.info()["predict_algo"] == _abi.PREDICT_BRUTE
        assert svm.predict_stats() == [K, 1]
        for k in range(K):
            assert np.array_equal(V[:, k], svm.predict_values(Zc, A[k], b[k])), k
            assert svm.info()["predict_algo"] == _abi.PREDICT_BRUTE
    assert np.all(np.isfinite(V))


def test_fallback_point_longer_than_the_lds_capacity():
    """One point with 2060 entries (more than the 2048 the expansion holds per point) among ordinary ones."""
    d = 2100
    X, _ = datagen.sparse_csr(N, d, NNZ, seed=72, dtype=np.float64)
    Zc, _ = datagen.sparse_csr(6, d, NNZ, seed=73, dtype=np.float64)
    rng = np.random.default_rng(74)
    rowptr, col, val, _, _ = Zc
    lcol = np.sort(rng.choice(d, size=2060, replace=False)).astype(np.int32)
    lval = rng.uniform(-0.1, 0.1, size=2060)
    cut = rowptr[3]  # the long point becomes point 3 of 7
    Zl = (np.concatenate([rowptr[:4], rowptr[3:] + 2060]).astype(np.int64), np.concatenate([col[:cut], lcol, col[cut:]]),
          np.concatenate([val[:cut], lval, val[cut:]]), 7, d)
    assert np.diff(Zl[0]).max() == 2060
    _check_fallback(X, Zl, np.float64)


def test_fallback_repeat_rows_overflow_the_list():
    """A dense-ish model: a point shares two or more features with more than 4096 support vectors."""
    n, d, k = 5000, 64, 16
    X, _ = datagen.sparse_csr(n, d, k, seed=75, dtype=np.float32)
    Zc, _ = datagen.sparse_csr(20, d, k, seed=76, dtype=np.float32)
    PX = (datagen.densify(X) != 0).astype(np.int64)[: n - 1]  # the last point is kept apart from the expansion
    PZ = (datagen.densify(Zc) != 0).astype(np.int64)
    assert ((PZ @ PX.T >= 2).sum(axis=1) > 4096).any()
    _check_fallback(X, Zc, np.float32)


# ---- 5. two bitmap passes --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_pass_inputs():
    n, d, k = 800_000, 20_000, 10  # more than the 786 432 rows of one bitmap pass
    X, _ = datagen.sparse_csr(n, d, k, seed=31, dtype=np.float32)
    Zc, _ = datagen.sparse_csr(64, d, k, seed=32, dtype=np.float32)
    rng = np.random.default_rng(81)
    return X, Zc, rng.standard_normal((3, n)).astype(np.float32), rng.standard_normal(3).astype(np.float32)


def test_class_sums_carried_across_two_bitmap_passes():
    X, Zc, A, b = _two_pass_inputs()
    with _svm("rbf", X, np.float32) as svm:
        assert svm.info()["sparse_algo"] == _abi.SPARSE_EXPANSION
        V = svm.predict_values_multi(Zc, alphas=A, biases=b)
        assert svm.info()["predict_algo"] == _abi.PREDICT_EXPANSION
        assert svm.predict_stats() == [3, 1]
        for k in range(3):
            assert np.array_equal(V[:, k], svm.predict_values(Zc, A[k], b[k])), k
    assert len({V[:, k].tobytes() for k in range(3)}) == 3


# ---- 6. exact arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brute", [False, True])
def test_exact_integers(brute, monkeypatch):
    """poly, degree 2, gamma 1, coef0 1 on nonzero integer features in [-2, 2] (12 per row) and integer alphas in
    [-3, 3] (n = 600), integer biases: |x . z| <= 48, (1 + x . z)^2 <= 2401, every moment, product and partial sum is an
    integer far below 2^53 — exact in fp64 in any order, so every class's value must equal the int64 one."""
    K = 3
    rng = np.random.default_rng(91)
    X, _ = datagen.sparse_csr(N, D, NNZ, seed=92, dtype=np.float64)
    Zc, _ = datagen.sparse_csr(NP, D, NNZ, seed=93, dtype=np.float64)
    ints = np.array([-2.0, -1.0, 1.0, 2.0])
    X = (X[0], X[1], rng.choice(ints, size=X[2].size), N, D)
    Zc = (Zc[0], Zc[1], rng.choice(ints, size=Zc[2].size), NP, D)
    A = rng.integers(-3, 4, size=(K, N))
    b = np.array([5, -7, 11])
    G = datagen.densify(Zc).astype(np.int64) @ datagen.densify(X).astype(np.int64).T
    want = ((1 + G) ** 2) @ A.T + b  # int64 [np][K]
    if brute:
        monkeypatch.setenv("PLSSVM_MI_PRED_BRUTE", "1")
    p = pm.Parameter("polynomial", degree=2, gamma=1.0, coef0=1.0, real_type=np.float64)
    p.csr = X
    with pm.CSVM(p, sparse_algo="expansion") as svm:
        V = svm.predict_values_multi(Zc, alphas=A.astype(np.float64), biases=b.astype(np.float64))
        assert svm.info()["predict_algo"] == (_abi.PREDICT_BRUTE if brute else _abi.PREDICT_EXPANSION)
    assert np.array_equal(V, want.astype(np.float64))


# ---- 7. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_sparse_context_usable():
    X, Zc, A, b = _inputs(np.float64)
    K = 3
    A3, b64 = np.ascontiguousarray(A[:K]), np.ascontiguousarray(b[:K], dtype=np.float64)
    Zd = datagen.densify(Zc)
    L = _abi.lib()
    with _svm("rbf", X, np.float64, sparse_algo="expansion") as svm:
        out = np.zeros((K, NP))
        base = dict(ctx=svm._ctx, A=ptr(A3), K=K, lda=N, b=ptr(b64), Z=ptr(Zd), r=ptr(Zc[0]), c=ptr(Zc[1]), v=ptr(Zc[2]),
                    fmt=_abi.VAL_REAL, np=NP, d=D, out=ptr(out), ldo=NP)

        def dense(**kw):
            a = {**base, **kw}
            return L.plssvm_mi_predict_multi_dense(*[a[k] for k in ("ctx", "A", "K", "lda", "b", "Z", "np", "d", "out", "ldo")])

        def csr(**kw):
            a = {**base, **kw}
            return L.plssvm_mi_predict_multi_csr(*[a[k] for k in ("ctx", "A", "K", "lda", "b", "r", "c", "v", "fmt", "np", "d",
                                                                  "out", "ldo")])

        for call in (dense, csr):
            assert call(K=0) == -1
            assert call(b=None) == -1
            assert call(lda=N - 1) == -1
            assert call(ldo=NP - 1) == -1
        assert np.all(out == 0.0)
        assert L.plssvm_mi_get_predict_stats(svm._ctx, None) == -1
        assert csr() == 0  # the context is still usable
        assert svm.predict_stats() == [K, 1]
        assert np.array_equal(out.T, svm.predict_values_multi(Zc, alphas=A3, biases=b[:K]))
