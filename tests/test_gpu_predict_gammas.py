"""GPU tests of the gamma lanes of predict (csrc/predict_gamma.hip) behind plssvm_mi_predict_gammas_dense /
CSVM.predict_values_gammas: up to 8 (gamma, alpha, bias) models share one pass over the pair distances.

1. parity with float64 numpy (direct distances on the data as the real type holds it), the predict bar of
   tests/test_gpu_predict.py: 1e-10 (fp64) / 1e-4 (fp32) of max|ref| per lane;
2. the contract, bitwise: column l is predict_values on a fresh context created with gammas[l], and depends on nothing
   but that lane's model and the point;
3. learn_gammas' models are the defaults;
4. refusals and argument errors leave the context usable.
Shapes (n, np, d, lanes): one tile and one lane; m = 128, an exactly full tile, LW = 4 with a dead slot; ragged tiles,
d off the chunk depth, two lane groups 8 + 1; three segments, the last ragged.
"""
import ctypes
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
SEG_ROWS = _abi.PREDICT_SEG_TILES * 128
SHAPES = [(2, 1, 1, 1), (129, 128, 24, 3), (130, 300, 257, 9), (2 * SEG_ROWS + 131, 130, 24, 2)]
KERNELS = ["rbf", "laplacian"]
DTYPES = [np.float64, np.float32]


@functools.lru_cache(maxsize=None)
def _inputs(n, npts, d, K, dtype, offset=0.0):
    X, y = datagen.blobs(n, d, seed=41, dtype=dtype)
    Z, _ = datagen.blobs(npts, d, seed=42, dtype=dtype)
    X, Z = (X + dtype(offset)).astype(dtype), (Z + dtype(offset)).astype(dtype)
    rng = np.random.default_rng(43)
    A = rng.standard_normal((K, n)).astype(dtype)
    b = rng.standard_normal(K).astype(dtype)
    g = np.geomspace(0.25 / d, 4.0 / d, K).astype(dtype).astype(np.float64)  # distinct, as the device holds them
    for a in (X, Z, A, b, g, y):
        a.setflags(write=False)
    return X, Z, A, b, g, y


def _svm(kernel, X, gamma, dtype, labels=None, **kw):
    p = pm.Parameter(kernel, gamma=float(gamma), real_type=dtype)
    p.data, p.labels = X, labels
    svm = pm.CSVM(p, **kw)
    svm.setup_data_on_device()
    return svm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_and_fresh_context(shape, kernel, dtype):
    X, Z, A, b, g, _ = _inputs(*shape, dtype)
    diff = Z.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]
    D = (diff ** 2).sum(-1) if kernel == "rbf" else np.abs(diff).sum(-1)  # [np][n]
    with _svm(kernel, X, 1.0 / shape[2], dtype) as svm:
        V = svm.predict_values_gammas(Z, g, A, b)
        assert svm.info()["predict_algo"] == _abi.PREDICT_TILES and svm.predict_stats() == [min(shape[3], 8), 1]
    assert V.shape == (shape[1], shape[3]) and V.dtype == dtype
    for l in range(shape[3]):
        ref = np.exp(-g[l] * D) @ A[l].astype(np.float64) + float(b[l])
        err = np.abs(V[:, l] - ref).max() / np.abs(ref).max()
        print(f"lane {l} gamma {g[l]:.3g}: rel err {err:.3e}")
        assert err <= TOL[dtype], (l, err)
        with _svm(kernel, X, g[l], dtype) as one:
            assert np.array_equal(V[:, l], one.predict_values(Z, A[l], b[l])), l


# offset 50: data off the origin, so that the rbf centring shift of the points is exercised
@pytest.mark.parametrize("kernel,dtype,offset", [(k, t, 0.0) for k in KERNELS for t in DTYPES] + [("rbf", t, 50.0) for t in DTYPES])
def test_value_depends_on_the_lane_and_the_point_only(kernel, dtype, offset, monkeypatch):
    n, npts, d, K = SHAPES[2]
    X, Z, A, b, g, _ = _inputs(n, npts, d, K, dtype, offset)
    with _svm(kernel, X, 1.0 / d, dtype) as svm:
        own, tiles = svm.predict_values(Z, A[0], b[0]), svm.info()["kp_cache_tiles"]
        V = svm.predict_values_gammas(Z, g, A, b)
        assert np.isfinite(V).all() and np.abs(V).max() > 0
        if offset:
            with _svm(kernel, X, g[4], dtype) as one:
                assert np.array_equal(V[:, 4], one.predict_values(Z, A[4], b[4]))
        assert np.array_equal(svm.predict_values_gammas(Z, g, A, b), V)  # the run
        assert np.array_equal(svm.predict_values_gammas(Z, g[:8], A[:8], b[:8]), V[:, :8])  # the number of lanes
        assert np.array_equal(svm.predict_values_gammas(Z, g[8:], A[8:], b[8:]), V[:, 8:])
        perm = np.random.default_rng(5).permutation(K)  # the lane's position
        assert np.array_equal(svm.predict_values_gammas(Z, g[perm], A[perm], b[perm]), V[:, perm])
        assert np.array_equal(svm.predict_values_gammas(Z[::-1], g, A, b), V[::-1])  # the points' order and number
        assert np.array_equal(svm.predict_values_gammas(Z[[137]], g, A, b), V[[137]])
        monkeypatch.setenv("PLSSVM_MI_PRED_CHUNK", "128")  # the chunking
        assert np.array_equal(svm.predict_values_gammas(Z, g, A, b), V)
        monkeypatch.delenv("PLSSVM_MI_PRED_CHUNK")
        # the leading dimensions: NaN past n in ALPHA is never read, sentinels past np in OUT are kept
        AL = np.full((K, n + 3), np.nan, dtype=dtype)
        AL[:, :n] = A
        out = np.full((K, npts + 2), -7.0, dtype=dtype)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        code = _abi.lib().plssvm_mi_predict_gammas_dense(svm._ctx, vp(g), vp(AL), K, n + 3, vp(b.astype(np.float64)), vp(Z),
                                                         npts, d, vp(out), npts + 2)
        assert code == 0 and np.array_equal(out[:, :npts].T, V) and (out[:, npts:] == -7.0).all()
        # the context is what it was
        assert np.array_equal(svm.predict_values(Z, A[0], b[0]), own) and svm.info()["kp_cache_tiles"] == tiles


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_after_learn_gammas(kernel, dtype):
    n, npts, d, K = SHAPES[2]
    X, Z, _, _, g, y = _inputs(n, npts, d, K, dtype)
    with _svm(kernel, X, 1.0 / d, dtype, labels=y) as svm:
        svm.learn_gammas(g, np.geomspace(0.5, 8.0, K))
        V = svm.predict_values_gammas(Z)
        assert svm.predict_stats() == [8, 1]
        assert np.array_equal(V, svm.predict_values_gammas(Z, svm.gammas, svm.alphas, svm.biases)) and np.isfinite(V).all()
        assert np.array_equal(svm.predict_gammas(Z), np.where(V > 0, 1, -1))


def test_refusals_and_argument_errors():
    n, npts, d, K = SHAPES[1]
    X, Z, A, b, g, _ = _inputs(n, npts, d, K, np.float64)
    for name, kw in dict(rbf_csr={}, linear={}, polynomial={}, rbf_sim=dict(sim_rank=(0, 2))).items():
        p = pm.Parameter(name.split("_")[0], gamma=0.1)
        if name == "rbf_csr":
            p.csr = (np.arange(n + 1, dtype=np.int64) * d, np.tile(np.arange(d, dtype=np.int32), n), X.ravel().copy(), n, d)
        else:
            p.data = X
        with pm.CSVM(p, **kw) as svm:
            with pytest.raises(_abi.BackendError, match=": gamma lanes run on") as e:
                svm.predict_values_gammas(Z, g, A, b)
            assert e.value.code == -5, name
            assert np.isfinite(svm.predict_values(Z, A[0], b[0])).all()  # the context stays usable
    with _svm("rbf", X, 0.1, np.float64) as svm:
        for bad in ([], [0.1, np.nan, 0.1], [np.inf] * 3, [0.0] * 3, [-1.0] * 3, g[:2]):
            with pytest.raises(ValueError):
                svm.predict_values_gammas(Z, bad, A, b)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        call = lambda gam=g, nl=K, lda=n, nz=npts, dz=d, ldo=npts, z=Z: _abi.lib().plssvm_mi_predict_gammas_dense(
            svm._ctx, vp(np.asarray(gam, dtype=np.float64)), vp(A), nl, lda, vp(b), None if z is None else vp(z), nz, dz,
            vp(out), ldo)
        out = np.full((K, npts), -7.0)
        assert [call(nl=0), call(gam=[0.1, -1.0, 0.1]), call(lda=n - 1), call(ldo=npts - 1), call(dz=d + 1), call(z=None)] == [-1] * 6
        assert call(nz=0) == 0 and (out == -7.0).all()  # no points: OK, out untouched
        assert call() == 0 and np.array_equal(out.T, svm.predict_values_gammas(Z, g, A, b))
