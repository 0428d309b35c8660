"""GPU tests of the gamma lanes (csrc/kp_gamma.hip): run_device_kernel_gammas / learn_gammas form a tile's distances
once and serve up to 8 (gamma, p) lanes from them.

Values: float64 numpy on the rounded data with direct ((x - z)**2).sum() / abs(x - z).sum() distances and the LS-SVM K.p
formula of tests/test_gpu_laplacian.py, the project's bars (1e-12 / 1e-4 of max|want| per lane). Everything else is
bitwise against a fresh context created with the lane's gamma. Shapes: m = 129 and 257 are a tile edge plus one row, 299
a tile triangle with an interior tile; d = 17 and 40 are no multiples of the chunk depth.
"""
import ctypes

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi
from test_gpu_laplacian import assert_close

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KERNELS = ["rbf", "laplacian"]
COST = 2.0


def gamma_grid(d, dtype, count=8):
    return np.geomspace(0.01 / d, 10.0 / d, count).astype(dtype).astype(np.float64)  # as the device holds them


def data(n, d, offset, dtype):
    rng = np.random.default_rng(n * 1000 + d)
    X = (rng.uniform(0.0, 1.0, size=(n, d)) + offset).astype(dtype)
    P = rng.uniform(-1.0, 2.0, size=(8, n - 1)).astype(dtype)  # signed
    return X, P, np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)


def make_svm(kernel, X, gamma, dtype, labels=None, **kw):
    p = pm.Parameter(kernel, gamma=float(gamma), cost=COST, epsilon=1e-6, real_type=dtype)
    p.data, p.labels = X, None if labels is None else labels.astype(dtype)
    return pm.CSVM(p, **kw)


def distances(kernel, X):
    X = X.astype(np.float64)
    diff = X[:, None, :] - X[None, :, :]
    return (diff ** 2).sum(-1) if kernel == "rbf" else np.abs(diff).sum(-1)


@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("n,d", [(n, d) for n in (130, 258, 300) for d in (17, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_values_against_numpy(kernel, dtype, n, d, offset):
    X, P, _ = data(n, d, offset, dtype)
    m, D, g8 = n - 1, distances(kernel, X), gamma_grid(d, dtype)
    with make_svm(kernel, X, 1.0 / d, dtype) as svm:
        svm.setup_data_on_device()
        for lanes in ([3], [0, 4, 7], list(range(8))):
            for add in (1.0, -1.0):
                RET = np.zeros((len(lanes), m), dtype=dtype)
                svm.run_device_kernel_gammas(g8[lanes], RET, P[lanes], add)
                for row, l in enumerate(lanes):
                    K, p = np.exp(-g8[l] * D), P[l].astype(np.float64)
                    q, qa = K[:m, m], K[m, m] + 1.0 / COST
                    want = add * (K[:m, :m] @ p + (qa - q) * p.sum() - q @ p + p / COST)
                    assert_close(RET[row], want, dtype, f"L={len(lanes)} lane {row} gamma {g8[l]:.3g} add {add:g}")


@pytest.mark.parametrize("kp_cache", [False, None], ids=["implicit", "cached"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_lane_is_bitwise_the_fresh_context(kernel, dtype, kp_cache):
    n, d = 300, 40
    X, P, _ = data(n, d, 0.0, dtype)
    m, g8 = n - 1, gamma_grid(d, dtype)
    with make_svm(kernel, X, 1.0 / d, dtype) as svm:
        svm.setup_data_on_device()
        R8 = svm.run_device_kernel_gammas(g8, np.zeros((8, m), dtype=dtype), P, 1.0)
        pick = [5, 0, 7]  # lane 5 moves to position 0
        R3 = svm.run_device_kernel_gammas(g8[pick], np.zeros((3, m), dtype=dtype), P[pick], 1.0)
        R1 = svm.run_device_kernel_gammas(g8[[5]], np.zeros((1, m), dtype=dtype), P[[5]], 1.0)
    assert np.array_equal(R3, R8[pick]) and np.array_equal(R1[0], R8[5])
    for l in pick:
        with make_svm(kernel, X, g8[l], dtype, kp_cache=kp_cache) as one:
            one.setup_data_on_device()
            one.generate_q()
            first = one.run_device_kernel(None, np.zeros(m, dtype=dtype), P[l], 1.0)   # forms (and stores) the tiles
            again = one.run_device_kernel(None, np.zeros(m, dtype=dtype), P[l], 1.0)   # streams stored ones
        assert np.isfinite(first).all() and np.abs(first).max() > 0
        assert np.array_equal(R8[l], first) and np.array_equal(R8[l], again), (kernel, dtype, l)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_learn_gammas_bitwise(kernel, dtype):
    n, d = 258, 40
    X, _, y = data(n, d, 0.0, dtype)
    g9 = gamma_grid(d, dtype, 9)  # two groups
    costs = np.array([0.5, 1.0, 2.0, 4.0, 8.0, 0.25, 3.0, 1.5, 16.0])
    with make_svm(kernel, X, 1.0 / d, dtype, labels=y) as svm:
        svm.learn()
        own, info0 = (svm.alpha.copy(), svm.bias, svm.iters, svm.trace.copy()), svm.info()
        svm.learn_gammas(g9, costs)
        got = (svm.alphas.copy(), svm.biases.copy(), svm.iters_multi.copy(), [t.copy() for t in svm.traces])
        assert np.array_equal(svm.gammas, g9)
        info1 = svm.info()
        svm.learn()
        assert np.array_equal(svm.alpha, own[0]) and svm.bias == own[1] and svm.iters == own[2] and np.array_equal(svm.trace, own[3])
        assert (info0["multi_width"], info0["kp_cache_tiles"]) == (info1["multi_width"], info1["kp_cache_tiles"])
        svm.learn_gammas(g9[:3])  # costs None: the context's cost on every lane
        at_own_cost = svm.alphas.copy()
    print("iterations per lane:", got[2])
    for k in range(9):
        for cost, alphas in ((costs[k], got[0]), (COST, at_own_cost if k < 3 else None)):
            if alphas is None:
                continue
            with make_svm(kernel, X, g9[k], dtype, labels=y) as one:
                one.setup_data_on_device()
                one.set_cost(cost)
                one.learn()
                assert np.array_equal(alphas[k], one.alpha), (k, cost)
                if alphas is got[0]:
                    assert got[1][k] == one.bias and got[2][k] == one.iters and np.array_equal(got[3][k], one.trace), k


def test_refusals():
    X, P, y = data(130, 17, 0.0, np.float64)
    m, g = 129, [0.01, 0.1]
    dense = dict(rbf_csr=None, linear=None, polynomial=None, rbf_sim=dict(sim_rank=(0, 2)))
    for name, kw in dense.items():
        kernel = name.split("_")[0]
        p = pm.Parameter(kernel, gamma=0.1, cost=COST)
        p.labels = y
        if name == "rbf_csr":
            p.csr = (np.arange(131, dtype=np.int64) * 17, np.tile(np.arange(17, dtype=np.int32), 130), X.ravel().copy(), 130, 17)
        else:
            p.data = X
        with pm.CSVM(p, **(kw or {})) as svm:
            for call in (lambda: svm.run_device_kernel_gammas(g, np.zeros((2, m)), P[:2], 1.0), lambda: svm.learn_gammas(g)):
                with pytest.raises(_abi.BackendError, match="gamma lanes run on") as e:
                    call()
                assert e.value.code == -5, name
    with make_svm("rbf", X, 0.1, np.float64, labels=y) as svm:
        svm.setup_data_on_device()
        for bad in ([], [0.1, np.nan], [np.inf], [0.0], [-1.0]):
            with pytest.raises(ValueError):
                svm.learn_gammas(bad)
            with pytest.raises(ValueError):
                svm.run_device_kernel_gammas(bad, np.zeros((max(len(bad), 1), m)), P[:max(len(bad), 1)], 1.0)
        with pytest.raises(ValueError):
            svm.learn_gammas(g, costs=[1.0])
        gam, out = (ctypes.c_double * 1)(-1.0), np.zeros(130)
        code = _abi.lib().plssvm_mi_learn_gammas(svm._ctx, y.ctypes.data_as(ctypes.c_void_p), gam, None, 1, 5, 1e-3,
                                                 out.ctypes.data_as(ctypes.c_void_p), None, None, None)
        assert code == -1  # ERR_ARG
        svm.learn_gammas(g)  # the context stays usable
        assert np.isfinite(svm.alphas).all()
