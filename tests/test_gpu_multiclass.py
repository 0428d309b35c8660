"""Multi-class one-vs-all training on a batched multi-vector K·P.

The K one-vs-all systems share Q~, so plssvm_mi_kp_multi / _solve_cg_multi / _learn_multi visit every kernel-matrix
tile once for all right-hand sides of a group and then run the single solve's own launches per lane. Every result must
therefore be BITWISE what the single-vector calls give for that vector alone: all comparisons here are np.array_equal
against run_device_kernel / learn / solver_CG on a second context of the same build (those are pinned against the
oracle by the rest of the suite).

Shapes as in test_gpu_kp_cache.py: m = 1300 (d = 20) is 66 tiles in three super-blocks (a full diagonal one, a ragged
off-diagonal one, a ragged diagonal one) with padded rows in the last tile row and d no multiple of the K-chunk depth;
m = 130 is the two-tile case.
"""
import ctypes
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

D = 20
TILE = 128
K = 5
IMAX = 200
DTYPES = {"f64": np.float64, "f32": np.float32}

# kernel, m, real, gamma, C, eps: the CPU oracle's iterations per class on this data are 90 / 82 / 89 / 80 / 80 (the
# first row: across the every-50th explicit residual, lanes stopping at different times), 33 / 32 / 33 / 33 / 31,
# 35 / 31 / 34 / 32 / 31, 19 / 20 / 20 / 19 / 20, 10 / 10 / 10 / 10 / 9 and 11 / 11 / 10 / 10 / 11
SETTINGS = [
    ("rbf", 1300, "f64", 1.0, 100.0, 1e-8),
    ("rbf", 1300, "f64", 1.0, 10.0, 1e-6),
    ("polynomial", 1300, "f64", 0.05, 10.0, 1e-6),
    ("linear", 1300, "f64", 0.05, 10.0, 1e-6),
    ("rbf", 1300, "f32", 1.0, 10.0, 1e-4),
    ("rbf", 130, "f64", 1.0, 10.0, 1e-6),
]


@functools.lru_cache(maxsize=None)
def _data(m, dtype):
    """5 unbalanced classes (class 0 takes a further quarter of the points) around 5 centres, features in [-1, 1]."""
    n = m + 1
    rng = np.random.default_rng(7)
    centers = rng.uniform(-10, 10, (K, D))
    lab = rng.integers(0, K, n)
    lab = np.where(rng.uniform(size=n) < 0.25, 0, lab)
    X = rng.normal(size=(n, D)) * 4 + centers[lab]
    lo, hi = X.min(axis=0), X.max(axis=0)
    X = np.ascontiguousarray(((X - lo) / (hi - lo) * 2 - 1).astype(DTYPES[dtype]))
    X.setflags(write=False)
    lab.setflags(write=False)
    return X, lab


def _svm(kernel, m, dtype, gamma=None, cost=1.0, eps=1e-3, **kw):
    X, _ = _data(m, dtype)
    p = pm.Parameter(kernel, gamma=1.0 / D if gamma is None else gamma, coef0=0.5, cost=cost, epsilon=eps,
                     real_type=DTYPES[dtype])
    p.data = X
    if kernel == "linear":
        kw.setdefault("kp_mode", "pairwise")
    return pm.CSVM(p, **kw)


def _ready(svm):
    svm.setup_data_on_device()
    svm.generate_q()
    return svm


# ---- 1. kp_multi columns equal kp columns --------------------------------------------------------------------------
PAD = 7
ADD = -0.5


def _kp_inputs(m, dtype):
    rng = np.random.default_rng(300 + m)
    P = np.full((K, m + PAD), np.nan, DTYPES[dtype])
    P[:, :m] = rng.uniform(-1, 2, (K, m))
    RET = rng.uniform(-1, 1, (K, m + PAD)).astype(DTYPES[dtype])
    return P, RET


@functools.lru_cache(maxsize=None)
def _reference_kp(kernel, dtype, m):
    """RET_c + ADD * Q~ P_c per vector through plssvm_mi_kp (cache off), computed once per case."""
    P, RET = _kp_inputs(m, dtype)
    with _svm(kernel, m, dtype, kp_cache=False) as svm:
        _ready(svm)
        out = np.stack([svm.run_device_kernel(None, RET[c, :m].copy(), P[c, :m], ADD) for c in range(K)])
    assert np.isfinite(out).all() and np.abs(out - RET[:, :m]).max() > 0
    out.setflags(write=False)
    return out


def _check_kp_multi(svm, kernel, dtype, m, R):
    P, RET = _kp_inputs(m, dtype)
    want = _reference_kp(kernel, dtype, m)
    got = svm.run_device_kernel_multi(None, RET[:R].copy(), P[:R], ADD)
    assert np.array_equal(got[:, m:], RET[:R, m:]), "the rows' tails were written"
    assert np.array_equal(got[:, :m], want[:R]), (kernel, dtype, m, R, np.abs(got[:, :m] - want[:R]).max())


@pytest.mark.parametrize("R", [1, 2, 3, 5])
@pytest.mark.parametrize("m", [1300, 130])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", ["rbf", "polynomial", "linear"])
def test_kp_multi_columns_are_bitwise_kp(kernel, dtype, m, R):
    nb = -(-m // TILE)
    with _svm(kernel, m, dtype, kp_cache=True) as svm:
        _ready(svm)
        assert svm.info()["multi_width"] >= 2
        _check_kp_multi(svm, kernel, dtype, m, R)  # fresh setup: the records are not filled yet
        _check_kp_multi(svm, kernel, dtype, m, R)  # streamed from the filled records
        assert svm.info()["kp_cache_tiles"] == nb * (nb + 1) // 2
    with _svm(kernel, m, dtype, kp_cache=False) as svm:
        _ready(svm)
        assert svm.info()["multi_width"] >= 2 and svm.info()["kp_cache_tiles"] == 0
        _check_kp_multi(svm, kernel, dtype, m, R)


@pytest.mark.parametrize("R", [2, 5])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kp_multi_with_a_partial_cache(dtype, R, monkeypatch):
    m = 1300
    rec = TILE * TILE * DTYPES[dtype]().itemsize
    monkeypatch.setenv("PLSSVM_MI_MEM_BUDGET", str(47 * rec + rec // 2))
    with _svm("rbf", m, dtype, kp_cache=True) as svm:
        _ready(svm)
        assert svm.info()["kp_cache_tiles"] == 47 and svm.info()["multi_width"] >= 2
        _check_kp_multi(svm, "rbf", dtype, m, R)
        _check_kp_multi(svm, "rbf", dtype, m, R)


# ---- 2. learn_multi equals K learn() calls ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_learn(setting, imax=IMAX, graph=None):
    """K single learn() calls with the one-vs-all labels on one context; graph: only part of the cache key (the
    caller has set PLSSVM_MI_GRAPH accordingly)."""
    kernel, m, dtype, gamma, cost, eps = SETTINGS[setting]
    _, lab = _data(m, dtype)
    with _svm(kernel, m, dtype, gamma, cost, eps) as svm:
        return _single_learns(svm, lab, imax)


def _single_learns(svm, lab, imax):
    """(classes, [(alpha, bias, iters, trace) per class]) of learn() on each one-vs-all label vector, on one context."""
    classes, Y = pm.one_vs_all(lab, svm.dtype)
    out = []
    svm.setup_data_on_device()
    for k in range(len(classes)):
        svm.params.labels = Y[k]
        svm.learn(imax)
        out.append((svm.alpha.copy(), svm.bias, svm.iters, svm.trace.copy()))
    assert all(np.isfinite(o[0]).all() for o in out)
    return classes, out


def _assert_learn_equal(svm, ref):
    classes, singles = ref
    assert np.array_equal(svm.classes, classes)
    for k, (alpha, bias, iters, trace) in enumerate(singles):
        assert svm.iters_multi[k] == iters, (k, svm.iters_multi, [s[2] for s in singles])
        assert np.array_equal(svm.traces[k], trace), (k, np.abs(svm.traces[k] - trace).max())
        assert np.array_equal(svm.alphas[k], alpha), (k, np.abs(svm.alphas[k] - alpha).max())
        assert svm.biases[k] == bias, (k, svm.biases[k], bias)


def _learn_multi(setting, imax=IMAX, **kw):
    kernel, m, dtype, gamma, cost, eps = SETTINGS[setting]
    svm = _svm(kernel, m, dtype, gamma, cost, eps, **kw)
    svm.learn_multi(_data(m, dtype)[1], imax)
    return svm


@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_learn_multi_is_bitwise_k_learns(setting):
    ref = _reference_learn(setting)
    iters = [s[2] for s in ref[1]]
    assert len(set(iters)) > 1 and max(iters) < IMAX, iters  # the lanes stop at different iterations
    if setting == 0:
        assert max(iters) > 50  # across the every-50th explicit residual
    with _learn_multi(setting) as svm:
        assert svm.info()["multi_width"] >= 2
        _assert_learn_equal(svm, ref)


@pytest.mark.parametrize("graph", ["0", None])
def test_learn_multi_with_graphs_off_and_on(graph, monkeypatch):
    if graph is None:
        monkeypatch.delenv("PLSSVM_MI_GRAPH", raising=False)
    else:
        monkeypatch.setenv("PLSSVM_MI_GRAPH", graph)
    ref = _reference_learn(0, IMAX, graph or "unset")
    with _learn_multi(0) as svm:
        _assert_learn_equal(svm, ref)


def test_abi_learn_multi_is_learn_lanes():
    """plssvm_mi_learn_multi stays in the ABI though CSVM.learn_multi goes through plssvm_mi_learn_lanes: called
    directly on the two-tile setting, its alphas, biases, traces and iteration counts are learn_multi()'s bits."""
    kernel, m, dtype, gamma, cost, eps = SETTINGS[5]
    lab = _data(m, dtype)[1]
    with _svm(kernel, m, dtype, gamma, cost, eps) as svm:
        svm.learn_multi(lab, IMAX)
        _, Y = pm.one_vs_all(lab, svm.dtype)
        nk, n = Y.shape
        alphas, biases = np.zeros((nk, n), dtype=svm.dtype), np.zeros(nk)
        trace, it = np.full((nk, IMAX + 1), np.nan), np.zeros(nk, dtype=np.int64)
        assert _abi.lib().plssvm_mi_learn_multi(svm._ctx, pm._ptr(Y), nk, n, IMAX, float(eps), pm._ptr(alphas), pm._ptr(biases),
                                                pm._ptr(trace), pm._ptr(it)) == _abi.OK
        assert nk == K and svm.iters_multi.min() > 0
        assert np.array_equal(it, svm.iters_multi) and np.array_equal(alphas, svm.alphas)
        assert np.array_equal(biases.astype(svm.dtype), svm.biases)
        for k in range(nk):
            assert np.array_equal(trace[k, : it[k] + 1], svm.traces[k])
            assert np.isnan(trace[k, it[k] + 1:]).all()  # a row is filled up to iters[k]


# ---- 3. chunking ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 1])
def test_groups_of_the_width(width):
    """multi_width = 2: 5 classes run as groups of 2, 2, 1; multi_width = 1: one at a time through the single solve."""
    ref = _reference_learn(1)
    with _learn_multi(1, multi_width=width) as svm:
        assert svm.info()["multi_width"] == width
        _assert_learn_equal(svm, ref)


# ---- 4. two multi solves on one context -------------------------------------------------------------------------------
def test_two_multi_solves_on_one_context():
    """The solves stop inside a polled batch (polls after 4, 12, 28, 40 iterations), then the same context solves
    again: only a product without a stop flag may fill the tile records, so both equal a fresh context's."""
    imax = 40
    ref = _reference_learn(1, imax)
    iters = [s[2] for s in ref[1]]
    assert all(28 < it < imax for it in iters), iters
    kernel, m, dtype, gamma, cost, eps = SETTINGS[1]
    lab = _data(m, dtype)[1]
    with _svm(kernel, m, dtype, gamma, cost, eps) as svm:
        svm.learn_multi(lab, imax)
        _assert_learn_equal(svm, ref)
        svm.learn_multi(lab, imax)
        _assert_learn_equal(svm, ref)
        assert svm.info()["kp_cache_tiles"] == 66


# ---- 5. fallback paths --------------------------------------------------------------------------------------------------
def _three_rhs(m, dtype):
    rng = np.random.default_rng(55)
    return rng.uniform(-1, 1, (3, m)).astype(dtype)


def test_fallback_on_stored_sparse_data():
    n, d = 301, 64
    csr, _ = datagen.sparse_csr(n, d, 8, seed=5, dtype=np.float64)
    lab = np.random.default_rng(9).integers(0, 3, n) * 2.5  # float class labels
    classes, Y = pm.one_vs_all(lab)

    def ctx():
        p = pm.Parameter("rbf", gamma=0.1, cost=10.0, epsilon=1e-6)
        p.csr = csr
        return pm.CSVM(p)

    singles = []
    with ctx() as svm:
        svm.setup_data_on_device()
        for k in range(3):
            svm.params.labels = Y[k]
            svm.learn(30)
            singles.append((svm.alpha.copy(), svm.bias, svm.iters, svm.trace.copy()))
    with ctx() as svm:
        svm.learn_multi(lab, 30)
        info = svm.info()
        assert info["is_sparse"] == 1 and info["sparse_algo"] != _abi.SPARSE_DENSE
        assert info["multi_width"] == 1
        _assert_learn_equal(svm, (classes, singles))


def test_lanes_on_densified_sparse_data():
    """CSR data densified on the device runs the tile path, so its one-vs-all solves are lanes: m = 300 is three tile
    rows, six tiles. gamma = 0.1, C = 100, eps = 1e-6: the CPU oracle's iterations per class are 60 / 59 / 59, past the
    explicit residual of iteration 50."""
    n, d, imax = 301, 64, 120
    csr, _ = datagen.sparse_csr(n, d, 8, seed=5, dtype=np.float64)
    lab = np.random.default_rng(9).integers(0, 3, n) * 2.5

    def ctx():
        p = pm.Parameter("rbf", gamma=0.1, cost=100.0, epsilon=1e-6)
        p.csr = csr
        return pm.CSVM(p, sparse_algo="dense")

    with ctx() as svm:
        ref = _single_learns(svm, lab, imax)
    iters = [s[2] for s in ref[1]]
    assert len(ref[0]) == 3 and 50 < max(iters) < imax, iters
    with ctx() as svm:
        svm.learn_multi(lab, imax)
        info = svm.info()
        assert info["is_sparse"] == 1 and info["sparse_algo"] == _abi.SPARSE_DENSE
        assert info["multi_width"] >= 2
        _assert_learn_equal(svm, ref)


def test_time_kp_multi_leaves_the_context_intact():
    m, dtype = 130, "f64"
    lab = _data(m, dtype)[1]
    with _svm("rbf", m, dtype, eps=1e-6) as svm:
        ref = _single_learns(svm, lab, IMAX)
    with _svm("rbf", m, dtype, eps=1e-6) as svm:
        _ready(svm)
        assert svm.info()["multi_width"] >= 2
        ms = svm.time_kp_multi(3, reps=2)
        assert np.isfinite(ms) and ms > 0
        _check_kp_multi(svm, "rbf", dtype, m, 3)
        svm.learn_multi(lab, IMAX)
        _assert_learn_equal(svm, ref)


def test_fallback_on_a_simulated_rank():
    m, dtype = 1300, "f64"
    B = _three_rhs(m, DTYPES[dtype])
    with _svm("rbf", m, dtype, sim_rank=(1, 3)) as svm:
        _ready(svm)
        kp = [svm.run_device_kernel(None, np.zeros(m), B[c], 1.0).copy() for c in range(3)]
        cg = []
        for c in range(3):
            x = svm.solver_CG(B[c], 6, 1e-3).copy()
            cg.append((x, svm.iters, svm.trace.copy()))
    assert all(np.isfinite(v).all() for v in kp) and all(np.isfinite(x).all() for x, _, _ in cg)
    with _svm("rbf", m, dtype, sim_rank=(1, 3)) as svm:
        _ready(svm)
        assert svm.info()["multi_width"] == 1
        got = svm.run_device_kernel_multi(None, np.zeros((3, m)), B, 1.0)
        X = svm.solver_CG_multi(B, 6, 1e-3)
        for c in range(3):
            assert np.array_equal(got[c], kp[c])
            assert np.array_equal(X[c], cg[c][0]) and svm.iters_multi[c] == cg[c][1]
            assert np.array_equal(svm.traces[c], cg[c][2])


# ---- 6. prediction --------------------------------------------------------------------------------------------------------
def test_predict_multi():
    kernel, m, dtype, gamma, cost, eps = SETTINGS[1]
    X, lab = _data(m, dtype)
    with _learn_multi(1) as svm:
        V = svm.predict_values_multi(X)
        assert V.shape == (m + 1, K)
        for k in range(K):
            assert np.array_equal(V[:, k], svm.predict_values(X, svm.alphas[k], svm.biases[k]))
        pred = svm.predict_multi(X)
        assert np.array_equal(pred, svm.classes[np.argmax(V, axis=1)])
    majority = np.bincount(lab).max() / lab.size
    assert np.mean(pred == lab) >= majority  # a sanity bound, not a tuned number


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable():
    m, dtype = 130, "f64"
    P, RET = _kp_inputs(m, dtype)
    L = _abi.lib()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    with _svm("rbf", m, dtype) as svm:
        _ready(svm)
        out = RET[:2].copy()
        it = np.zeros(2, np.int64)
        X = np.zeros((2, m + PAD))
        assert L.plssvm_mi_kp_multi(svm._ctx, None, ptr(P), ptr(out), 0, m + PAD, 1.0) == -1
        assert L.plssvm_mi_kp_multi(svm._ctx, None, ptr(P), ptr(out), 2, m - 1, 1.0) == -1
        assert L.plssvm_mi_kp_multi(svm._ctx, None, None, ptr(out), 2, m + PAD, 1.0) == -1
        assert L.plssvm_mi_solve_cg_multi(svm._ctx, ptr(out), 0, m + PAD, None, 10, 1e-3, ptr(X), None, ptr(it)) == -1
        assert L.plssvm_mi_solve_cg_multi(svm._ctx, ptr(out), 2, m - 1, None, 10, 1e-3, ptr(X), None, ptr(it)) == -1
        assert L.plssvm_mi_learn_multi(svm._ctx, ptr(out), 0, m + PAD, 10, 1e-3, ptr(X), None, None, ptr(it)) == -1
        assert L.plssvm_mi_learn_multi(svm._ctx, ptr(out), 2, m, 10, 1e-3, ptr(X), None, None, ptr(it)) == -1  # ldy < n
        assert L.plssvm_mi_time_kp_multi(svm._ctx, 0, 1, None) == -1
        assert np.array_equal(out, RET[:2])
        with pytest.raises(pm.BackendError) as e:
            svm._check(L.plssvm_mi_kp_multi(svm._ctx, None, ptr(P), ptr(out), 2, m - 1, 1.0))
        assert e.value.code == -1 and "leading dimension" in str(e.value)
        with pytest.raises(ValueError, match="at least 2 classes"):
            svm.learn_multi(np.ones(m + 1, np.int64))
        with pytest.raises(ValueError, match="at least"):
            svm.run_device_kernel_multi(None, np.zeros((2, m - 1)), np.zeros((2, m - 1)), 1.0)
        _check_kp_multi(svm, "rbf", dtype, m, 3)  # still usable
