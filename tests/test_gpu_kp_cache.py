"""Stored kernel-matrix tiles of the dense pairwise path (PLSSVM_MI_OPT_KP_CACHE).

The first K·p of a setup stores the 128 x 128 tiles of k(x_i, x_j) it forms (KP_COMPUTE_STORE), later ones stream them
(KP_LOAD) through the same epilogue, so every result must be BITWISE the implicit product's: all comparisons here are
np.array_equal against a context with the cache off.

Shapes: m = 1300 (d = 20) gives nb = 11 tile rows, i.e. 66 tiles in three super-blocks — a full diagonal one (tiles
[0, 36)), an off-diagonal one with a ragged row count (3 x 8 tiles, [36, 60)) and a ragged diagonal one ([60, 66)) —
with padded rows in the last tile row and d no multiple of the K-chunk depth; m = 130 (nb = 2) is the tiny case.
"""
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import datagen

pytestmark = pytest.mark.gpu

D = 20
TILE = 128
DTYPES = {"f64": np.float64, "f32": np.float32}


@functools.lru_cache(maxsize=None)
def _data(m, dtype, seed=11):
    X, y = datagen.blobs(m + 1, D, seed=seed, dtype=DTYPES[dtype])
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _vectors(m, dtype, count=3):
    rng = np.random.default_rng(100 + m)
    return [rng.uniform(-1, 2, m).astype(DTYPES[dtype]) for _ in range(count)]


def _svm(kernel, dtype, m, cache, seed=11, **kw):
    X, y = _data(m, dtype, seed)
    p = pm.Parameter(kernel, gamma=1.0 / D, coef0=0.5, real_type=DTYPES[dtype])
    p.data, p.labels = X, y
    if kernel == "linear":
        kw.setdefault("kp_mode", "pairwise")
    return pm.CSVM(p, kp_cache=cache, **kw)


def _kps(svm, m, dtype):
    """Three K·p with different p on a fresh setup: with the cache on, the first fills and the others load."""
    svm.setup_data_on_device()
    svm.generate_q()
    return [svm.run_device_kernel(None, np.zeros(m, DTYPES[dtype]), v, 1.0).copy() for v in _vectors(m, dtype)]


@functools.lru_cache(maxsize=None)
def _reference_kps(kernel, dtype, m, sim=None):
    """The implicit product (cache off), computed once per case and shared."""
    with _svm(kernel, dtype, m, False, sim_rank=sim) as svm:
        out = _kps(svm, m, dtype)
        assert svm.info()["kp_cache_tiles"] == 0 and svm.info()["kp_cache_bytes"] == 0
    for o in out:
        o.setflags(write=False)
    return tuple(out)


def _tiles(m):
    nb = -(-m // TILE)
    return nb * (nb + 1) // 2


@pytest.mark.parametrize("m", [1300, 130])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", ["rbf", "polynomial", "linear"])
def test_kp_from_cache_is_bitwise_the_computed_one(kernel, dtype, m):
    want = _reference_kps(kernel, dtype, m)
    with _svm(kernel, dtype, m, True) as svm:
        got = _kps(svm, m, dtype)
        info = svm.info()
    assert info["kp_cache_tiles"] == _tiles(m) == info["tiles_local"]
    assert info["kp_cache_bytes"] == _tiles(m) * TILE * TILE * DTYPES[dtype]().itemsize
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(w).all() and np.abs(w).max() > 0
        assert np.array_equal(g, w), (kernel, dtype, m, k, np.abs(g - w).max())


# T tiles cached of m = 1300's 66: inside the diagonal super-block, inside the off-diagonal one, none
@pytest.mark.parametrize("want_tiles", [20, 47, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_partial_cache(dtype, want_tiles, monkeypatch):
    m = 1300
    rec = TILE * TILE * DTYPES[dtype]().itemsize
    budget = want_tiles * rec + rec // 2 if want_tiles else rec - 1
    want = _reference_kps("rbf", dtype, m)
    monkeypatch.setenv("PLSSVM_MI_MEM_BUDGET", str(budget))
    with _svm("rbf", dtype, m, True) as svm:
        got = _kps(svm, m, dtype)
        info = svm.info()
    assert info["kp_cache_tiles"] == min(_tiles(m), budget // rec) == want_tiles
    assert info["kp_cache_bytes"] == want_tiles * rec
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (dtype, want_tiles, k, np.abs(g - w).max())


def test_env_switch_turns_the_cache_off(monkeypatch):
    m = 130
    monkeypatch.setenv("PLSSVM_MI_KP_CACHE", "0")
    with _svm("rbf", "f64", m, None) as svm:
        got = _kps(svm, m, "f64")
        assert svm.info()["kp_cache_tiles"] == 0
    for g, w in zip(got, _reference_kps("rbf", "f64", m)):
        assert np.array_equal(g, w)


def _cg61(cache, dtype, m=1300):
    _, y = _data(m, dtype)
    with _svm("rbf", dtype, m, cache) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        svm.cg_begin((y[:-1] - y[-1]).astype(DTYPES[dtype]), None, eps=1e-3)
        it, _ = svm.cg_step(61, force=True)
        assert it == 61
        x, trace, _ = svm.cg_result(62)
        return x.copy(), trace.copy(), svm.info()["kp_cache_tiles"]


@pytest.mark.parametrize("graph", ["0", None])
def test_cg_across_a_graph_block(graph, monkeypatch):
    """61 forced iterations: the every-50th explicit residual (run 49) and, with graphs on, one captured block."""
    if graph is None:
        monkeypatch.delenv("PLSSVM_MI_GRAPH", raising=False)
    else:
        monkeypatch.setenv("PLSSVM_MI_GRAPH", graph)
    x1, t1, tiles1 = _cg61(True, "f64")
    x0, t0, tiles0 = _cg61(False, "f64")
    assert tiles1 == _tiles(1300) and tiles0 == 0
    assert len(t1) == 62 and np.isfinite(t1).all()
    assert np.array_equal(t1, t0), np.abs(t1 - t0).max()
    assert np.array_equal(x1, x0), np.abs(x1 - x0).max()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_share_of_a_simulated_rank(dtype):
    m = 1300
    want = _reference_kps("rbf", dtype, m, sim=(1, 3))
    with _svm("rbf", dtype, m, True, sim_rank=(1, 3)) as svm:
        got = _kps(svm, m, dtype)
        info = svm.info()
    assert 0 < info["tiles_local"] < _tiles(m)
    assert info["kp_cache_tiles"] == info["tiles_local"]
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (dtype, k)


def test_a_second_setup_drops_the_records():
    m, dtype = 1300, "f64"
    X2, _ = _data(m, dtype, seed=29)
    v = _vectors(m, dtype, 1)[0]
    with _svm("rbf", dtype, m, True) as svm:
        first = _kps(svm, m, dtype)  # fills and loads the first data's tiles
        svm.params.data = X2
        svm.setup_data_on_device()
        svm.generate_q()
        a = svm.run_device_kernel(None, np.zeros(m), v, 1.0).copy()  # fills again
        b = svm.run_device_kernel(None, np.zeros(m), v, 1.0).copy()  # loads
        assert svm.info()["kp_cache_tiles"] == _tiles(m)
    with _svm("rbf", dtype, m, False, seed=29) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        want = svm.run_device_kernel(None, np.zeros(m), v, 1.0).copy()
    assert not np.array_equal(first[0], want)
    assert np.array_equal(a, want) and np.array_equal(b, want)


def test_solves_after_an_early_exit():
    """A solve whose kernels leave at `converged` inside a polled batch, then a second solve on the same context: only
    a K·p without a stop flag may fill the records, so both solves equal a fresh context's (cache on and off)."""
    m, dtype = 1300, "f64"
    _, y = _data(m, dtype)
    b = y[:-1] - y[-1]

    def solve(svm):
        x = svm.solver_CG(b, 40, 1e-3).copy()
        return x, svm.trace.copy(), svm.iters

    with _svm("rbf", dtype, m, True) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        first, second = solve(svm), solve(svm)
    fresh = {}
    for cache in (True, False):
        with _svm("rbf", dtype, m, cache) as svm:
            svm.setup_data_on_device()
            svm.generate_q()
            fresh[cache] = solve(svm)
    it = fresh[False][2]
    assert 0 < it < 40 and it not in (4, 12, 28), it  # converged, and inside a batch (polls after 4, 12, 28)
    for got in (first, second, fresh[True]):
        assert got[2] == it
        assert np.array_equal(got[1], fresh[False][1])
        assert np.array_equal(got[0], fresh[False][0])
