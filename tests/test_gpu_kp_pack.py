"""Stored fp64 tiles at 7 bytes per value (csrc/kp_pack.hpp, DESIGN.md §3.1.2, PLSSVM_MI_OPT_KP_PACK).

A cached tile whose values are all positive normal numbers within 16 binades is stored as 52 mantissa bits + a 4-bit
exponent offset per value and decoded while it is streamed; every other tile keeps its raw record. The decode is
exact, so every result must be BITWISE what raw records and the implicit product give: all comparisons here are
np.array_equal.

Shapes: d = 20; m = 130 is 3 tiles (nb = 2), m = 300 is 6 tiles (nb = 3) with padded rows in the last tile row.
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
GAMMA_WIDE = 40.0  # tiles of spread points span far more than 15 binades (15 ln 2 / 40 = 0.26 in squared distance)


def _tiles(m):
    nb = -(-m // TILE)
    return nb * (nb + 1) // 2


@functools.lru_cache(maxsize=None)
def _blobs(m, dtype, seed=11):
    X, y = datagen.blobs(m + 1, D, seed=seed, dtype=DTYPES[dtype])
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def _mixed(m=300):
    """Rows 0..255 (tile rows 0 and 1) are a tight cluster, the rest is spread over [-1, 1]: with GAMMA_WIDE the three
    tiles among the cluster hold values next to 1, the three tiles of the last tile row hold exp(-40 |x_i - x_j|^2)
    over many binades (and the padded rows' and the diagonal's values beside them)."""
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (m + 1, D))
    X[:256] = rng.uniform(-0.5, 0.5, D) + 1e-3 * rng.standard_normal((256, D))
    y = np.where(rng.uniform(size=m + 1) < 0.5, -1.0, 1.0)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _vectors(m, dtype, count=3):
    rng = np.random.default_rng(100 + m)
    return [rng.uniform(-1, 2, m).astype(DTYPES[dtype]) for _ in range(count)]


def _svm(kernel, dtype, data, gamma=1.0 / D, **kw):
    X, y = data
    p = pm.Parameter(kernel, gamma=gamma, coef0=0.5, real_type=DTYPES[dtype])
    p.data, p.labels = X.astype(DTYPES[dtype], copy=False), y.astype(DTYPES[dtype], copy=False)
    if kernel == "linear":
        kw.setdefault("kp_mode", "pairwise")
    return pm.CSVM(p, **kw)


def _kps(svm, m, dtype):
    """Three K·p with different p on a fresh setup: with the cache on, the first fills and the others stream."""
    svm.setup_data_on_device()
    svm.generate_q()
    return [svm.run_device_kernel(None, np.zeros(m, DTYPES[dtype]), v, 1.0).copy() for v in _vectors(m, dtype)]


@functools.lru_cache(maxsize=None)
def _implicit(kernel, dtype, m, which="blobs", gamma=1.0 / D):
    """The implicit product (cache off), computed once per case and shared."""
    data = _blobs(m, dtype) if which == "blobs" else _mixed(m)
    with _svm(kernel, dtype, data, gamma, kp_cache=False) as svm:
        out = _kps(svm, m, dtype)
        info = svm.info()
    assert info["kp_cache_tiles"] == 0 and info["kp_cache_packed_tiles"] == 0
    for o in out:
        assert np.isfinite(o).all() and np.abs(o).max() > 0
        o.setflags(write=False)
    return tuple(out)


def _assert_all_equal(got, want, tag):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (tag, k, np.abs(g - w).max())


@pytest.mark.parametrize("m", [130, 300])
def test_rbf_packed_equals_raw_equals_implicit(m):
    want = _implicit("rbf", "f64", m)
    with _svm("rbf", "f64", _blobs(m, "f64"), kp_pack=True) as svm:
        on = _kps(svm, m, "f64")
        info = svm.info()
    assert info["kp_cache_packed_tiles"] == info["kp_cache_tiles"] == _tiles(m) > 0
    assert info["kp_cache_bytes"] == _tiles(m) * TILE * TILE * 8  # the record stride does not change
    with _svm("rbf", "f64", _blobs(m, "f64"), kp_pack=False) as svm:
        off = _kps(svm, m, "f64")
        info = svm.info()
    assert info["kp_cache_tiles"] == _tiles(m) and info["kp_cache_packed_tiles"] == 0
    _assert_all_equal(on, off, ("on/off", m))
    _assert_all_equal(on, want, ("on/implicit", m))
    _assert_all_equal(off, want, ("off/implicit", m))


def test_default_is_on_and_the_environment_switch_turns_it_off(monkeypatch):
    m = 130
    want = _implicit("rbf", "f64", m)
    with _svm("rbf", "f64", _blobs(m, "f64")) as svm:
        got = _kps(svm, m, "f64")
        assert svm.info()["kp_cache_packed_tiles"] == _tiles(m)
    _assert_all_equal(got, want, "default")
    monkeypatch.setenv("PLSSVM_MI_KP_PACK", "0")
    with _svm("rbf", "f64", _blobs(m, "f64")) as svm:
        got = _kps(svm, m, "f64")
        info = svm.info()
    assert info["kp_cache_tiles"] == _tiles(m) and info["kp_cache_packed_tiles"] == 0
    _assert_all_equal(got, want, "env")


def test_no_tile_is_counted_before_the_fill():
    m = 130
    with _svm("rbf", "f64", _blobs(m, "f64")) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        info = svm.info()
        assert info["kp_cache_tiles"] == _tiles(m) and info["kp_cache_packed_tiles"] == 0
        svm.run_device_kernel(None, np.zeros(m), _vectors(m, "f64", 1)[0], 1.0)
        assert svm.info()["kp_cache_packed_tiles"] == _tiles(m)


def test_mixed_cache():
    """Packed and raw tiles in one cache: also on the host, the spread rows' tiles are not packable."""
    m = 300
    X, _ = _mixed(m)
    rows = X[256:m]
    d2 = ((rows[:, None, :] - X[None, :128, :]) ** 2).sum(-1)
    k = np.exp(-GAMMA_WIDE * d2)
    assert (k == 0).any() or np.log2(k.max() / k[k > 0].min()) > 16  # tile (2, 0) cannot pack
    assert np.exp(-GAMMA_WIDE * ((X[:256, None, :] - X[None, :256, :]) ** 2).sum(-1)).min() > 0.5  # the cluster can
    want = _implicit("rbf", "f64", m, "mixed", GAMMA_WIDE)
    with _svm("rbf", "f64", _mixed(m), GAMMA_WIDE) as svm:
        got = _kps(svm, m, "f64")
        info = svm.info()
    assert info["kp_cache_tiles"] == _tiles(m) == 6
    assert 0 < info["kp_cache_packed_tiles"] < info["kp_cache_tiles"], info["kp_cache_packed_tiles"]
    assert info["kp_cache_packed_tiles"] == 3  # tiles (0, 0), (1, 0), (1, 1)
    _assert_all_equal(got, want, "mixed")


@pytest.mark.parametrize("kernel,dtype", [("linear", "f64"), ("polynomial", "f64"), ("rbf", "f32")])
@pytest.mark.parametrize("m", [130, 300])
def test_other_kernels_and_real_types(kernel, dtype, m):
    want = _implicit(kernel, dtype, m)
    with _svm(kernel, dtype, _blobs(m, dtype)) as svm:
        got = _kps(svm, m, dtype)
        info = svm.info()
    assert info["kp_cache_tiles"] == _tiles(m)
    if dtype == "f32":
        assert info["kp_cache_packed_tiles"] == 0
    _assert_all_equal(got, want, (kernel, dtype, m))


def test_partial_cache(monkeypatch):
    m = 300
    rec = TILE * TILE * 8
    budget = 4 * rec + rec // 2
    want = _implicit("rbf", "f64", m)
    monkeypatch.setenv("PLSSVM_MI_MEM_BUDGET", str(budget))
    with _svm("rbf", "f64", _blobs(m, "f64")) as svm:
        got = _kps(svm, m, "f64")
        info = svm.info()
    assert info["kp_cache_tiles"] == budget // rec == 4  # the descriptors take nothing from the budget
    assert info["kp_cache_bytes"] == 4 * rec
    assert info["kp_cache_packed_tiles"] == 4
    _assert_all_equal(got, want, "partial")


@pytest.mark.parametrize("which,gamma", [("blobs", 1.0 / D), ("mixed", GAMMA_WIDE)])
def test_kp_multi_on_a_packed_cache(which, gamma):
    m, R = 300, 3
    data = _blobs(m, "f64") if which == "blobs" else _mixed(m)
    P = np.stack(_vectors(m, "f64", R))
    with _svm("rbf", "f64", data, gamma) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        single = [svm.run_device_kernel(None, np.zeros(m), P[c], 1.0).copy() for c in range(R)]  # fills, then streams
        assert svm.info()["kp_cache_packed_tiles"] == (6 if which == "blobs" else 3)
        assert svm.info()["multi_width"] >= R
        multi = svm.run_device_kernel_multi(None, np.zeros((R, m)), P, 1.0)
    _assert_all_equal(single, _implicit("rbf", "f64", m, which, gamma), "single")
    _assert_all_equal(list(multi), single, "multi")


def test_learn_multi_on_a_packed_cache():
    m = 300
    X, _ = _blobs(m, "f64")
    lab = np.arange(m + 1) % 3
    out = {}
    for pack in (True, False):
        p = pm.Parameter("rbf", gamma=1.0 / D, cost=10.0, epsilon=1e-6, real_type=np.float64)
        p.data = X
        with pm.CSVM(p, kp_pack=pack) as svm:
            svm.learn_multi(lab, 200)
            info = svm.info()
            assert info["kp_cache_packed_tiles"] == (_tiles(m) if pack else 0)
            assert info["multi_width"] >= 3
            out[pack] = (svm.alphas.copy(), np.array(svm.biases), list(svm.iters_multi), [t.copy() for t in svm.traces])
    # the single-vector solves, one class at a time, on packed records
    classes, Y = pm.one_vs_all(lab, np.float64)
    p = pm.Parameter("rbf", gamma=1.0 / D, cost=10.0, epsilon=1e-6, real_type=np.float64)
    p.data = X
    with pm.CSVM(p, kp_pack=True) as svm:
        svm.setup_data_on_device()
        for k in range(len(classes)):
            svm.params.labels = Y[k]
            svm.learn(200)
            for pack in (True, False):
                assert out[pack][2][k] == svm.iters and 0 < svm.iters < 200
                assert np.array_equal(out[pack][3][k], svm.trace)
                assert np.array_equal(out[pack][0][k], svm.alpha)
                assert out[pack][1][k] == svm.bias
        assert svm.info()["kp_cache_packed_tiles"] == _tiles(m)


def _cg61(pack, m=300):
    _, y = _blobs(m, "f64")
    with _svm("rbf", "f64", _blobs(m, "f64"), kp_pack=pack) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        svm.cg_begin(y[:-1] - y[-1], None, eps=1e-3)
        it, _ = svm.cg_step(61, force=True)
        assert it == 61
        x, trace, _ = svm.cg_result(62)
        return x.copy(), trace.copy(), svm.info()["kp_cache_packed_tiles"]


def test_cg_across_a_graph_block(monkeypatch):
    """61 forced iterations: the every-50th explicit residual and one captured block of iterations."""
    monkeypatch.delenv("PLSSVM_MI_GRAPH", raising=False)
    x1, t1, packed1 = _cg61(True)
    x0, t0, packed0 = _cg61(False)
    assert packed1 == _tiles(300) and packed0 == 0
    assert len(t1) == 62 and np.isfinite(t1).all()
    assert np.array_equal(t1, t0), np.abs(t1 - t0).max()
    assert np.array_equal(x1, x0), np.abs(x1 - x0).max()


def test_a_second_setup_rebuilds_descriptors_and_counter():
    """gamma = 40 on both data sets: the blobs' tiles are all raw there, three of the mixed data's are packed."""
    m = 300
    v = _vectors(m, "f64", 1)[0]

    def two_products(svm):
        svm.setup_data_on_device()
        svm.generate_q()
        a = svm.run_device_kernel(None, np.zeros(m), v, 1.0).copy()  # fills
        b = svm.run_device_kernel(None, np.zeros(m), v, 1.0).copy()  # streams
        return a, b, svm.info()["kp_cache_packed_tiles"]

    fresh = {}
    for which, data in (("blobs", _blobs(m, "f64")), ("mixed", _mixed(m))):
        with _svm("rbf", "f64", data, GAMMA_WIDE) as svm:
            fresh[which] = two_products(svm)
        assert np.array_equal(fresh[which][0], fresh[which][1])
    assert fresh["blobs"][2] != fresh["mixed"][2] == 3
    for first, second in (("blobs", "mixed"), ("mixed", "blobs")):
        data = {"blobs": _blobs(m, "f64"), "mixed": _mixed(m)}
        with _svm("rbf", "f64", data[first], GAMMA_WIDE) as svm:
            got1 = two_products(svm)
            svm.params.data = data[second][0]
            got2 = two_products(svm)
        for got, want in ((got1, fresh[first]), (got2, fresh[second])):
            assert got[2] == want[2]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    want = _implicit("rbf", "f64", m, "mixed", GAMMA_WIDE)
    assert np.array_equal(fresh["mixed"][0], want[0])
