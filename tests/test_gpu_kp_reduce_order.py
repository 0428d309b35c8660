"""The summation order of the dense K·p slab pass, pinned against recorded results.

kp_reduce_share_kernel adds a row's slab values in sixteen chains (chain g: the column super-blocks g, g + 16, ... in
ascending order, one value at a time) and then the chains in g order. Its block shape, loads and prefetch are free to
change; the order is not. So nothing here compares the build with itself: every K·p vector, the CG solution and its
residual trace are compared with np.array_equal against tests/golden/kp_reduce_order/*.npz, which
tests/golden/make_kp_reduce_order.py recorded from the build before the slab pass was reshaped.

Shapes (d = 8): m = 100 is one diagonal tile; m = 1100 is nine tile rows — two rows of super-blocks, a ragged last
tile, diagonal and off-diagonal super-blocks; m = 16517 = 129 * 128 + 5 has nb = 130 tile rows, i.e. 17 column
super-blocks, so chain 0 wraps (CS = 0 and 16), the last super-block has 2 tiles and the last tile 5 rows: the
smallest shape at which a chain has more than one super-block.
"""
import functools
import os

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import datagen

pytestmark = pytest.mark.gpu

D = 8
TILE = 128
SHAPES = [100, 1100, 16517]
DTYPES = {"f64": np.float64, "f32": np.float32}
KERNELS = ["rbf", "linear"]
SIMS = [(1, 3), (0, 3)]
M_SIM = 16517
M_CG = 1100
CG_ITERS = 60
CLASSES = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kp_reduce_order")


@functools.lru_cache(maxsize=None)
def _data(m, dtype):
    X, y = datagen.blobs(m + 1, D, seed=23, dtype=DTYPES[dtype])
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _vector(m, dtype):
    return np.random.default_rng(500 + m).uniform(-1, 2, m).astype(DTYPES[dtype])


def _svm(kernel, dtype, m, cache, **kw):
    X, y = _data(m, dtype)
    p = pm.Parameter(kernel, gamma=1.0 / D, real_type=DTYPES[dtype])
    p.data, p.labels = X, y
    if kernel == "linear":
        kw.setdefault("kp_mode", "pairwise")
    return pm.CSVM(p, kp_cache=cache, **kw)


def kp_twice(kernel, dtype, m, cache, sim=None):
    """The same K·p twice on a fresh setup, through kp_host: with the cache on the first fills the records and the
    second streams them."""
    v = _vector(m, dtype)
    with _svm(kernel, dtype, m, cache, sim_rank=sim) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        out = [svm.run_device_kernel(None, np.zeros(m, DTYPES[dtype]), v, 1.0).copy() for _ in range(2)]
        return out, svm.info()


def cg60(single_steps):
    """60 forced CG iterations at m = 1100, fp64 RBF: as one cg_step(60) (a captured 50-iteration block and the
    every-50th reset product), or as 60 calls of cg_step(1)."""
    _, y = _data(M_CG, "f64")
    with _svm("rbf", "f64", M_CG, True) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        svm.cg_begin((y[:-1] - y[-1]).astype(np.float64), None, eps=1e-3)
        if single_steps:
            for k in range(CG_ITERS):
                it, _ = svm.cg_step(1, force=True)
                assert it == k + 1
        else:
            it, _ = svm.cg_step(CG_ITERS, force=True)
            assert it == CG_ITERS
        x, trace, _ = svm.cg_result(CG_ITERS + 1)
        return x.copy(), trace.copy()


def kp_name(kernel, dtype, m, sim=None):
    return f"kp_{kernel}_{dtype}_{m}" + (f"_rank{sim[0]}of{sim[1]}" if sim else "")


@functools.lru_cache(maxsize=None)
def _golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


def _tiles(m):
    nb = -(-m // TILE)
    return nb * (nb + 1) // 2


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("m", SHAPES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_kp_is_bitwise_the_recorded_one(kernel, dtype, m, cache):
    want = _golden(kp_name(kernel, dtype, m))["kp"]
    assert want.dtype == DTYPES[dtype] and want.shape == (m,) and np.isfinite(want).all() and np.abs(want).max() > 0
    got, info = kp_twice(kernel, dtype, m, cache)
    assert info["kp_cache_tiles"] == (_tiles(m) if cache else 0)
    for k, g in enumerate(got):
        assert np.array_equal(g, want), (kernel, dtype, m, cache, k, np.abs(g - want).max())


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("sim", SIMS)
def test_share_of_a_simulated_rank(sim, cache):
    """Rank 1 of 3's share begins and ends inside a row of super-blocks; rank 0's begins at the first."""
    want = _golden(kp_name("rbf", "f64", M_SIM, sim))["kp"]
    got, info = kp_twice("rbf", "f64", M_SIM, cache, sim)
    assert 0 < info["tiles_local"] < _tiles(M_SIM)
    whole = _golden(kp_name("rbf", "f64", M_SIM))["kp"]
    assert not np.array_equal(want, whole)
    for k, g in enumerate(got):
        assert np.array_equal(g, want), (sim, cache, k, np.abs(g - want).max())


@pytest.mark.parametrize("single_steps", [False, True])
def test_cg_of_60_iterations(single_steps):
    want = _golden("cg_rbf_f64_1100")
    assert len(want["trace"]) == CG_ITERS + 1 and np.isfinite(want["trace"]).all()
    x, trace = cg60(single_steps)
    assert np.array_equal(trace, want["trace"]), np.abs(trace - want["trace"]).max()
    assert np.array_equal(x, want["x"]), np.abs(x - want["x"]).max()


def test_learn_multi_of_three_classes():
    """The MULTI slabs go through the same pass: per class bitwise the single solve, as in test_gpu_multiclass.py."""
    m, imax = M_CG, 100
    X, _ = _data(m, "f64")
    lab = np.random.default_rng(41).integers(0, CLASSES, m + 1)
    classes, Y = pm.one_vs_all(lab, np.dtype(np.float64))
    assert len(classes) == CLASSES

    def context():
        p = pm.Parameter("rbf", gamma=1.0 / D, epsilon=1e-4, real_type=np.float64)
        p.data = X
        return pm.CSVM(p)

    singles = []
    with context() as svm:
        svm.setup_data_on_device()
        for k in range(CLASSES):
            svm.params.labels = Y[k]
            svm.learn(imax)
            singles.append((svm.alpha.copy(), svm.bias, svm.iters, svm.trace.copy()))
    with context() as svm:
        svm.learn_multi(lab, imax)
        assert svm.info()["multi_width"] >= 2
        assert np.array_equal(svm.classes, classes)
        for k, (alpha, bias, iters, trace) in enumerate(singles):
            assert 0 < iters
            assert svm.iters_multi[k] == iters, (k, svm.iters_multi, iters)
            assert np.array_equal(svm.traces[k], trace), k
            assert np.array_equal(svm.alphas[k], alpha), k
            assert svm.biases[k] == bias, k


def test_partial_cache(monkeypatch):
    """About half of m = 1100's 45 tiles stored: one stream launch and one compute launch feed the same slab."""
    m, want_tiles = M_CG, 22
    rec = TILE * TILE * 8
    monkeypatch.setenv("PLSSVM_MI_MEM_BUDGET", str(want_tiles * rec + rec // 2))
    want = _golden(kp_name("rbf", "f64", m))["kp"]
    got, info = kp_twice("rbf", "f64", m, True)
    assert info["kp_cache_tiles"] == want_tiles
    for k, g in enumerate(got):
        assert np.array_equal(g, want), (k, np.abs(g - want).max())
