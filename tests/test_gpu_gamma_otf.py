"""Gamma lanes on the sparse on-the-fly path: one walk over the pairs serves up to 8 rbf widths, and
every lane is BITWISE a fresh on-the-fly context created with its gamma (multi_width=1: the single kernel).

The shapes are tests/test_gpu_otf_lanes.py's. windows: m = 2100, one row past a partner window in fp32 (2048) and past
two in fp64 (1024). ragged: m = 300, three rows of 70 entries (past the 64 features held in registers), column 0 in all
300 rows (a segment longer than a wave), signed values, an empty last point. The grid logspace(-2, 2, 11) runs as groups
of 8 + 3 and holds factored and direct lanes on every (shape, dtype); on ragged fp32 the first group mixes them."""
import ctypes
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

DTYPES = {"f64": np.float64, "f32": np.float32}
COST, NVEC, IMAX = 10.0, 11, 80
GAMMAS = np.logspace(-2, 2, NVEC)
COSTS = np.where(np.arange(NVEC) % 2 == 1, 1000.0, COST)  # a cost of its own on half the lanes


def _windows():
    csr, y = datagen.sparse_csr(2101, 40, 6, seed=11, dtype=np.float32)
    return csr, y


def _ragged():
    n, d, rng = 301, 200, np.random.default_rng(12)
    rows = [np.r_[0, 1 + np.sort(rng.choice(d - 1, 69 if i in (5, 150, 299) else 5, replace=False))] for i in range(n - 1)]
    rows.append(np.zeros(0, np.int64))
    col = np.concatenate(rows).astype(np.int32)
    val = (rng.uniform(0.05, 1.0, col.size) * rng.choice([-1.0, 1.0], col.size)).astype(np.float32)
    csr = (np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64), col, val, n, d)
    return csr, np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    (rowptr, col, val, n, d), y = {"windows": _windows, "ragged": _ragged}[shape]()
    m, rng = n - 1, np.random.default_rng(13)
    P = rng.uniform(-1, 2, (NVEC, m))
    P[0] = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)  # signed, zero sum
    P[1] = 0.0
    P[1, m - 1] = 1.0
    return (rowptr, col, val.astype(DTYPES[dtype]), n, d), P.astype(DTYPES[dtype]), y.astype(DTYPES[dtype])


def _svm(shape, dtype, gamma=0.1, kernel="rbf", eps=1e-6, class_weight=None, sparse_algo="onthefly", **opts):
    csr, _, y = _case(shape, dtype)
    p = pm.Parameter(kernel, gamma=float(gamma), cost=COST, epsilon=eps, real_type=DTYPES[dtype], class_weight=class_weight)
    p.csr, p.labels = csr, y
    return pm.CSVM(p, sparse_algo=sparse_algo, **opts)


@functools.lru_cache(maxsize=None)
def _fresh(shape, dtype, rbf_form):
    """Per gamma, on a fresh single-kernel context: its pair form and add * Q~ P_l for add = +-1."""
    P, out = _case(shape, dtype)[1], []
    for g, p in zip(GAMMAS, P):
        with _svm(shape, dtype, g, multi_width=1, rbf_form=rbf_form) as one:
            one.setup_data_on_device()
            one.generate_q()
            out.append((bool(one.info()["rbf_factored"]), {a: one.run_device_kernel(None, np.zeros_like(p), p, a).copy() for a in (1.0, -1.0)}))
    return out


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype):
    """Q~_gamma P_l in long double from the densified rows, at the gammas as the device holds them."""
    csr, P, _ = _case(shape, dtype)
    X = datagen.densify(csr, np.float64).astype(np.longdouble)
    G = X @ X.T
    D, m, ci = np.diag(G)[:, None] + np.diag(G)[None, :] - 2 * G, X.shape[0] - 1, 1 / np.longdouble(COST)
    want = []
    for g, p in zip(GAMMAS.astype(DTYPES[dtype]), P.astype(np.longdouble)):
        K = np.exp(-np.longdouble(g) * D)
        q = K[:m, m]
        want.append(K[:m, :m] @ p - q * p.sum() - q @ p + (K[m, m] + ci) * p.sum() + ci * p)
    return np.array(want)


@pytest.mark.parametrize("shape,dtype,nvec,rbf_form", [(s, t, n, 0) for s in ("windows", "ragged") for t in ("f32", "f64") for n in (3, 8, 11)]
                         + [("ragged", "f32", 8, 1)])
def test_kp_lane_is_bitwise_the_fresh_context(shape, dtype, nvec, rbf_form):
    P, fresh, want = _case(shape, dtype)[1], _fresh(shape, dtype, rbf_form), _reference(shape, dtype)[:nvec]
    forms = [f for f, _ in fresh]
    if rbf_form == 0:  # both forms run, and on ragged fp32 they share the first group
        assert True in forms and False in forms and (len(set(forms[:8])) == 2) == ((shape, dtype) == ("ragged", "f32")), forms
    else:
        assert not any(forms)
    with _svm(shape, dtype, rbf_form=rbf_form) as svm:
        svm.setup_data_on_device()
        for add in (1.0, -1.0):
            got = svm.run_device_kernel_gammas(GAMMAS[:nvec], np.zeros_like(P[:nvec]), P[:nvec], add)
            for l in range(nvec):
                assert np.array_equal(got[l], fresh[l][1][add]), (l, add, forms[l], np.abs(got[l] - fresh[l][1][add]).max())
            err = np.abs(got - add * want).max(axis=1) / np.abs(want).max(axis=1)
            print("lane errors:", err.astype(np.float64))
            assert (err <= (1e-12 if dtype == "f64" else 1e-4)).all(), err
        info = svm.info()
        assert info["sparse_algo"] == _abi.SPARSE_ONTHEFLY and info["multi_width"] >= 2


@pytest.mark.parametrize("shape,dtype,class_weight", [(s, t, None) for s in ("windows", "ragged") for t in ("f32", "f64")]
                         + [("ragged", "f64", {1.0: 3.0})])
def test_learn_gammas_is_bitwise_the_fresh_learns(shape, dtype, class_weight):
    eps = 1e-6 if dtype == "f64" else 1e-4
    ref = []
    for g, c in zip(GAMMAS, COSTS):
        with _svm(shape, dtype, g, eps=eps, class_weight=class_weight, multi_width=1) as one:
            one.setup_data_on_device()
            one.set_cost(c)
            one.learn(IMAX)
            ref.append((one.alpha.copy(), one.bias, one.iters, one.trace.copy()))
    iters = [r[2] for r in ref]
    print("iterations per lane:", iters)
    assert len(set(iters)) > 1 and max(iters) > 50, iters  # lanes stop at different times, one past the iteration-50 reset
    with _svm(shape, dtype, eps=eps, class_weight=class_weight) as svm:
        svm.learn(IMAX)
        own = (svm.alpha.copy(), svm.bias, svm.iters, svm.trace.copy())
        svm.learn_gammas(GAMMAS, COSTS, IMAX)
        for k, (alpha, bias, it, trace) in enumerate(ref):
            assert svm.iters_multi[k] == it, (k, svm.iters_multi, iters)
            assert np.array_equal(svm.traces[k], trace) and np.array_equal(svm.alphas[k], alpha) and svm.biases[k] == bias, k
        # the context is untouched by the call, and by one refused for a bad gamma
        bad, out = (ctypes.c_double * 2)(0.1, -1.0), np.zeros((2, svm.num_data_points), dtype=DTYPES[dtype])
        y = np.ascontiguousarray(svm.params.labels, dtype=DTYPES[dtype])
        assert _abi.lib().plssvm_mi_learn_gammas(svm._ctx, y.ctypes.data_as(ctypes.c_void_p), bad, None, 2, 5, 1e-3,
                                                 out.ctypes.data_as(ctypes.c_void_p), None, None, None) == -1
        svm.learn(IMAX)
        assert np.array_equal(svm.alpha, own[0]) and svm.bias == own[1] and svm.iters == own[2] and np.array_equal(svm.trace, own[3])


@pytest.mark.parametrize("name,kernel,opts", [
    ("expansion", "rbf", dict(sparse_algo="expansion")), ("pattern", "rbf", dict(sparse_algo="pattern")),
    ("densified", "rbf", dict(sparse_algo="dense")), ("polynomial", "polynomial", {}),
    ("simulated rank", "rbf", dict(sim_rank=(0, 2))), ("one at a time", "rbf", dict(multi_width=1))])
def test_refusals(name, kernel, opts):
    P = _case("ragged", "f64")[1]
    with _svm("ragged", "f64", kernel=kernel, **opts) as svm:
        svm.setup_data_on_device()
        for call in (lambda: svm.run_device_kernel_gammas(GAMMAS[:2], np.zeros_like(P[:2]), P[:2], 1.0), lambda: svm.learn_gammas(GAMMAS[:2])):
            with pytest.raises(_abi.BackendError, match="gamma lanes run on") as e:
                call()
            assert e.value.code == -5, name
        assert np.isfinite(svm.generate_q()).all()  # the context stays usable
