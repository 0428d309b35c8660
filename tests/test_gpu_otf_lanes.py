"""Lanes on the sparse on-the-fly path: one pass over the pairs serves up to 8 vectors, and every
lane is BITWISE the single-vector product or solve (a second context with multi_width=1, the parent's behaviour).

windows: m = 2100 is one row past a partner window in fp32 (2048) and past two in fp64 (1024). ragged: m = 300, three
rows of 70 entries (past the 64 features held in registers), column 0 in all 300 rows (a window segment longer than a
wave) and an empty last point. Both hold float32 values, so fp32 and fp64 share one long-double reference."""
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

DTYPES = {"f64": np.float64, "f32": np.float32}
COST = 10.0
# kernel, parameters, context options
VARIANTS = {
    "rbf_factored": ("rbf", dict(gamma=0.1), {}),
    "rbf_direct": ("rbf", dict(gamma=0.1), dict(rbf_form=1)),
    "poly3": ("polynomial", dict(degree=3, gamma=0.05, coef0=0.5), {}),
    "poly17": ("polynomial", dict(degree=17, gamma=0.05, coef0=0.5), {}),
    "linear": ("linear", {}, dict(kp_mode="pairwise")),
}
NVEC = 11


def _windows():
    return datagen.sparse_csr(2101, 40, 6, seed=11, dtype=np.float32)[0]


def _ragged():
    n, d, rng = 301, 200, np.random.default_rng(12)
    rows = [np.r_[0, 1 + np.sort(rng.choice(d - 1, 69 if i in (5, 150, 299) else 5, replace=False))] for i in range(n - 1)]
    rows.append(np.zeros(0, np.int64))
    col = np.concatenate(rows).astype(np.int32)
    val = (rng.uniform(0.05, 1.0, col.size) * rng.choice([-1.0, 1.0], col.size)).astype(np.float32)
    return np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64), col, val, n, d


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    rowptr, col, val, n, d = {"windows": _windows, "ragged": _ragged}[shape]()
    m, rng = n - 1, np.random.default_rng(13)
    P = rng.uniform(-1, 2, (NVEC, m))
    P[0] = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)  # signed, zero sum
    P[1] = 0.0
    P[1, m - 1] = 1.0
    return (rowptr, col, val.astype(DTYPES[dtype]), n, d), P.astype(DTYPES[dtype])


def _svm(csr, dtype, kernel="rbf", kparams=None, cost=COST, eps=1e-3, **opts):
    p = pm.Parameter(kernel, cost=cost, epsilon=eps, real_type=DTYPES[dtype], **(kparams or dict(gamma=0.1)))
    p.csr = csr
    return pm.CSVM(p, sparse_algo="onthefly", **opts)


@functools.lru_cache(maxsize=None)
def _singles(shape, dtype, variant):
    """add * Q~ P_c per vector and add = +-1 through the single product, one at a time."""
    csr, P = _case(shape, dtype)
    kernel, kparams, opts = VARIANTS[variant]
    with _svm(csr, dtype, kernel, kparams, multi_width=1, **opts) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        assert svm.info()["multi_width"] == 1
        return {a: np.stack([svm.run_device_kernel(None, np.zeros_like(p), p, a).copy() for p in P]) for a in (1.0, -1.0)}


@functools.lru_cache(maxsize=None)
def _reference(shape, variant):
    """Q~ P in long double from the densified rows: Q~_ij = k_ij - q_i - q_j + k_mm + 1/C + delta_ij / C."""
    csr, P = _case(shape, "f64")
    kernel, kp, _ = VARIANTS[variant]
    X = datagen.densify(csr, np.float64).astype(np.longdouble)
    G = X @ X.T
    if kernel == "rbf":
        nrm = np.diag(G)
        K = np.exp(-np.longdouble(kp["gamma"]) * (nrm[:, None] + nrm[None, :] - 2 * G))
    elif kernel == "polynomial":
        K = (np.longdouble(kp["gamma"]) * G + np.longdouble(kp["coef0"])) ** kp["degree"]
    else:
        K = G
    m, Pl, ci = X.shape[0] - 1, P.astype(np.longdouble).T, 1 / np.longdouble(COST)
    q = K[:m, m]
    return (K[:m, :m] @ Pl - np.outer(q, Pl.sum(0)) - (q @ Pl)[None, :] + (K[m, m] + ci) * Pl.sum(0)[None, :] + ci * Pl).T


@pytest.mark.parametrize("nvec", [3, 8, 11])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", ["windows", "ragged"])
def test_kp_lanes_are_bitwise_the_single_product(shape, dtype, variant, nvec):
    csr, P = _case(shape, dtype)
    kernel, kparams, opts = VARIANTS[variant]
    single, want = _singles(shape, dtype, variant), _reference(shape, variant)[:nvec]
    with _svm(csr, dtype, kernel, kparams, **opts) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        info = svm.info()
        assert info["sparse_algo"] == _abi.SPARSE_ONTHEFLY
        assert info["multi_width"] >= 2
        for add in (1.0, -1.0):
            got = svm.run_device_kernel_multi(None, np.zeros_like(P[:nvec]), P[:nvec], add)
            for c in range(nvec):
                assert np.array_equal(got[c], single[add][c]), (c, add, np.abs(got[c] - single[add][c]).max())
            err = np.abs(got - add * want).max(axis=1) / np.abs(want).max(axis=1)
            assert (err <= (1e-12 if dtype == "f64" else 1e-4)).all(), err


def _assert_rows_equal(svm, singles):
    for k, (alpha, bias, iters, trace) in enumerate(singles):
        assert svm.iters_multi[k] == iters, (k, svm.iters_multi, [s[2] for s in singles])
        assert np.array_equal(svm.traces[k], trace) and np.array_equal(svm.alphas[k], alpha) and svm.biases[k] == bias, k


def _one_vs_all_singles(svm, lab, imax):
    out = []
    svm.setup_data_on_device()
    for y in pm.one_vs_all(lab, svm.dtype)[1]:
        svm.params.labels = y
        svm.learn(imax)
        out.append((svm.alpha.copy(), svm.bias, svm.iters, svm.trace.copy()))
    return out


@pytest.mark.parametrize("nclass,width,imax", [(3, None, 120), (5, 2, 120)])
def test_learn_multi_is_bitwise_the_single_learns(nclass, width, imax):
    """test_lanes_on_densified_sparse_data's data and parameters on the on-the-fly path; width 2 with five classes:
    groups of 2, 2 and 1."""
    csr, _ = datagen.sparse_csr(301, 64, 8, seed=5, dtype=np.float64)
    lab = np.random.default_rng(9).integers(0, nclass, 301) * 2.5
    opts = {} if width is None else dict(multi_width=width)
    with _svm(csr, "f64", cost=100.0, eps=1e-6, multi_width=1) as svm:
        ref = _one_vs_all_singles(svm, lab, imax)
    iters = [s[2] for s in ref]
    assert len(ref) == nclass
    if width is None:
        assert 50 < max(iters) < imax, iters  # the group crosses the explicit residual of iteration 50
    with _svm(csr, "f64", cost=100.0, eps=1e-6, **opts) as svm:
        svm.learn_multi(lab, imax)
        info = svm.info()
        assert info["sparse_algo"] == _abi.SPARSE_ONTHEFLY and info["multi_width"] == (width or info["multi_width"]) >= 2
        _assert_rows_equal(svm, ref)


def test_learn_costs_is_bitwise_set_cost_and_learn():
    costs, imax = [0.1, 10.0, 1000.0], 60
    csr, y = datagen.sparse_csr(2101, 40, 6, seed=11, dtype=np.float64)
    ref = []
    with _svm(csr, "f64", multi_width=1) as svm:
        svm.params.labels = y
        for c in costs:
            svm.set_cost(c)
            svm.learn(imax)
            ref.append((svm.alpha.copy(), svm.bias, svm.iters, svm.trace.copy()))
    with _svm(csr, "f64") as svm:
        svm.params.labels = y
        svm.learn_costs(costs, imax)
        assert svm.info()["sparse_algo"] == _abi.SPARSE_ONTHEFLY and svm.info()["multi_width"] >= 2
        _assert_rows_equal(svm, ref)
