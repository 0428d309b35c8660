"""GPU tests of point weights (plssvm_mi_set_point_weights) and of lanes that differ in their diagonal
(plssvm_mi_learn_lanes): per-point costs C s_i, cost grids and one-vs-all with weighted positives.

The arithmetic under test: row i's diagonal term of Q~p is ((1/C)(1/s_i)) p_i, QA_cost = k(x_m, x_m) + (1/C)(1/s_m), both
reciprocals and their product rounded in the real type; everything else of Q~p and of learn's tail as without weights.

Shapes n x d = 131 x 5 (two tile rows, a diagonal and an off-diagonal tile) and 301 x 37 (three ragged tile rows).
Data: rng = default_rng(0); y_i = +1 where i % 4 == 0, else -1; X = normal(n, d) + 1.5 y on the first three features,
divided by max|X|; gamma = 1/d rounded to float32; s_i = 4 for the positives, 1 otherwise. imax = 2000 is passed
explicitly (the default, num_features, is 5). The references are float64 numpy on the rounded inputs.

Bars: K.p 1e-12 (fp64) / 1e-4 (fp32) of max|Q~p|, the project's K.p bar. Whatever the library promises bitwise (uniform
weights, lanes against single solves, restored state) is compared with np.array_equal. The bar of the solved system is
derived inside test_solves_the_weighted_system.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")
DTYPES = [np.float64, np.float32]
SHAPES = [(131, 5), (301, 37)]
KP_TOL = {np.float64: 1e-12, np.float32: 1e-4}
IMAX = 2000
# the bitwise comparisons solve this far, so that they cross the 50th iteration's explicit residual and a replayed block
EPS = {np.float64: 1e-10, np.float32: 1e-5}
ERR_ARG = -1


def kernel_matrix(kernel, X, gamma, coef0=0.0, degree=3):
    X = np.asarray(X, dtype=np.float64)
    if kernel == "laplacian":
        D = np.empty((X.shape[0], X.shape[0]))
        for a in range(0, X.shape[0], 64):
            D[a:a + 64] = np.abs(X[a:a + 64, None, :] - X[None, :, :]).sum(-1)
        return np.exp(-gamma * D)
    G = X @ X.T
    if kernel == "linear":
        return G
    if kernel == "polynomial":
        return (gamma * G + coef0) ** degree
    nrm = np.diag(G)
    return np.exp(-gamma * np.maximum(nrm[:, None] + nrm[None, :] - 2 * G, 0.0))


@functools.lru_cache(maxsize=None)
def dense_case(n, d, dtype, kernel):
    """X, y, s in the real type, gamma as the device holds it, K [n][n] in float64; computed once and shared."""
    rng = np.random.default_rng(0)
    y = np.where(np.arange(n) % 4 == 0, 1.0, -1.0)
    X = rng.normal(size=(n, d))
    X[:, :3] += 1.5 * y[:, None]
    X /= np.abs(X).max()
    X = X.astype(dtype)
    g = float(np.float32(1.0 / d))
    s = np.where(y > 0, 4.0, 1.0)
    K = kernel_matrix(kernel, X, g)
    for a in (X, y, s, K):
        a.setflags(write=False)
    return X, y.astype(dtype), s.astype(dtype), g, K


def dense_svm(kernel, X, y, gamma, dtype, cost=1.0, epsilon=1e-3, **kw):
    p = pm.Parameter(kernel, gamma=gamma, cost=cost, epsilon=epsilon, real_type=dtype)
    p.data = np.ascontiguousarray(X, dtype=dtype)
    p.labels = None if y is None else np.asarray(y, dtype=dtype)
    return pm.CSVM(p, **kw)


@functools.lru_cache(maxsize=None)
def csr_case(dtype):
    """tests/test_gpu_sparse.py's small matrix: 300 x 500, 10 entries per row; with its dense float64 form."""
    csr, y = datagen.sparse_csr(300, 500, 10, seed=800, dtype=dtype)
    rowptr, col, val, n, d = csr
    Xd = np.zeros((n, d))
    for i in range(n):
        Xd[i, col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]].astype(dtype)
    s = np.where(np.arange(n) % 3 == 0, 4.0, 1.0).astype(dtype)
    s[-1] = 2.0
    return csr, np.asarray(y, dtype=dtype), Xd, s


def csr_svm(csr, kernel, dtype, y=None, algo="auto", mode="auto", cost=1.0, coef0=1.0, epsilon=1e-3, **kw):
    rowptr, col, val, n, d = csr
    p = pm.Parameter(kernel, gamma=1.0 / d, coef0=coef0, real_type=dtype, cost=cost, epsilon=epsilon)
    p.csr = (rowptr, col, val.astype(dtype), n, d)
    p.labels = y
    return pm.CSVM(p, kp_mode=mode, sparse_algo=algo, **kw)


def weighted_kp(K, s, cost, p64, add, dtype):
    """add * Q~p in float64 with the diagonal and QA_cost as the real type rounds them."""
    m = K.shape[0] - 1
    t = np.dtype(dtype).type
    cinv = t(1) / t(cost)
    diag = (cinv * (t(1) / np.asarray(s, dtype=dtype))).astype(np.float64)  # (1/C)(1/s_i), each step rounded in T
    q = K[:m, m]
    qa = K[m, m] + diag[m]
    return add * (K[:m, :m] @ p64 + (qa - q) * p64.sum() - q @ p64 + diag[:m] * p64), qa


def assert_kp_close(got, want, dtype, what):
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    print(f"{what}: max abs error {err:.3e} = {err / scale:.3e} of max|want| {scale:.3e} (bar {KP_TOL[dtype]:.0e})")
    assert err <= KP_TOL[dtype] * scale, (what, err, scale)


def kp_vectors(m, dtype):
    rng = np.random.default_rng(5 + m)
    return {"positive": rng.uniform(1.0, 2.0, m).astype(dtype), "signed": rng.uniform(-1.0, 2.0, m).astype(dtype)}


def solved(svm):
    return svm.alpha.copy(), svm.bias, int(svm.iters), svm.trace.copy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def lane(svm, k):
    return svm.alphas[k].copy(), svm.biases[k], int(svm.iters_multi[k]), svm.traces[k].copy()


# ---- 1. K.p values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["rbf", "laplacian"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weighted_kp_dense(shape, kernel, dtype):
    n, d = shape
    X, y, s, g, K = dense_case(n, d, dtype, kernel)
    m, cost = n - 1, 0.5
    with dense_svm(kernel, X, y, g, dtype, cost=cost) as svm:
        svm.set_point_weights(s)
        svm.generate_q()
        for name, p in kp_vectors(m, dtype).items():
            for add in (1.0, -1.0):
                want, qa = weighted_kp(K, s, cost, p.astype(np.float64), add, dtype)
                assert abs(float(svm.QA_cost) - qa) <= KP_TOL[dtype] * qa
                ret = svm.run_device_kernel(None, np.zeros(m, dtype=dtype), p, add)
                assert_kp_close(ret, want, dtype, f"{kernel} {n}x{d} {name} add={add:g}")
        # the weights change the product by far more than the bar: the check above is one of the weights
        plain, _ = weighted_kp(K, np.ones(n), cost, p.astype(np.float64), -1.0, dtype)
        assert np.abs(plain - want).max() > 100 * KP_TOL[dtype] * np.abs(want).max()


SPARSE_PATHS = [("linear", "auto", "auto", 0), ("rbf", "auto", "auto", _abi.SPARSE_EXPANSION),
                ("polynomial", "auto", "auto", _abi.SPARSE_EXPANSION), ("rbf", "auto", "pattern", _abi.SPARSE_PATTERN),
                ("rbf", "auto", "onthefly", _abi.SPARSE_ONTHEFLY), ("rbf", "auto", "dense", _abi.SPARSE_DENSE)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,mode,algo,want_algo", SPARSE_PATHS, ids=lambda v: str(v))
def test_weighted_kp_sparse_paths(kernel, mode, algo, want_algo, dtype):
    csr, y, Xd, s = csr_case(dtype)
    n, d = Xd.shape
    m, cost = n - 1, 0.5
    K = kernel_matrix(kernel, Xd, float(np.dtype(dtype).type(1.0 / d)), coef0=1.0)
    with csr_svm(csr, kernel, dtype, algo=algo, mode=mode, cost=cost) as svm:
        svm.set_point_weights(s)
        svm.generate_q()
        info = svm.info()
        assert info["is_sparse"] == 1 and info["sparse_algo"] == want_algo
        assert (info["kp_mode"] == _abi.KP_FACTORED) == (kernel == "linear")
        for name, p in kp_vectors(m, dtype).items():
            want, _ = weighted_kp(K, s, cost, p.astype(np.float64), -1.0, dtype)
            ret = svm.run_device_kernel(None, np.zeros(m, dtype=dtype), p, -1.0)
            assert_kp_close(ret, want, dtype, f"csr {kernel} {algo} {name}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_weighted_kp_simulated_ranks_sum_to_the_product(dtype):
    n, d = 301, 37
    X, y, s, g, K = dense_case(n, d, dtype, "rbf")
    m, W = n - 1, 3
    p = kp_vectors(m, dtype)["signed"]

    def product(sim):
        with dense_svm("rbf", X, y, g, dtype, cost=0.5, sim_rank=sim) as svm:
            svm.set_point_weights(s)
            svm.generate_q()
            return svm.run_device_kernel(None, np.zeros(m, dtype=dtype), p, 1.0).astype(np.float64)

    whole = product(None)
    shares = sum(product((r, W)) for r in range(W))
    want, _ = weighted_kp(K, s, 0.5, p.astype(np.float64), 1.0, dtype)
    assert_kp_close(whole, want, dtype, "single rank")
    assert_kp_close(shares, whole, dtype, "sum of the simulated ranks' shares")


# ---- 2. uniform weights are the unweighted bits ----------------------------------------------------------------------
def uniform_contexts(dtype):
    X, y, s, g, _ = dense_case(301, 37, dtype, "rbf")
    csr, yc, _, sc = csr_case(dtype)
    e = 0.0  # no stop: every solve runs its 120 iterations, through two explicit residuals and one replayed block
    return [("dense rbf", lambda: dense_svm("rbf", X, y, g, dtype, cost=20.0, epsilon=e), s, 120),
            ("csr linear", lambda: csr_svm(csr, "linear", dtype, y=yc, cost=20.0, epsilon=e), sc, 120),
            ("csr rbf", lambda: csr_svm(csr, "rbf", dtype, y=yc, cost=20.0, epsilon=e), sc, 120)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2], ids=["dense-rbf", "csr-linear", "csr-rbf"])
def test_uniform_weights_are_todays_bits(which, dtype):
    name, make, s, imax = uniform_contexts(dtype)[which]
    with make() as svm:
        plain = solved(svm.learn(imax))
        svm.set_point_weights(np.ones_like(s))
        ones = solved(svm.learn(imax))
        svm.set_point_weights(s)
        weighted = solved(svm.learn(imax))
        svm.set_point_weights(None)
        cleared = solved(svm.learn(imax))
        svm.learn_costs([20.0], imax)
        grid = lane(svm, 0)
    print(f"{name}: {plain[2]} iterations, weighted {weighted[2]}")
    # (dense and CSR linear run all 120; the fp32 kernel expansion's recurrence residual reaches 0 after 49 and stops)
    assert plain[2] > 0 and np.isfinite(plain[0]).all()
    assert same(ones, plain), "uniform weights changed the solve"
    assert not np.array_equal(weighted[0], plain[0]), "the weights were ignored"
    assert same(cleared, plain), "clearing the weights did not restore the solve"
    assert same(grid, plain), "learn_costs([C]) is not learn() at C"


# ---- 3. lanes are the single solves ----------------------------------------------------------------------------------
COSTS = [0.1, 1.0, 10.0, 0.3, 3.0, 300.0, 0.5, 2.0, 5.0, 0.2, 20.0]


@functools.lru_cache(maxsize=None)
def lane_inputs(n, dtype):
    """11 lanes: labels (the recipe's, their negation, and rotations of them), the cost list, weights in [0.5, 4]."""
    rng = np.random.default_rng(n)
    y = np.where(np.arange(n) % 4 == 0, 1.0, -1.0)
    Y = np.stack([np.roll(y, k) * (-1.0 if k % 2 else 1.0) for k in range(11)]).astype(dtype)
    S = rng.uniform(0.5, 4.0, size=(11, n)).astype(dtype)
    S[3] = 1.0  # one lane with uniform weights
    return np.ascontiguousarray(Y), np.array(COSTS), np.ascontiguousarray(S)


@functools.lru_cache(maxsize=None)
def lane_references(n, d, dtype, kernel):
    """set_cost(c_k); set_point_weights(S_k); learn(Y_k) for the 11 lanes, on a context of their own."""
    X, y, s, g, _ = dense_case(n, d, dtype, kernel)
    Y, costs, S = lane_inputs(n, dtype)
    out = []
    with dense_svm(kernel, X, y, g, dtype, epsilon=EPS[dtype]) as svm:
        for k in range(11):
            svm.params.labels = Y[k]
            svm.set_cost(costs[k])
            svm.set_point_weights(S[k])
            out.append(solved(svm.learn(IMAX)))
    return out


def run_lanes(svm, Y, costs, S, nlane):
    svm._learn_lanes(np.ascontiguousarray(Y[:nlane]), costs[:nlane], np.ascontiguousarray(S[:nlane]), IMAX)
    return [lane(svm, k) for k in range(nlane)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,shape", [("rbf", (301, 37)), ("laplacian", (131, 5))], ids=["rbf-301x37", "laplacian-131x5"])
@pytest.mark.parametrize("graph", ["graph-on", "graph-off"])
@pytest.mark.parametrize("cache", [True, False], ids=["cache-on", "cache-off"])
@pytest.mark.parametrize("width", [None, 2, 1], ids=["w-auto", "w2", "w1"])
def test_lanes_are_the_single_solves(width, cache, graph, kernel, shape, dtype, monkeypatch):
    n, d = shape
    if graph == "graph-off":
        monkeypatch.setenv("PLSSVM_MI_GRAPH", "0")
    else:
        monkeypatch.delenv("PLSSVM_MI_GRAPH", raising=False)
    X, y, s, g, _ = dense_case(n, d, dtype, kernel)
    Y, costs, S = lane_inputs(n, dtype)
    refs = lane_references(n, d, dtype, kernel)
    with dense_svm(kernel, X, y, g, dtype, cost=3.0, epsilon=EPS[dtype], multi_width=width, kp_cache=cache) as svm:
        svm.set_point_weights(s)
        before = solved(svm.learn(IMAX))
        assert svm.info()["multi_width"] == {None: 8, 2: 2, 1: 1}[width]
        for nlane in (3, 8, 11):
            got = run_lanes(svm, Y, costs, S, nlane)
            for k in range(nlane):
                assert got[k][2] > 0
                assert same(got[k], refs[k]), f"lane {k} of {nlane} (width {width}, cache {cache}, {graph})"
        # cost-only lanes on the context's own weights, and one weight row for every lane
        svm.learn_costs(costs[:3], IMAX)
        shared = [lane(svm, k) for k in range(3)]
        svm._learn_lanes(np.ascontiguousarray(np.tile(y, (3, 1))), costs[:3], s, IMAX)
        one_row = [lane(svm, k) for k in range(3)]
        after = solved(svm.learn(IMAX))
        for k in range(3):
            svm.set_cost(costs[k])
            single = solved(svm.learn(IMAX))
            assert same(shared[k], single) and same(one_row[k], single), f"cost lane {k}"
    assert same(after, before), "the context's cost or weights were not restored"
    assert not same(refs[0], refs[1])
    print(f"iterations per lane: {[r[2] for r in refs]}")
    assert max(r[2] for r in refs) > 50, "some lane must cross the explicit residual of the 50th iteration"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_lanes_on_a_csr_context_run_one_after_another(kernel, dtype):
    csr, yc, _, sc = csr_case(dtype)
    n = csr[3]
    Y, costs, S = lane_inputs(n, dtype)
    with csr_svm(csr, kernel, dtype, y=yc, cost=3.0, epsilon=EPS[dtype]) as svm:
        svm.set_point_weights(sc)
        before = solved(svm.learn(60))
        assert svm.info()["multi_width"] == 1
        svm._learn_lanes(np.ascontiguousarray(Y[:3]), costs[:3], np.ascontiguousarray(S[:3]), 60)
        got = [lane(svm, k) for k in range(3)]
        after = solved(svm.learn(60))
        for k in range(3):
            svm.params.labels = Y[k]
            svm.set_cost(costs[k])
            svm.set_point_weights(S[k])
            assert same(got[k], solved(svm.learn(60))), f"lane {k}"
    assert same(after, before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_learn_multi_class_weight_is_the_weighted_learn_per_class(dtype):
    n, d = 301, 37
    rng = np.random.default_rng(3)
    labels = np.arange(n) % 3 + 5
    X = rng.normal(size=(n, d))
    X[:, :3] += 2.0 * np.eye(3)[labels - 5]
    X = (X / np.abs(X).max()).astype(dtype)
    cw = {5: 3.0, 7: 0.5}
    g = float(np.float32(1.0 / d))
    with dense_svm("rbf", X, None, g, dtype, epsilon=EPS[dtype]) as svm:
        svm.learn_multi(labels, IMAX, class_weight=cw)
        assert np.array_equal(svm.classes, [5, 6, 7])
        got = [lane(svm, c) for c in range(3)]
        svm.learn_multi(labels, IMAX)
        plain = [lane(svm, c) for c in range(3)]
        _, Yc = pm.one_vs_all(labels, dtype)
        for c, cls in enumerate(svm.classes):
            svm.params.labels = Yc[c]
            svm.set_point_weights(np.where(labels == cls, cw.get(cls, 1.0), 1.0))
            assert same(got[c], solved(svm.learn(IMAX))), f"class {cls}"
        with pytest.raises(ValueError, match="does not have"):
            svm.learn_multi(labels, IMAX, class_weight={4: 2.0})
    assert same(got[1], plain[1]) and not same(got[0], plain[0]) and not same(got[2], plain[2])


# ---- 4. it solves the weighted system --------------------------------------------------------------------------------
def numpy_cg(Q, b, eps, imax):
    """The reference recurrence in Q's dtype: x0 = 1, explicit residual every 50th iteration (as numpy_cg of
    tests/test_gpu_laplacian.py)."""
    t = Q.dtype.type
    x = np.ones(Q.shape[0], dtype=Q.dtype)
    r = b - Q @ x
    dv = r.copy()
    delta = r @ r
    d0 = delta
    for it in range(imax):
        Ad = Q @ dv
        a = delta / (dv @ Ad)
        x = x + a * dv
        r = b - Q @ x if it % 50 == 49 else r - a * Ad
        dn = r @ r
        if dn <= t(eps) ** 2 * d0:
            break
        dv = dn / delta * dv + r
        delta = dn
    return x


def direct_solution(K, s, cost, y):
    n = K.shape[0]
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = K + np.diag(1.0 / (cost * s))
    A[:n, n] = A[n, :n] = 1.0
    z = np.linalg.solve(A, np.concatenate([y, [0.0]]))
    return z[:n], z[n]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cost", [1.0, 10.0])
@pytest.mark.parametrize("kernel", ["rbf", "laplacian"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_solves_the_weighted_system(shape, kernel, cost, dtype):
    """alpha (all n entries) and the bias against numpy's direct solve of the bordered system
    [[K + diag(1/(C s)), 1], [1^T, 0]] [alpha; b] = [y; 0], at epsilon = 1e-10 (fp64) / 1e-5 (fp32).

    The bar is 10x what the reference recurrence itself leaves when numpy runs it in the same real type on the explicit
    Q~ (the GPU sums in another order), measured as max|alpha - alpha_direct| / max|alpha_direct| (the bias error on the
    same scale, the larger of the two), and at most 0.05. The cap is a condition of the test: the unweighted solution is
    at least 0.27 of max|alpha| away, which is asserted too, so a solve that ignored the weights fails."""
    n, d = shape
    X, y, s, g, K = dense_case(n, d, dtype, kernel)
    m = n - 1
    eps = 1e-10 if dtype == np.float64 else 1e-5
    y64, s64 = y.astype(np.float64), s.astype(np.float64)
    a_ref, b_ref = direct_solution(K, s64, cost, y64)
    a_plain, _ = direct_solution(K, np.ones(n), cost, y64)
    scale = np.abs(a_ref).max()
    sep = np.abs(a_plain - a_ref).max() / scale
    assert sep >= 0.27, sep

    def errors(alpha, bias):
        return max(np.abs(np.asarray(alpha, dtype=np.float64) - a_ref).max(), abs(float(bias) - b_ref)) / scale

    diag = 1.0 / (cost * s64)
    q = K[:m, m]
    qa = K[m, m] + diag[m]
    Q = (K[:m, :m] + qa - q[:, None] - q[None, :] + np.diag(diag[:m])).astype(dtype)
    x = numpy_cg(Q, (y64[:m] - y64[m]).astype(dtype), eps, IMAX).astype(np.float64)
    own = errors(np.concatenate([x, [-x.sum()]]), y64[m] + qa * x.sum() - q @ x)
    bar = 10.0 * own
    assert 0 < bar <= 0.05, (own, "the numpy reference itself is outside the cap")
    with dense_svm(kernel, X, y, g, dtype, cost=cost, epsilon=eps) as svm:
        svm.set_point_weights(s)
        svm.learn(IMAX)
        err = errors(svm.alpha, svm.bias)
        iters = svm.iters
    print(f"{kernel} {n}x{d} C={cost:g} {np.dtype(dtype).name}: {iters} iterations, error {err:.3e} of max|alpha|, numpy's own "
          f"{own:.3e}, bar {bar:.3e}, unweighted solution {sep:.3f} away")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_fused_sparse_finalizes_take_the_weights(kernel, dtype):
    """The CG iteration of the factored sparse linear path and of the kernel expansion forms Q~d in a fused finalize of
    its own (not the kernel test 1 reaches). Three iterations from x0 = 1 against the same three iterations in float64
    numpy. Each iterate is a rational function of a handful of K.p products, each within the K.p bar; 100x that bar of
    max|x| leaves room for three of them compounding, and the unweighted diagonal moves x by far more (asserted)."""
    csr, yc, Xd, sc = csr_case(dtype)
    n, d = Xd.shape
    m, cost = n - 1, 0.5
    K = kernel_matrix(kernel, Xd, float(np.dtype(dtype).type(1.0 / d)))

    def three(s):
        t = np.dtype(dtype).type
        diag = ((t(1) / t(cost)) * (t(1) / np.asarray(s, dtype=dtype))).astype(np.float64)
        q = K[:m, m]
        Q = K[:m, :m] + (K[m, m] + diag[m]) - q[:, None] - q[None, :] + np.diag(diag[:m])
        y64 = yc.astype(np.float64)
        return numpy_cg(Q, y64[:m] - y64[m], 0.0, 3)

    want, plain = three(sc), three(np.ones(n))
    with csr_svm(csr, kernel, dtype, y=yc, cost=cost, epsilon=0.0) as svm:
        svm.set_point_weights(sc)
        svm.generate_q()
        x = svm.solver_CG((yc[:m] - yc[m]).astype(dtype), 3, 0.0).astype(np.float64)
        assert svm.iters == 3
    scale = np.abs(want).max()
    err = np.abs(x - want).max() / scale
    print(f"csr {kernel} {np.dtype(dtype).name}: three iterations within {err:.3e} of max|x|; unweighted {np.abs(plain - want).max() / scale:.3e}")
    assert np.abs(plain - want).max() / scale > 10 * 100 * KP_TOL[dtype]
    assert err <= 100 * KP_TOL[dtype]


# ---- 5. errors leave the context usable ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_leave_the_context_usable(dtype):
    n, d = 131, 5
    X, y, s, g, _ = dense_case(n, d, dtype, "rbf")
    Y, costs, S = lane_inputs(n, dtype)
    L = _abi.lib()
    with dense_svm("rbf", X, y, g, dtype, cost=2.0) as svm:
        with pytest.raises(pm.BackendError) as e:  # before a setup
            svm._check(L.plssvm_mi_set_point_weights(svm._ctx, pm._ptr(np.ascontiguousarray(s))))
        assert e.value.code == ERR_ARG
        svm.set_point_weights(s)
        before = solved(svm.learn(IMAX))
        for bad in (0.0, -1.0, np.nan, np.inf):
            w = s.copy()
            w[n // 2] = bad
            with pytest.raises(pm.BackendError) as e:
                svm.set_point_weights(w)
            assert e.value.code == ERR_ARG
        assert same(solved(svm.learn(IMAX)), before), "a rejected weight vector changed the context's weights"

        def lanes(Yk, nlane, ldy, cc, SS, lds):
            K = max(nlane, 1)
            al, bi, it = np.zeros((K, n), dtype=dtype), np.zeros(K), np.zeros(K, dtype=np.int64)
            return L.plssvm_mi_learn_lanes(svm._ctx, pm._ptr(Yk), nlane, ldy, pm._ptr(cc), pm._ptr(SS), lds, IMAX, 1e-3,
                                           pm._ptr(al), pm._ptr(bi), None, pm._ptr(it))

        Y3, S3, c3 = np.ascontiguousarray(Y[:3]), np.ascontiguousarray(S[:3]), costs[:3].copy()
        assert lanes(Y3, 3, n, c3, S3, n) == _abi.OK
        assert lanes(Y3, 0, n, c3, S3, n) == ERR_ARG
        assert lanes(Y3, 3, n - 1, c3, S3, n) == ERR_ARG
        assert lanes(Y3, 3, n, c3, S3, n - 1) == ERR_ARG
        for bad in (0.0, -2.0, np.nan, np.inf):
            cb = c3.copy()
            cb[1] = bad
            assert lanes(Y3, 3, n, cb, S3, n) == ERR_ARG
            Sb = S3.copy()
            Sb[2, 7] = bad
            assert lanes(Y3, 3, n, c3, Sb, n) == ERR_ARG
            assert lanes(Y3, 3, n, c3, np.ascontiguousarray(Sb[2]), 0) == ERR_ARG
        assert same(solved(svm.learn(IMAX)), before), "a rejected call changed the context"


# ---- 6. the command line ---------------------------------------------------------------------------------------------
def write_libsvm(path, X, labels):
    with open(path, "w") as f:
        for row, lab in zip(X, labels):
            f.write(f"{lab:g} " + " ".join(f"{k}:{v!r}" for k, v in enumerate(row.tolist())) + "\n")


def model_alphas(path, binary):
    """The coefficient columns of a model file's SV lines: [n] for a binary model, [K][n] for a one-vs-all one."""
    with open(path) as f:
        lines = f.read().splitlines()
    sv = lines[lines.index("SV") + 1:]
    ncoef = 1 if binary else int(next(l for l in lines if l.startswith("nr_class")).split()[1])
    return np.array([[float(t) for t in l.split()[:ncoef]] for l in sv]).T


def test_cli_class_weights_binary(tmp_path):
    n, d = 131, 5
    X, y, s, g, _ = dense_case(n, d, np.float64, "rbf")
    f, model = tmp_path / "w.libsvm", tmp_path / "w.model"
    write_libsvm(f, X, y)
    subprocess.run([TRAIN, "-q", "-t", "2", "-g", repr(g), "--max_iter", str(IMAX), "--class_weights", "1:4", str(f), str(model)],
                   check=True)
    p = pm.Parameter("rbf", gamma=g, class_weight={1: 4.0})
    p.data, p.labels = np.array(X), np.array(y)
    with pm.CSVM(p) as svm:
        svm.learn(IMAX)
        alpha = svm.alpha
    got = model_alphas(model, True)[0]
    order = np.concatenate([np.flatnonzero(y > 0), np.flatnonzero(y < 0)])  # the file lists the positive class first
    assert np.array_equal(got, np.array([float(repr(float(a))) for a in alpha[order]]))
    plain = tmp_path / "p.model"
    subprocess.run([TRAIN, "-q", "-t", "2", "-g", repr(g), "--max_iter", str(IMAX), str(f), str(plain)], check=True)
    assert not np.array_equal(model_alphas(plain, True)[0], got)


def test_cli_class_weights_multiclass(tmp_path):
    n, d = 131, 5
    rng = np.random.default_rng(9)
    labels = np.arange(n) % 3 + 1
    X = rng.normal(size=(n, d))
    X[:, :3] += 2.0 * np.eye(3)[labels - 1]
    X /= np.abs(X).max()
    g = float(np.float32(1.0 / d))
    f, model = tmp_path / "m.libsvm", tmp_path / "m.model"
    write_libsvm(f, X, labels)
    subprocess.run([TRAIN, "-q", "-t", "2", "-g", repr(g), "--max_iter", str(IMAX), "--multiclass", "--class_weights",
                    "1:3,3:0.5", str(f), str(model)], check=True)
    p = pm.Parameter("rbf", gamma=g)
    p.data = X
    with pm.CSVM(p) as svm:
        svm.learn_multi(labels, IMAX, class_weight={1: 3.0, 3: 0.5})
        alphas = svm.alphas
    got = model_alphas(model, False)
    assert got.shape[0] == 3 and got.shape[1] == n
    # the one-vs-all file groups the support vectors by class, in class order
    order = np.concatenate([np.flatnonzero(labels == c) for c in (1, 2, 3)])
    assert np.array_equal(got, np.vectorize(lambda a: float(repr(float(a))))(alphas[:, order]))


def test_class_weight_of_learn_does_not_reach_a_later_learn_multi():
    """Parameter.class_weight is for learn(); a learn_multi that passes none trains unweighted, as on a fresh context,
    while weights the caller set with set_point_weights stay for every class."""
    n, d = 131, 5
    X, y, s, g, _ = dense_case(n, d, np.float64, "rbf")
    labels = np.arange(n) % 3
    with dense_svm("rbf", X, None, g, np.float64) as svm:
        svm.learn_multi(labels, IMAX)
        fresh = [lane(svm, c) for c in range(3)]
        svm.set_point_weights(s)
        svm.learn_multi(labels, IMAX)
        kept = [lane(svm, c) for c in range(3)]
    p = pm.Parameter("rbf", gamma=g, class_weight={1: 4.0})
    p.data, p.labels = np.array(X), np.array(y)
    with pm.CSVM(p) as svm:
        weighted = solved(svm.learn(IMAX))
        svm.learn_multi(labels, IMAX)
        after = [lane(svm, c) for c in range(3)]
        again = solved(svm.learn(IMAX))
    assert all(same(a, b) for a, b in zip(after, fresh))
    assert not any(same(a, b) for a, b in zip(kept, fresh))
    assert same(again, weighted)
