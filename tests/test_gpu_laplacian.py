"""GPU tests of the Laplacian kernel k(x, z) = exp(-gamma ||x - z||_1) on dense data: the L1-distance tile kernels
(csrc/kp_tiles.hip, csrc/predict_tiles.hip) and everything downstream of them.

The reference is float64 numpy on the already-rounded inputs, D = |X[:, None, :] - X[None, :, :]|.sum(-1),
K = exp(-gamma D); the CPU oracle does not know this kernel. Bars: the project's K.p bars of tests/test_gpu_parity.py
(absolute error <= 1e-12 of max|want| in fp64, 1e-4 in fp32), for predict scaled by max|value|; alpha / rho 1e-9 /
2e-2 and the CG residual trace 1e-6 (fp64) / 1e-3 on the first three entries (fp32), as there. Everything the library
promises bitwise (the tile cache in every record form, the batched K.p and solves, the predict contract) is compared
with np.array_equal.

Shapes: (130, 5) two tile rows, a diagonal and an off-diagonal tile, d below one chunk; (300, 37) three ragged tile
rows, d off the chunk depth; (385, 256) m = exactly three tiles; (386, 256) one row more. Data: uniform [-1, 1], the
same plus 100 (L1 differences do not cancel: no shift is needed), and gamma = 1 at (300, 37), where most values
underflow towards 0 and stored fp64 tiles stay raw. The edges: (2, 1) one row, one feature; (3, 5); (129, 16) m = exactly
one tile and d exactly one chunk of 16; (130, 17) one row and one feature more; (1100, 3) nine tile rows, i.e. two rows
of super-blocks on a single rank; (300, 37) once more with a signed vector, whose sum cancels. At m = 1100, d = 8 a
memory budget of 22 of the 45 tiles makes every K.p one launch over the stored prefix and one Laplacian KP_COMPUTE launch
over the rest.
"""
import ctypes
import functools

import numpy as np
import pytest

import cg_trace_cases as cgc
import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KP_TOL = {np.float64: 1e-12, np.float32: 1e-4}
COST = 1.0
# (n, d, offset, gamma; None: 1 / d)
KP_CASES = [(130, 5, 0.0, None), (130, 5, 100.0, None), (300, 37, 0.0, None), (300, 37, 100.0, None),
            (385, 256, 0.0, None), (385, 256, 100.0, None), (386, 256, 0.0, None), (386, 256, 100.0, None),
            (300, 37, 0.0, 1.0),
            (2, 1, 0.0, None), (3, 5, 0.0, None), (129, 16, 0.0, None), (130, 17, 0.0, None), (1100, 3, 0.0, None),
            (300, 37, 0.0, None, "signed")]  # a fifth entry: the vector is uniform(-1, 2), not [1, 2]


def l1_kernel(X, Z, gamma):
    """exp(-gamma ||x - z||_1) for every row pair, in float64."""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    D = np.empty((X.shape[0], Z.shape[0]))
    for a in range(0, X.shape[0], 64):
        D[a:a + 64] = np.abs(X[a:a + 64, None, :] - Z[None, :, :]).sum(-1)
    return np.exp(-float(gamma) * D)


def rounded_gamma(d, dtype, gamma=None):
    return float(dtype(1.0) / dtype(d)) if gamma is None else float(dtype(gamma))


@functools.lru_cache(maxsize=None)
def kp_case(n, d, offset, gamma, dtype):
    """X in the real type, gamma as the device holds it, K [n][n] in float64; computed once and shared."""
    rng = np.random.default_rng(n * 1000 + d)
    X = (rng.uniform(-1.0, 1.0, size=(n, d)) + offset).astype(dtype)
    g = rounded_gamma(d, dtype, gamma)
    K = l1_kernel(X, X, g)
    X.setflags(write=False)
    K.setflags(write=False)
    return X, g, K


def make_svm(X, gamma, dtype, labels=None, epsilon=1e-3, **kw):
    p = pm.Parameter("laplacian", gamma=gamma, cost=COST, epsilon=epsilon, real_type=dtype)
    p.data = np.ascontiguousarray(X, dtype=dtype)
    p.labels = None if labels is None else np.asarray(labels, dtype=dtype)
    return pm.CSVM(p, **kw)


def vectors(m, dtype, count=2, seed=3, signed=False):
    rng = np.random.default_rng(seed + m)
    return [rng.uniform(-1.0 if signed else 1.0, 2.0, m).astype(dtype) for _ in range(count)]


def assert_close(got, want, dtype, what):
    scale = max(np.abs(want).max(), 1e-300)
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    print(f"{what}: max abs error {err:.3e} = {err / scale:.3e} of max|want| {scale:.3e} (bar {KP_TOL[dtype]:.0e})")
    assert err <= KP_TOL[dtype] * scale, (what, err, scale)


# ---- K.p and q against numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", KP_CASES, ids=lambda c: f"{c[0]}x{c[1]}+{c[2]:g}-g{c[3]}" + "".join(f"-{x}" for x in c[4:]))
def test_kp_and_q_against_numpy(case, dtype):
    n, d, offset, gamma = case[:4]
    signed = "signed" in case[4:]
    X, g, K = kp_case(n, d, offset, gamma, dtype)
    m = n - 1
    with make_svm(X, g, dtype) as svm:
        svm.setup_data_on_device()
        q = svm.generate_q()
        info = svm.info()
        assert info["kernel"] == 4 and info["rbf_shift"] == 0 and not info["is_sparse"]
        q_ref, qa_ref = K[:m, m], K[m, m] + 1.0 / COST
        assert_close(q, q_ref, dtype, "q")
        assert abs(float(svm.QA_cost) - qa_ref) <= KP_TOL[dtype] * qa_ref
        p = vectors(m, dtype, 1, signed=signed)[0]
        assert not signed or ((p < 0).any() and (p > 0).any())
        p64 = p.astype(np.float64)
        kp_ref = K[:m, :m] @ p64
        assert_close(svm.kp_part(p, "kernel"), kp_ref, dtype, "kp_part")
        for add in (1.0, -1.0):
            ret = np.zeros(m, dtype=dtype)
            svm.run_device_kernel(None, ret, p, add)
            want = add * (kp_ref + (qa_ref - q_ref) * p64.sum() - q_ref @ p64 + p64 / COST)
            assert_close(ret, want, dtype, f"run_device_kernel add={add:g}")


# ---- the tile cache: implicit, filling and streamed K.p give the same bits in every record form ------------------------
@pytest.mark.parametrize("gamma", [None, 1.0], ids=["g1/d", "g1"])
@pytest.mark.parametrize("dtype,pack", [(np.float32, None), (np.float64, True), (np.float64, "wide"), (np.float64, False)],
                         ids=["f32", "f64-pack", "f64-wide", "f64-raw"])
def test_cache_invariance_bitwise(dtype, pack, gamma):
    n, d = 300, 37
    X, g, _ = kp_case(n, d, 0.0, gamma, dtype)
    m = n - 1
    tiles = 6  # three tile rows
    p1, p2 = vectors(m, dtype)
    with make_svm(X, g, dtype, kp_cache=False) as svm:
        svm.setup_data_on_device()
        want1, want2 = svm.kp_part(p1).copy(), svm.kp_part(p2).copy()
        assert svm.info()["kp_cache_tiles"] == 0
    kw = {} if pack is None else {"kp_pack": pack}
    with make_svm(X, g, dtype, kp_cache=True, **kw) as svm:
        svm.setup_data_on_device()
        fill = svm.kp_part(p1).copy()     # forms the tiles and stores them
        stream1 = svm.kp_part(p1).copy()  # streams them
        stream2 = svm.kp_part(p2).copy()
        info = svm.info()
    assert np.isfinite(want1).all() and np.abs(want1).max() > 0
    assert np.array_equal(fill, want1) and np.array_equal(stream1, want1) and np.array_equal(stream2, want2)
    assert info["kp_cache_tiles"] == tiles, info
    raw = info["kp_cache_tiles"] - info["kp_cache_packed_tiles"]
    print(f"tiles {tiles}: raw {raw}, 7-byte {info['kp_cache_packed_tiles'] - info['kp_cache_narrow_tiles']}, "
          f"narrow {info['kp_cache_narrow_tiles']}")
    assert 0 <= info["kp_cache_narrow_tiles"] <= info["kp_cache_packed_tiles"] <= tiles, info
    if dtype == np.float32 or pack is False:
        assert info["kp_cache_packed_tiles"] == 0, info  # fp32 records and unpacked fp64 records are raw
    elif gamma == 1.0:
        assert raw >= 1, info  # values from 1 on the diagonal down to e^-30: too many binades for a packed record
    else:
        assert info["kp_cache_packed_tiles"] >= 1, info  # values within a few binades of 1
    if pack == "wide":
        assert info["kp_cache_narrow_tiles"] == 0, info


@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_cache_bitwise(dtype, monkeypatch):
    """m = 1100, d = 8: 45 tiles, a budget for 22 raw records and a half (test_gpu_kp_reduce_order.test_partial_cache's).
    Tiles [0, 22) are stored by the filling K.p and streamed afterwards, tiles [22, 45) are formed by a Laplacian
    KP_COMPUTE launch each time (launch_kp_tiles, launch_kp_tiles_multi): the same bits as with no cache at all, which
    is itself within the bar of numpy."""
    n, d, R, want_tiles = 1101, 8, 3, 22
    X, g, K = kp_case(n, d, 0.0, None, dtype)
    m = n - 1
    P = np.stack(vectors(m, dtype, R, seed=29, signed=True))
    q_ref, qa_ref = K[:m, m], K[m, m] + 1.0 / COST

    def run(svm):
        svm.setup_data_on_device()
        svm.generate_q()
        first = svm.run_device_kernel(None, np.zeros(m, dtype=dtype), P[0], 1.0).copy()
        second = svm.run_device_kernel(None, np.zeros(m, dtype=dtype), P[0], 1.0).copy()
        multi = svm.run_device_kernel_multi(None, np.zeros((R, m), dtype=dtype), P, 1.0).copy()
        return first, second, multi, svm.info()

    with make_svm(X, g, dtype, kp_cache=False) as svm:
        want, again, want_multi, info = run(svm)
        assert info["kp_cache_tiles"] == 0
    assert np.array_equal(again, want) and np.array_equal(want_multi[0], want)
    for c in range(R):
        p64 = P[c].astype(np.float64)
        ref = K[:m, :m] @ p64 + (qa_ref - q_ref) * p64.sum() - q_ref @ p64 + p64 / COST
        assert_close(want_multi[c], ref, dtype, f"no cache, vector {c}")
    rec = 128 * 128 * np.dtype(dtype).itemsize
    monkeypatch.setenv("PLSSVM_MI_MEM_BUDGET", str(want_tiles * rec + rec // 2))
    with make_svm(X, g, dtype, kp_cache=True) as svm:
        fill, stream, multi, info = run(svm)
    assert info["kp_cache_tiles"] == want_tiles, info
    assert np.array_equal(fill, want), np.abs(fill - want).max()
    assert np.array_equal(stream, want), np.abs(stream - want).max()
    assert np.array_equal(multi, want_multi), np.abs(multi - want_multi).max()


# ---- batched K.p and one-vs-all training ------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", [True, False], ids=["cached", "implicit"])
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_kp_multi_rows_are_the_single_call(dtype, R, cache):
    n, d = 300, 37
    X, g, _ = kp_case(n, d, 0.0, None, dtype)
    m = n - 1
    P = np.stack(vectors(m, dtype, R, seed=17))
    with make_svm(X, g, dtype, kp_cache=cache) as svm:
        svm.setup_data_on_device()
        svm.generate_q()
        single = np.stack([svm.run_device_kernel(None, np.zeros(m, dtype=dtype), P[c], 1.0) for c in range(R)])
        RET = np.zeros((R, m), dtype=dtype)
        svm.run_device_kernel_multi(None, RET, P, 1.0)
    assert np.abs(single).max() > 0 and np.array_equal(RET, single)


@functools.lru_cache(maxsize=None)
def three_blobs(dtype):
    rng = np.random.default_rng(23)
    centres = rng.uniform(-1.0, 1.0, size=(3, 16))
    cls = rng.permutation(np.arange(300) % 3)
    X = (centres[cls] + 0.15 * rng.standard_normal((300, 16))).astype(dtype)
    X.setflags(write=False)
    return X, cls.astype(np.float64)


@pytest.mark.parametrize("cache", [None, False], ids=["cached", "implicit"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_learn_multi_is_learn_per_class(dtype, cache):
    X, labels = three_blobs(dtype)
    g = rounded_gamma(16, dtype)
    with make_svm(X, g, dtype, labels=labels, kp_cache=cache) as svm:
        svm.learn_multi(imax=30)
        classes, alphas, biases = svm.classes.copy(), svm.alphas.copy(), svm.biases.copy()
        iters, traces = svm.iters_multi.copy(), [t.copy() for t in svm.traces]
    assert list(classes) == [0.0, 1.0, 2.0]
    _, Y = pm.one_vs_all(labels, np.dtype(dtype))
    for c in range(3):
        with make_svm(X, g, dtype, labels=Y[c], kp_cache=cache) as one:
            one.learn(imax=30)
            assert one.iters == iters[c] and one.iters > 0
            assert np.array_equal(one.trace, traces[c])
            assert np.array_equal(one.alpha, alphas[c])
            assert one.bias == biases[c]


# ---- simulated ranks -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sim_case(dtype):
    return kp_case(1200, 16, 0.0, None, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_simulated_rank_shares_sum_to_the_full_kp(dtype):
    X, g, K = sim_case(dtype)
    m = X.shape[0] - 1
    p = vectors(m, dtype, 1)[0]
    p64 = p.astype(np.float64)
    q_ref, qa_ref = K[:m, m], K[m, m] + 1.0 / COST
    want = K[:m, :m] @ p64 + (qa_ref - q_ref) * p64.sum() - q_ref @ p64 + p64 / COST
    total = np.zeros(m)
    local = []
    for r in range(3):
        with make_svm(X, g, dtype, sim_rank=(r, 3)) as svm:
            svm.setup_data_on_device()
            svm.generate_q()
            total += svm.run_device_kernel(None, np.zeros(m, dtype=dtype), p, 1.0).astype(np.float64)
            local.append(svm.info()["tiles_local"])
    # ten tile rows = three super-blocks of 36, 16 and 3 tiles: the split is by whole super-blocks, so one of the three
    # ranks may own none (its share is then zero) while the others own different ones
    assert sum(local) == 10 * 11 // 2 and sorted(local)[1] > 0, local
    assert_close(total, want, dtype, "sum of the shares")


# ---- CG against the numpy restatement on the explicit matrix -------------------------------------------------------------
def numpy_cg(Q, y, eps, imax):
    """cg_trace_cases.trace_extended, returning the iterate too (the same statements: the traces must be equal)."""
    m = Q.shape[0]
    yl = np.asarray(y, dtype=np.longdouble)
    b = yl[:m] - yl[m]
    x = np.ones(m, dtype=np.longdouble)
    r = b - Q @ x
    dv = r.copy()
    delta = r @ r
    d0, tr = delta, [delta]
    for it in range(imax):
        Ad = Q @ dv
        a = delta / (dv @ Ad)
        x += a * dv
        r = b - Q @ x if it % 50 == 49 else r - a * Ad
        dn = r @ r
        tr.append(dn)
        if dn <= np.longdouble(eps) ** 2 * d0:
            break
        dv = dn / delta * dv + r
        delta = dn
    return x, np.array(tr, dtype=np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_learn_against_numpy_cg(dtype):
    """n = 400, d = 16, C = 1 on two well-separated blobs (datagen.blobs, seed 6, cluster_std 2: the long-double model
    separates the training points), learn() against the long-double numpy CG on the explicit matrix.

    From the start vector x = 1 the residual falls by eight orders of magnitude in three iterations (delta / delta0 =
    7.3e-5, 3.9e-8, 1.1e-8, then 9.3e-10, 1.6e-10), and any fp64 CG leaves the long-double iterate quickly on such a
    system: numpy's own float64 CG on the same matrix (explicit, or in the library's implicit form K p + (QA - q_i)
    sum p - q.p + p / C) deviates in alpha by 2e-13 / 5e-11 / 7e-9 of max|alpha| after 2 / 3 / 4 iterations, a
    coherent offset of all elements that the last one, -sum, collects; on datagen's default blobs (seed 11) it is 1e-11 /
    4e-9 / 8e-7, and the library itself measured 2.2e-7 after 4 iterations there (trace within 3e-11). So this system
    gives no "few tens of iterations" at which alpha is comparable at 1e-9. epsilon is set so that the solve ends after
    three iterations, where float64 arithmetic is a factor 17 inside the alpha bar: 1.45e-4 in fp64 (eps^2 = 2.1e-8 lies
    a factor 1.8 under iteration 2 and 1.9 over iteration 3; the trace is good to 2e-13 there, so the count does not
    hang on rounding) and 1e-3 in fp32 (two iterations: the three trace entries the fp32 bar covers).

    On an MI355X, as written: fp64 three iterations, trace within 2.1e-13, alpha within 5.3e-10 of max|alpha|; fp32 two
    iterations, trace within 3.4e-5, alpha within 7.3e-4."""
    n, d = 400, 16
    X, y = datagen.blobs(n, d, seed=6, dtype=dtype, cluster_std=2.0)
    g = rounded_gamma(d, dtype)
    eps = 1.45e-4 if dtype == np.float64 else 1e-3
    m = n - 1
    K = l1_kernel(X, X, g).astype(np.longdouble)
    qa = K[m, m] + np.longdouble(1.0 / COST)
    Q = K[:m, :m] + qa - K[:m, m][:, None] - K[:m, m][None, :] + np.eye(m, dtype=np.longdouble) / np.longdouble(COST)
    trace = cgc.trace_extended(dict(y=y, eps=eps), Q=Q)
    assert 2 <= len(trace) - 1 < cgc.IMAX and trace[-1] <= eps ** 2 * trace[0]  # the numpy CG itself converges
    x, trace2 = numpy_cg(Q, y, eps, cgc.IMAX)
    assert np.array_equal(trace, trace2)
    alpha_ref = np.concatenate([x, [-x.sum()]]).astype(np.float64)
    rho_ref = -float(np.longdouble(y[m]) + qa * x.sum() - K[:m, m] @ x)
    with make_svm(X, g, dtype, labels=y, epsilon=eps) as svm:
        svm.learn(imax=cgc.IMAX)
        got_trace, alpha, rho, iters = svm.trace.copy(), svm.alpha.astype(np.float64), float(svm.rho), svm.iters
    print(f"iterations {iters} (numpy {len(trace) - 1}); trace rel err "
          f"{np.abs(got_trace[:len(trace)] / trace[:len(got_trace)] - 1).max():.3e}; alpha err "
          f"{np.abs(alpha - alpha_ref).max() / np.abs(alpha_ref).max():.3e}; rho {rho:.6g} vs {rho_ref:.6g}")
    assert iters == len(trace) - 1
    if dtype == np.float64:
        np.testing.assert_allclose(got_trace, trace, rtol=1e-6)
        np.testing.assert_allclose(alpha, alpha_ref, rtol=1e-9, atol=1e-9 * np.abs(alpha_ref).max())
        assert abs(rho - rho_ref) <= 1e-9 * max(1.0, abs(rho_ref))
    else:
        np.testing.assert_allclose(got_trace[:3], trace[:3], rtol=1e-3)
        np.testing.assert_allclose(alpha, alpha_ref, rtol=2e-2, atol=2e-2 * np.abs(alpha_ref).max())
        assert abs(rho - rho_ref) <= 2e-2 * max(1.0, abs(rho_ref))


# ---- predict ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def predict_case(n, d, npts, K, dtype):
    """A model (X, A [K][n], b [K]) and points Z on uniform [-1, 1] data; values [K][npts] in float64."""
    rng = np.random.default_rng(n + 7 * d + npts)
    X = rng.uniform(-1.0, 1.0, size=(n, d)).astype(dtype)
    Z = rng.uniform(-1.0, 1.0, size=(npts, d)).astype(dtype)
    A = rng.standard_normal((K, n)).astype(dtype)
    b = rng.standard_normal(K).astype(dtype)
    g = rounded_gamma(d, dtype)
    want = A.astype(np.float64) @ l1_kernel(X, Z, g) + b.astype(np.float64)[:, None]
    for a in (X, Z, A, b, want):
        a.setflags(write=False)
    return X, Z, A, b, g, want


def to_csr(Z):
    rr, cc = np.nonzero(Z)
    rowptr = np.concatenate([[0], np.cumsum((Z != 0).sum(axis=1))]).astype(np.int64)
    return rowptr, cc.astype(np.int32), Z[rr, cc], Z.shape[0], Z.shape[1]


@pytest.mark.parametrize("npts", [1, 130, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_values_against_numpy(dtype, npts, monkeypatch):
    monkeypatch.setenv("PLSSVM_MI_PRED_CHUNK", "128")
    X, Z, A, b, g, want = predict_case(300, 37, npts, 1, dtype)
    with make_svm(X, g, dtype) as svm:
        got = svm.predict_values(Z, alpha=A[0], bias=b[0])
        assert svm.info()["predict_algo"] == 3  # PLSSVM_MI_PREDICT_TILES
    assert_close(got, want[0], dtype, f"predict_values np={npts}")


@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_contract_bitwise(dtype, K, monkeypatch):
    """Row c of the nclass call is the single call with (alpha_c, bias_c); a permuted subset of the points, another
    chunking and CSR points give the same bits; the path is the tile kernel with and without PLSSVM_MI_PRED_GEMM=1."""
    X, Z, A, b, g, want = predict_case(300, 37, 300, K, dtype)
    with make_svm(X, g, dtype) as svm:
        multi = svm.predict_values_multi(Z, alphas=A, biases=b)  # [np][K]
        assert svm.info()["predict_algo"] == 3
        for c in range(K):
            assert_close(multi[:, c], want[c], dtype, f"class {c} of {K}")
        monkeypatch.setenv("PLSSVM_MI_PRED_GEMM", "1")  # no meaning for this kernel: ignored
        single = np.stack([svm.predict_values(Z, alpha=A[c], bias=b[c]) for c in range(K)], axis=1)
        assert svm.info()["predict_algo"] == 3
        monkeypatch.delenv("PLSSVM_MI_PRED_GEMM")
        assert np.array_equal(multi, single)
        pick = np.random.default_rng(5).permutation(300)[:77]
        assert np.array_equal(svm.predict_values_multi(Z[pick], alphas=A, biases=b), multi[pick])
        monkeypatch.setenv("PLSSVM_MI_PRED_CHUNK", "128")
        assert np.array_equal(svm.predict_values_multi(Z, alphas=A, biases=b), multi)
        Zs = np.where(np.random.default_rng(6).random(Z.shape) < 0.5, Z, 0).astype(dtype)  # CSR points with real zeros
        dense = svm.predict_values_multi(Zs, alphas=A, biases=b)
        assert np.array_equal(svm.predict_values_multi(to_csr(Zs), alphas=A, biases=b), dense)
        assert np.array_equal(svm.predict_values(to_csr(Zs), alpha=A[0], bias=b[0]), dense[:, 0])
        assert svm.info()["predict_algo"] == 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_across_a_segment_boundary(dtype):
    """n = 2200: m = 2199 rows are 18 support-vector tiles, one segment of PLSSVM_MI_PREDICT_SEG_TILES = 16 and a second of
    two, so every point's sum crosses a segment boundary."""
    assert _abi.PREDICT_SEG_TILES == 16
    X, Z, A, b, g, want = predict_case(2200, 8, 130, 3, dtype)
    with make_svm(X, g, dtype) as svm:
        multi = svm.predict_values_multi(Z, alphas=A, biases=b)
        single = svm.predict_values(Z, alpha=A[1], bias=b[1])
    for c in range(3):
        assert_close(multi[:, c], want[c], dtype, f"class {c}")
    assert np.array_equal(multi[:, 1], single)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["csr", "coo"])
def test_sparse_setup_is_refused_and_the_context_stays_usable(form):
    dtype = np.float64
    X, g, K = kp_case(130, 5, 0.0, None, dtype)
    m = X.shape[0] - 1
    rowptr, col, val, n, d = to_csr(X)
    L = _abi.lib()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with make_svm(X, g, dtype) as svm:
        if form == "csr":
            rc = L.plssvm_mi_setup_csr(svm._ctx, ptr(rowptr), ptr(col), ptr(val), _abi.VAL_REAL, n, d)
        else:
            row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
            rc = L.plssvm_mi_setup_coo(svm._ctx, ptr(row), ptr(col), ptr(val), _abi.VAL_REAL, val.size, n, d)
        assert rc == -5  # PLSSVM_MI_ERR_UNSUPPORTED
        msg = L.plssvm_mi_last_error(svm._ctx).decode()
        assert "Laplacian kernel takes dense data" in msg, msg
        svm.setup_data_on_device()  # plssvm_mi_setup_dense on the same context
        p = vectors(m, dtype, 1)[0]
        assert_close(svm.kp_part(p), K[:m, :m] @ p, dtype, "kp_part after the refusal")
