"""GPU tests of held-out lanes (plssvm_mi_learn_held), plssvm_mi_train_values, CSVM.cross_validate and plssvm-train -v
(DESIGN.md §3.1.7).

Shapes n x d = 301 x 12 (three tile rows, the last ragged) and 1153 x 20 (ten tile rows, across the 1024-row super-block
boundary). Data, hold patterns and the numpy statements of the arithmetic: tests/cv_reference.py (pinned against the
bordered direct solve by tests/test_cv_cpu.py). C = 4 unless a test says otherwise; imax = 2000 is passed explicitly.

Bars: the K.p bar 1e-12 (fp64) / 1e-4 (fp32) of max|want|; whatever the library promises bitwise is compared with
np.array_equal; the bar of a solved system is derived inside the test from numpy's own run of the recurrence.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import cv_reference as ref
import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi, datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")
DTYPES = [np.float64, np.float32]
KP_TOL = {np.float64: 1e-12, np.float32: 1e-4}
# test 3 solves this far: at 1e-5 the float32 recurrence's own error (1e-2 .. 6e-2 of max|alpha|) times ten would reach
# the distance between a fold's model and the full-data model (0.03 .. 0.5); at 1e-7 it is 1e-4 .. 2e-3
EPS_SOLVE = {np.float64: 1e-10, np.float32: 1e-7}
IMAX = 2000
COST = 4.0
ERR_ARG, ERR_UNSUPPORTED = -1, -5
# (kernel, shape, dtype): rbf and laplacian in both types on both shapes; the pairwise linear tiles in one case, fp64 (in
# fp32 the recurrence's own error on X X^T, 2e-3 .. 4e-3 of max|alpha| at epsilon 1e-7, times ten passes half the 0.049
# that separates the last-seven-held model from the full-data one, so test 3's condition cannot hold there)
CASES = [(k, s, t) for k in ("rbf", "laplacian") for s in ((301, 12), (1153, 20)) for t in DTYPES] + [("linear", (301, 12), np.float64)]
CASE_IDS = [f"{k}-{s[0]}x{s[1]}-{np.dtype(t).name}" for k, s, t in CASES]


def dense_svm(kernel, X, y, gamma, dtype, cost=COST, epsilon=1e-3, **kw):
    p = pm.Parameter(kernel, gamma=gamma, cost=cost, epsilon=epsilon, real_type=dtype)
    p.data = np.ascontiguousarray(X, dtype=dtype)
    p.labels = None if y is None else np.asarray(y, dtype=dtype)
    return pm.CSVM(p, **kw)


def solved(svm):
    return svm.alpha.copy(), svm.bias, int(svm.iters), svm.trace.copy()


def lane(svm, k):
    return svm.alphas[k].copy(), svm.biases[k], int(svm.iters_multi[k]), svm.traces[k].copy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def pattern_rows(n):
    pats = ref.hold_patterns(n)
    names = list(pats)
    return names, np.stack([pats[k] for k in names])


# ---- 1. exact zeros and pivots ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,shape,dtype", CASES, ids=CASE_IDS)
def test_exact_zeros_and_pivots(kernel, shape, dtype):
    n, d = shape
    X, y, g, K = ref.blobs_case(n, d, dtype, kernel)
    names, H = pattern_rows(n)
    with dense_svm(kernel, X, y, g, dtype, epsilon=1e-4) as svm:
        svm.learn_held(H, imax=IMAX)
        alphas, piv, iters = svm.alphas.astype(np.float64), svm.pivots.copy(), svm.iters_multi.copy()
    for k, name in enumerate(names):
        want_t = int(np.flatnonzero(~H[k])[-1])
        assert piv[k] == want_t, (name, piv[k], want_t)
        assert np.all(alphas[k][H[k]] == 0.0), f"{name}: alpha is not exactly 0 on a held-out point"
        assert np.count_nonzero(alphas[k][~H[k]]) == (~H[k]).sum(), f"{name}: a training point has alpha 0"
        assert iters[k] > 0
        # alpha_t = -(the sum of the others), each partial sum rounded once: m roundings of at most eps sum|alpha|
        tol = n * np.finfo(dtype).eps * np.abs(alphas[k]).sum()
        assert abs(alphas[k].sum()) <= tol, (name, alphas[k].sum(), tol)
    # the fold that holds the last point out re-pivots to n - 2
    assert piv[names.index(f"a{(n - 1) % 5}")] == n - 2 and piv[names.index("c")] == n - 8 and piv[names.index("d")] == n - 1


# ---- 2. bitwise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,shape", [("rbf", (301, 12)), ("laplacian", (1153, 20))], ids=["rbf-301x12", "laplacian-1153x20"])
def test_all_zero_hold_rows_are_learn_costs(kernel, shape, dtype):
    n, d = shape
    X, y, g, _ = ref.blobs_case(n, d, dtype, kernel)
    costs = np.array([0.5, 4.0, 30.0])
    eps = 1e-10 if dtype == np.float64 else 1e-6
    with dense_svm(kernel, X, y, g, dtype, epsilon=eps) as svm:
        svm.learn_costs(costs, IMAX)
        want = [lane(svm, k) for k in range(3)]
        svm.learn_held(np.zeros((3, n), dtype=bool), costs=costs, imax=IMAX)
        got = [lane(svm, k) for k in range(3)]
        assert np.array_equal(svm.pivots, [n - 1] * 3)
        # one all-zero row among held ones, and a single lane
        H = np.stack([np.arange(n) % 5 == 0, np.zeros(n, dtype=bool), np.arange(n) % 5 == 1])
        svm.learn_held(H, costs=costs, imax=IMAX)
        mixed = lane(svm, 1)
        svm.learn_held(np.zeros((1, n), dtype=bool), costs=costs[2:], imax=IMAX)
        alone = lane(svm, 0)
        svm.set_cost(costs[1])
        single = solved(svm.learn(IMAX))
    for k in range(3):
        assert want[k][2] > 0
        assert same(got[k], want[k]), f"lane {k}: an all-zero hold row is not learn_costs' lane"
    assert same(mixed, want[1]) and same(alone, want[2]) and same(single, want[1])


@functools.lru_cache(maxsize=None)
def fold_lanes(n):
    costs = np.array([0.5, 4.0, 30.0])
    folds = np.arange(n) % 5
    H = np.concatenate([folds[None, :] == np.arange(5)[:, None]] * 3, axis=0)  # lane = cost * 5 + fold
    return H, np.repeat(costs, 5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,shape", [("rbf", (301, 12)), ("laplacian", (1153, 20))], ids=["rbf-301x12", "laplacian-1153x20"])
def test_lanes_are_the_single_lanes(kernel, shape, dtype, monkeypatch):
    """5 folds x 3 costs = 15 lanes: 12 with the last point as pivot (two groups) and the 3 of the fold that holds the
    last point out (pivot n - 2; their own q). Each against the same lane alone at width 1, with and without stored
    tiles; the 15 differ, so a lane returned in another's place fails."""
    n, d = shape
    X, y, g, _ = ref.blobs_case(n, d, dtype, kernel)
    H, costs = fold_lanes(n)
    eps = 1e-10 if dtype == np.float64 else 1e-6
    with dense_svm(kernel, X, y, g, dtype, epsilon=eps) as svm:
        before = solved(svm.learn(IMAX))
        assert svm.info()["multi_width"] == 8
        svm.learn_held(H, costs=costs, imax=IMAX)
        got = [lane(svm, k) for k in range(15)]
        piv = svm.pivots.copy()
        svm.learn_held(H[::-1], costs=costs[::-1], imax=IMAX)  # another order: other groups, the same lanes
        rev = [lane(svm, k) for k in range(15)][::-1]
        after = solved(svm.learn(IMAX))
    assert np.array_equal(piv, np.where(np.arange(15) % 5 == (n - 1) % 5, n - 2, n - 1))
    for cache in (True, False):
        if not cache:
            monkeypatch.setenv("PLSSVM_MI_KP_CACHE", "0")
        with dense_svm(kernel, X, y, g, dtype, epsilon=eps, multi_width=1) as one:
            for k in range(15):
                one.learn_held(H[k:k + 1], costs=costs[k:k + 1], imax=IMAX)
                assert same(got[k], lane(one, 0)), f"lane {k} (stored tiles: {cache})"
            assert one.info()["multi_width"] == 1 and (one.info()["kp_cache_tiles"] > 0) == cache
            one.learn_held(H[3:9], costs=costs[3:9], imax=IMAX)  # several lanes at width 1: one after another
            for k in range(3, 9):
                assert same(got[k], lane(one, k - 3)), f"lane {k} of a width-1 call"
    for k in range(15):
        assert same(rev[k], got[k]), f"lane {k} changed with the order of the lanes"
        for j in range(k):
            assert not np.array_equal(got[k][0], got[j][0])
    assert same(after, before), "the context's cost, weights or q were not restored"
    print(f"iterations per lane: {[r[2] for r in got]}")


# ---- 3. it solves the subset system ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,shape,dtype", CASES, ids=CASE_IDS)
def test_solves_the_subset_system(kernel, shape, dtype):
    """alpha (all n entries) and the bias of every hold pattern against numpy's direct solve of the bordered system on
    the training points, at epsilon = 1e-10 (fp64) / 1e-7 (fp32).

    The bar per lane is 10x what the reference recurrence leaves when numpy runs it in the same real type on the
    explicit submatrix from x0 = 1, as max error over max|alpha| (the bias on the same scale). Conditions, asserted: the
    bar is at most 0.05 and, where points are held out, at most half the distance between the lane's model and the
    full-data model on the lane's training points — a solve that ignored the mask fails."""
    n, d = shape
    X, y, g, K = ref.blobs_case(n, d, dtype, kernel)
    names, H = pattern_rows(n)
    eps = EPS_SOLVE[dtype]
    diag = ref.diagonal(COST, None, n, dtype)
    y64 = y.astype(np.float64)
    full, _ = ref.direct_subset(K, y64, np.zeros(n, dtype=bool), diag)
    with dense_svm(kernel, X, y, g, dtype, epsilon=eps) as svm:
        svm.learn_held(H, imax=IMAX)
        alphas, biases, iters = svm.alphas.astype(np.float64), svm.biases.astype(np.float64), svm.iters_multi.copy()
    for k, name in enumerate(names):
        a_ref, b_ref = ref.direct_subset(K, y64, H[k], diag)
        scale = np.abs(a_ref).max()

        def errors(alpha, bias):
            return max(np.abs(alpha - a_ref).max(), abs(bias - b_ref)) / scale

        t, R, Q, b, q, QA = ref.pivot_system(K, y64, H[k], diag)
        x, _, _ = ref.cg(Q.astype(dtype), b.astype(dtype), eps, IMAX)
        own = errors(*ref.lane_from_x(n, y64, t, R, q, QA, x))
        bar = 10.0 * own
        err = errors(alphas[k], biases[k])
        sep = np.abs(full[~H[k]] - a_ref[~H[k]]).max() / scale
        print(f"{kernel} {n}x{d} {np.dtype(dtype).name} {name}: {iters[k]} iterations, error {err:.3e} of max|alpha|, numpy's "
              f"own {own:.3e}, bar {bar:.3e}, full-data model {sep:.3f} away")
        assert 0 < bar <= 0.05, (name, own, "the numpy reference itself is outside the cap")
        if H[k].any():
            assert bar <= 0.5 * sep, (name, bar, sep)
        assert err <= bar, (name, err, bar)


# ---- 4. the masked product -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,shape,dtype", CASES, ids=CASE_IDS)
def test_masked_product_first_iterations(kernel, shape, dtype):
    """imax = 0: x is x0 = 1 on the active rows and trace[0] = |b - Q~x0|^2; imax = 1: one step. Against float64 numpy on
    the explicit submatrix, at the K.p bar tol = 1e-12 / 1e-4: x1 within tol max|x1|. The residual's entries are within
    tol max|Q~x0| =: e, so delta0 is within 2 e |r|_1 (+ the rounding of m squares and sums); delta1 = r1 . r1 with
    r1 = r0 - a Q~r0 doubles the relative error of two such products: 4 tol of the larger of delta0, delta1. The same
    step on the full system, read on the lane's rows, is farther than 10 tol away (asserted): ignoring the mask fails."""
    n, d = shape
    X, y, g, K = ref.blobs_case(n, d, dtype, kernel)
    names, H = pattern_rows(n)
    keep = [names.index(k) for k in ("a0", "a2", "b", "c")]
    H = H[keep]
    diag = ref.diagonal(COST, None, n, dtype)
    y64 = y.astype(np.float64)
    tol = KP_TOL[dtype]
    with dense_svm(kernel, X, y, g, dtype, epsilon=0.0) as svm:
        svm.learn_held(H, imax=0)
        x0, tr0, it0 = svm.alphas.astype(np.float64), [t.copy() for t in svm.traces], svm.iters_multi.copy()
        svm.learn_held(H, imax=1)
        x1, tr1, it1 = svm.alphas.astype(np.float64), [t.copy() for t in svm.traces], svm.iters_multi.copy()
    t_full, R_full, Q_full, b_full, _, _ = ref.pivot_system(K, y64, np.zeros(n, dtype=bool), diag)
    for k in range(H.shape[0]):
        t, R, Q, b, q, QA = ref.pivot_system(K, y64, H[k], diag)
        ones = np.ones(R.size)
        r0 = b - Q @ ones
        e = tol * np.abs(Q @ ones).max()
        assert it0[k] == 0 and it1[k] == 1
        assert np.array_equal(x0[k][R], ones) and x0[k][t] == -float(R.size)
        assert np.all(x0[k][H[k]] == 0.0) and np.all(x1[k][H[k]] == 0.0)
        d0 = r0 @ r0
        assert abs(tr0[k][0] - d0) <= 2 * e * np.abs(r0).sum() + 4 * n * np.finfo(dtype).eps * d0, (tr0[k][0], d0)
        assert tr1[k][0] == tr0[k][0]
        xs, trs, _ = ref.cg(Q, b, 0.0, 1)
        err = np.abs(x1[k][R] - xs).max() / np.abs(xs).max()
        # the same step on the full system, read on the lane's rows: what ignoring the mask would give
        xu, _, _ = ref.cg(Q_full, b_full, 0.0, 1)
        pos = np.searchsorted(R_full, R[R < t_full])
        away = np.abs(xu[pos] - xs[: pos.size]).max() / np.abs(xs).max()
        print(f"{kernel} {n}x{d} {np.dtype(dtype).name} lane {k}: x1 within {err:.3e} of max|x1|, unmasked {away:.3e} away; "
              f"delta1 {tr1[k][1]:.6e} against {trs[1]:.6e}")
        assert away > 10 * tol
        assert err <= tol
        assert abs(tr1[k][1] - trs[1]) <= 4 * tol * max(trs[0], trs[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["rbf", "laplacian"])
def test_masked_explicit_residual(kernel, dtype):
    """60 iterations with no stop test on 301 x 12: the 50th recomputes r = b - Q~x through the masked product that adds
    to what is stored. Against the direct solve, at 10x the error of numpy's same 60 iterations in the same type (at
    most 0.05 of max|alpha|, and at most half the distance to the full-data model, both asserted); every lane runs all
    60 and keeps its zeros. (No iterate matches numpy's to the K.p bar after 60 steps in another summation order — the
    first steps are held to that bar in test_masked_product_first_iterations — so this run is judged by where it ends.
    b is 0 on a held row, so there a stored 0 and r + add * 0 are the same number: the zeros of alpha are what this run
    can show of that store.)"""
    n, d = 301, 12
    X, y, g, K = ref.blobs_case(n, d, dtype, kernel)
    names, H = pattern_rows(n)
    diag = ref.diagonal(COST, None, n, dtype)
    y64 = y.astype(np.float64)
    full, _ = ref.direct_subset(K, y64, np.zeros(n, dtype=bool), diag)
    with dense_svm(kernel, X, y, g, dtype, epsilon=0.0) as svm:
        svm.learn_held(H, imax=60)
        alphas, biases, iters = svm.alphas.astype(np.float64), svm.biases.astype(np.float64), svm.iters_multi.copy()
    for k, name in enumerate(names):
        a_ref, b_ref = ref.direct_subset(K, y64, H[k], diag)
        scale = np.abs(a_ref).max()
        t, R, Q, b, q, QA = ref.pivot_system(K, y64, H[k], diag)
        x, _, its = ref.cg(Q.astype(dtype), b.astype(dtype), 0.0, 60)
        a_np, b_np = ref.lane_from_x(n, y64, t, R, q, QA, x)
        own = max(np.abs(a_np - a_ref).max(), abs(b_np - b_ref)) / scale
        err = max(np.abs(alphas[k] - a_ref).max(), abs(biases[k] - b_ref)) / scale
        sep = np.abs(full[~H[k]] - a_ref[~H[k]]).max() / scale
        print(f"{kernel} {np.dtype(dtype).name} {name}: error {err:.3e}, numpy's own {own:.3e}, full-data model {sep:.3f} away")
        assert iters[k] == 60 and its == 60
        assert 0 < 10 * own <= 0.05 and (not H[k].any() or 10 * own <= 0.5 * sep)
        assert err <= 10 * own
        assert np.all(alphas[k][H[k]] == 0.0)


# ---- 5. train_values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,shape,dtype", CASES, ids=CASE_IDS)
def test_train_values(kernel, shape, dtype):
    n, d = shape
    X, y, g, K = ref.blobs_case(n, d, dtype, kernel)
    rng = np.random.default_rng(n + 1)
    A = rng.uniform(-1.0, 2.0, size=(9, n)).astype(dtype)
    A[4, ::5] = 0.0  # a model with held-out points
    bias = rng.uniform(-1.0, 1.0, size=9).astype(dtype)
    tol = KP_TOL[dtype]
    with dense_svm(kernel, X, y, g, dtype) as svm:
        nine = svm.train_values(A, bias)
        three = svm.train_values(A[2:5], bias[2:5])
        one = svm.train_values(A[4], bias[4:5])
        svm.learn(IMAX)
        own = svm.train_values(svm.alpha, np.array([svm.bias]))[:, 0].astype(np.float64)
        pred = svm.predict_values(X).astype(np.float64)
        model = svm.alpha.astype(np.float64), float(svm.bias)
    with dense_svm(kernel, X, y, g, dtype, multi_width=1) as w1:
        seq = w1.train_values(A, bias)
    assert nine.shape == (n, 9) and one.shape == (n, 1)
    want = K @ A.astype(np.float64).T + bias.astype(np.float64)[None, :]
    scale = np.abs(want).max()
    err = np.abs(nine.astype(np.float64) - want).max()
    print(f"{kernel} {n}x{d} {np.dtype(dtype).name}: max abs error {err:.3e} = {err / scale:.3e} of max|want| (bar {tol:.0e}); "
          f"last point {abs(float(nine[n - 1, 0]) - want[n - 1, 0]):.3e}")
    assert err <= tol * scale
    assert np.array_equal(three, nine[:, 2:5]) and np.array_equal(one[:, 0], nine[:, 4]), "a row depends on nclass"
    assert np.array_equal(seq, nine), "a row depends on the width"
    # the learned model on its own training points: train_values against predict_values
    want_own = K @ model[0] + model[1]
    bar = tol * np.abs(want_own).max()
    assert np.abs(own - want_own).max() <= bar
    sure = np.abs(want_own) > bar  # both are within the bar of want_own, so there they have its sign
    assert sure.sum() > n // 2 and np.array_equal(np.sign(own[sure]), np.sign(pred[sure]))


# ---- 6. cross_validate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,shape", [("rbf", (301, 12)), ("laplacian", (1153, 20))], ids=["rbf-301x12", "laplacian-1153x20"])
def test_cross_validate_is_learn_held_and_train_values(kernel, shape, dtype):
    n, d = shape
    X, y, g, _ = ref.blobs_case(n, d, dtype, kernel)
    costs = [0.5, 4.0]
    eps = 1e-10 if dtype == np.float64 else 1e-6
    with dense_svm(kernel, X, y, g, dtype, epsilon=eps, cost=2.0) as svm:
        svm.learn_costs([1.0, 3.0], IMAX)
        multi = [lane(svm, k) for k in range(2)]
        before = solved(svm.learn(IMAX))
        acc, held, folds = svm.cross_validate(5, costs, imax=IMAX)
        assert np.array_equal(svm.alpha, before[0]) and svm.bias == before[1], "the model was replaced"
        assert all(same(lane(svm, k), multi[k]) for k in range(2)), "the multi-lane model was replaced"
        after = solved(svm.learn(IMAX))
        assert np.array_equal(folds, pm.stratified_folds(y, 5))
        H = np.concatenate([folds[None, :] == np.arange(5)[:, None]] * 2, axis=0)
        svm.learn_held(H, costs=np.repeat(costs, 5), imax=IMAX)
        vals = svm.train_values()
        mine = np.arange(n) % 7
        acc7, held7, folds7 = svm.cross_validate(7, None, folds=mine, imax=IMAX)
    assert same(after, before), "cross_validate changed the context's cost, weights or q"
    assert held.shape == (2, n) and acc.shape == (2,)
    for c in range(2):
        hand = vals[np.arange(n), c * 5 + folds]
        assert np.array_equal(held[c], hand), "held-out values are not learn_held's and train_values'"
        assert acc[c] == np.mean(np.where(hand > 0, 1, -1) == np.where(y > 0, 1, -1))
    assert np.array_equal(folds7, mine) and held7.shape == (1, n) and 0.5 < acc7[0] <= 1.0


@pytest.mark.parametrize("kernel,shape", [("rbf", (301, 12)), ("laplacian", (1153, 20))], ids=["rbf-301x12", "laplacian-1153x20"])
def test_cross_validate_accuracy_is_the_direct_solves(kernel, shape):
    """fp64, epsilon 1e-10: every held-out decision value against K alpha + b of numpy's direct subset solve. The bar on
    a value is 10x the recurrence's own alpha error (test 3: at most 4e-6 of max|alpha| here) times sum_j |k_ij| max|alpha|,
    taken at its largest, 1e-4 n max|K| max|alpha|; the case's smallest |decision value| is at least 10x that (asserted),
    so every sign, and the accuracy, must agree."""
    n, d = shape
    dtype = np.float64
    X, y, g, K = ref.blobs_case(n, d, dtype, kernel)
    costs = [0.5, 4.0]
    y64 = y.astype(np.float64)
    with dense_svm(kernel, X, y, g, dtype, epsilon=1e-10) as svm:
        acc, held, folds = svm.cross_validate(5, costs, imax=IMAX)
    for c, cost in enumerate(costs):
        diag = ref.diagonal(cost, None, n, dtype)
        want = np.empty(n)
        amax = 0.0
        for f in range(5):
            a, b = ref.direct_subset(K, y64, folds == f, diag)
            want[folds == f] = (K @ a + b)[folds == f]
            amax = max(amax, np.abs(a).max())
        bar = 10 * 4e-6 * amax * np.abs(K).sum(axis=1).max()
        margin = np.abs(want).min()
        err = np.abs(held[c] - want).max()
        print(f"{kernel} C={cost:g}: accuracy {acc[c]:.4f}, values within {err:.3e}, bar {bar:.3e}, smallest |value| {margin:.3e}")
        assert margin >= 10 * bar, (margin, bar)
        assert err <= bar
        assert acc[c] == np.mean(np.where(want > 0, 1, -1) == y64)


def test_cross_validate_takes_class_weight_and_point_weights():
    n, d = 301, 12
    dtype = np.float64
    X, y, g, K = ref.blobs_case(n, d, dtype, "rbf", True)
    y64 = y.astype(np.float64)
    s = np.where(y64 > 0, 3.0, 1.0)
    p = pm.Parameter("rbf", gamma=g, cost=COST, epsilon=1e-10, class_weight={1: 3.0})
    p.data, p.labels = np.array(X), np.array(y)
    with pm.CSVM(p) as svm:
        acc_cw, held_cw, folds = svm.cross_validate(5, imax=IMAX)
    with dense_svm("rbf", X, y, g, dtype, epsilon=1e-10) as svm:
        acc_plain, held_plain, _ = svm.cross_validate(5, imax=IMAX)
        svm.set_point_weights(s)
        acc_pw, held_pw, _ = svm.cross_validate(5, imax=IMAX)
    assert np.array_equal(held_cw, held_pw) and acc_cw[0] == acc_pw[0]
    assert not np.array_equal(held_cw, held_plain)
    diag = ref.diagonal(COST, s, n, dtype)
    want = np.empty(n)
    for f in range(5):
        a, b = ref.direct_subset(K, y64, folds == f, diag)
        want[folds == f] = (K @ a + b)[folds == f]
    assert np.abs(held_cw[0] - want).max() <= 1e-4 * np.abs(want).max()


# ---- 7. refusals leave the context usable ----------------------------------------------------------------------------
def raw_learn_held(svm, Y, H, ldh, nlane=None):
    n = svm.num_data_points
    K = H.shape[0] if nlane is None else nlane
    al, bi, it = np.zeros((K, n), dtype=svm.dtype), np.zeros(K), np.zeros(K, dtype=np.int64)
    return _abi.lib().plssvm_mi_learn_held(svm._ctx, pm._ptr(Y), K, n, None, None, 0, pm._ptr(H), ldh, 30, 1e-3,
                                           pm._ptr(al), pm._ptr(bi), None, pm._ptr(it), None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["csr-stored", "factored-linear", "one-reduction", "sim-rank"])
def test_unsupported_setups_refuse_and_stay_usable(which, dtype):
    n, d = 301, 12
    X, y, g, _ = ref.blobs_case(n, d, dtype, "rbf")
    if which == "csr-stored":
        csr, yc = datagen.sparse_csr(300, 500, 10, seed=800, dtype=dtype)
        p = pm.Parameter("rbf", gamma=1.0 / 500, real_type=dtype, cost=COST)
        p.csr = (csr[0], csr[1], csr[2].astype(dtype), csr[3], csr[4])
        p.labels = np.asarray(yc, dtype=dtype)
        make = lambda: pm.CSVM(p)  # noqa: E731
    elif which == "factored-linear":
        make = lambda: dense_svm("linear", X, y, g, dtype, kp_mode="factored")  # noqa: E731
    elif which == "one-reduction":
        make = lambda: dense_svm("rbf", X, y, g, dtype, cg_variant="one_reduction")  # noqa: E731
    else:
        make = lambda: dense_svm("rbf", X, y, g, dtype, sim_rank=(0, 2))  # noqa: E731
    with make() as svm:
        nn = svm.num_data_points
        before = solved(svm.learn(30))
        H = np.zeros((2, nn), dtype=bool)
        H[0, ::5] = True
        with pytest.raises(pm.BackendError) as e:
            svm.learn_held(H, imax=30)
        assert e.value.code == ERR_UNSUPPORTED and "held-out lanes" in str(e.value)
        print(f"{which}: {e.value}")
        with pytest.raises(pm.BackendError):
            svm.cross_validate(5, imax=30)
        assert same(solved(svm.learn(30)), before), "a refused call changed the context"
        # HOLD = NULL is learn_lanes, which every setup serves; train_values too
        Y = np.ascontiguousarray(np.tile(np.asarray(svm.params.labels, dtype=dtype), (2, 1)))
        al, bi, it, pv = np.zeros((2, nn), dtype=dtype), np.zeros(2), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
        assert _abi.lib().plssvm_mi_learn_held(svm._ctx, pm._ptr(Y), 2, nn, None, None, 0, None, 0, 30, 1e-3, pm._ptr(al),
                                               pm._ptr(bi), None, pm._ptr(it), pm._ptr(pv)) == _abi.OK
        assert np.array_equal(al[0], before[0]) and np.array_equal(pv, [nn - 1] * 2)
        if which == "sim-rank":  # a simulated rank's K.p is its share only: refused, not returned in part
            with pytest.raises(pm.BackendError) as e:
                svm.train_values(before[0], np.array([before[1]]))
            assert e.value.code == ERR_UNSUPPORTED and "train_values" in str(e.value)
            assert same(solved(svm.learn(30)), before)
        else:
            tv = svm.train_values(before[0], np.array([before[1]]))[:, 0].astype(np.float64)
            pr = svm.predict_values(svm.params.data if svm.params.data is not None else svm.params.csr).astype(np.float64)
            assert np.abs(tv - pr).max() <= 10 * KP_TOL[dtype] * max(np.abs(pr).max(), np.abs(before[0]).sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_leave_the_context_usable(dtype):
    n, d = 301, 12
    X, y, g, _ = ref.blobs_case(n, d, dtype, "rbf")
    with dense_svm("rbf", X, y, g, dtype) as svm:
        before = solved(svm.learn(IMAX))
        Y = np.ascontiguousarray(np.tile(y, (2, 1)))
        H = np.zeros((2, n), dtype=np.uint8)
        H[0, ::5] = 1
        assert raw_learn_held(svm, Y, H, n) == _abi.OK
        assert raw_learn_held(svm, Y, H, 0) == _abi.OK  # one row for both lanes
        assert raw_learn_held(svm, Y, H, n - 1) == ERR_ARG
        assert raw_learn_held(svm, Y, H, 1) == ERR_ARG
        assert raw_learn_held(svm, Y, H, n, nlane=0) == ERR_ARG
        one = H.copy()
        one[1, :] = 1
        one[1, 17] = 0  # a single training point
        assert raw_learn_held(svm, Y, one, n) == ERR_ARG
        assert "fewer than two" in _abi.lib().plssvm_mi_last_error(svm._ctx).decode()
        one[1, :] = 1
        assert raw_learn_held(svm, Y, one, n) == ERR_ARG
        one[1, :] = 1
        one[1, [5, n - 1]] = 0  # two are enough
        assert raw_learn_held(svm, Y, one, n) == _abi.OK
        assert same(solved(svm.learn(IMAX)), before)


@pytest.mark.parametrize("multi_width", [None, 1], ids=["auto", "width1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_lane_call_leaves_the_context_as_found(dtype, multi_width):
    """One context with point weights and a cost of its own: after every kind of multi-lane call — classes, a cost grid,
    per-lane weights, held lanes with a moved pivot, held lanes with nothing held, and calls refused with ERR_ARG in their
    last lane — first solver_CG with q = None, which solves with the q and QA_cost it finds in place, and then learn(),
    which forms q and QA_cost anew from the cost and the weights, return the bits they returned before: q, QA_cost, the
    cost, the weights and the hold rows are back. Batched and one lane at a time; the width that ran is asserted."""
    n, d = 301, 12
    X, y, g, _ = ref.blobs_case(n, d, dtype, "rbf")
    rng = np.random.default_rng(301)
    s = rng.uniform(0.5, 2.0, n).astype(dtype)
    S2 = rng.uniform(0.5, 2.0, (2, n)).astype(dtype)
    Y2 = np.ascontiguousarray(np.tile(np.asarray(y, dtype=dtype), (2, 1)))
    last = np.zeros((2, n), dtype=bool)
    last[:, n - 1] = True  # the pivot moves to n - 2
    one_left = np.zeros((2, n), dtype=bool)
    one_left[1, :] = True
    one_left[1, 17] = False
    S_bad = S2.copy()
    S_bad[1, 5] = 0.0
    eps = 1e-10 if dtype == np.float64 else 1e-6

    def refused(call):
        with pytest.raises(pm.BackendError) as e:
            call()
        assert e.value.code == ERR_ARG

    with dense_svm("rbf", X, y, g, dtype, epsilon=eps, multi_width=multi_width) as svm:
        svm.set_point_weights(s)
        before = solved(svm.learn(IMAX))
        assert before[2] > 0 and svm.info()["multi_width"] == (8 if multi_width is None else 1)
        b = (np.asarray(y, dtype=dtype)[: n - 1] - dtype(y[n - 1])).astype(dtype)

        def in_place():  # a solve on the q and QA_cost in place
            x = svm.solver_CG(b, IMAX, eps)
            return x.copy(), int(svm.iters), svm.trace.copy()

        found = in_place()
        assert found[1] > 0
        calls = {
            "learn_multi": lambda: svm.learn_multi(np.arange(n) % 3, IMAX),
            "learn_costs": lambda: svm.learn_costs([0.5, 30.0], IMAX),
            "per-lane weights": lambda: svm._learn_lanes(Y2, None, S2, IMAX),
            "held, moved pivot, per-lane weights": lambda: svm.learn_held(last, S=S2, imax=IMAX),
            "held, nothing held, per-lane weights": lambda: svm.learn_held(np.zeros((2, n), dtype=bool), S=S2, imax=IMAX),
            "a cost of -1": lambda: refused(lambda: svm._learn_lanes(Y2, np.array([0.5, -1.0]), None, IMAX)),
            "a weight of 0": lambda: refused(lambda: svm._learn_lanes(Y2, None, S_bad, IMAX)),
            "one training point": lambda: refused(lambda: svm.learn_held(one_left, S=S2, imax=IMAX)),
        }
        for name, call in calls.items():
            call()
            if not name.startswith(("a ", "one ")):
                assert svm.iters_multi.min() > 0, name
            if name.startswith("held, moved"):
                assert np.array_equal(svm.pivots, [n - 2] * 2)
            now = in_place()
            assert np.array_equal(now[0], found[0]) and now[1] == found[1] and np.array_equal(now[2], found[2]), \
                f"{name}: q or QA_cost in place are not as they were found"
            assert same(solved(svm.learn(IMAX)), before), f"{name}: the context is not as it was found"
        assert svm.info()["multi_width"] == (8 if multi_width is None else 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_densified_csr_takes_held_lanes(dtype):
    """A CSR context forced to the densified path against the dense context on the same matrix (300 x 500, 10 entries per
    row), three lanes, the second of which holds the last point out.

    One masked CG step (imax = 1): each context's x1 within the K.p bar of float64 numpy's step on the explicit submatrix
    (test 4's bar), and the two contexts within the K.p bar of each other. The full solve at epsilon 1e-10 / 1e-7: alpha
    and bias of both contexts against numpy's direct subset solve at test 3's bar — 10x what numpy's own run of the
    recurrence in the same type leaves, at most 0.05 and at most half the distance to the full-data model (asserted)."""
    csr, yc = datagen.sparse_csr(300, 500, 10, seed=800, dtype=dtype)
    rowptr, col, val, n, d = csr
    Xd = np.zeros((n, d), dtype=dtype)
    for i in range(n):
        Xd[i, col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]].astype(dtype)
    yc = np.asarray(yc, dtype=dtype)
    y64 = yc.astype(np.float64)
    g = float(np.float32(1.0 / d))
    K = ref.kernel_matrix("rbf", Xd, g)
    diag = ref.diagonal(COST, None, n, dtype)
    H = np.stack([np.arange(n) % 5 == 0, np.arange(n) % 5 == 4, np.arange(n) >= n - 7])  # the second holds the last point
    eps, tol = EPS_SOLVE[dtype], KP_TOL[dtype]

    def run(svm):
        svm.learn_held(H, imax=1)
        x1, piv = svm.alphas.astype(np.float64), svm.pivots.copy()
        svm.learn_held(H, imax=IMAX)
        return x1, piv, svm.alphas.astype(np.float64), svm.biases.astype(np.float64)

    p = pm.Parameter("rbf", gamma=g, real_type=dtype, cost=COST, epsilon=eps)
    p.csr = (rowptr, col, val.astype(dtype), n, d)
    p.labels = yc
    with pm.CSVM(p, sparse_algo="dense") as svm:
        svm.setup_data_on_device()
        assert svm.info()["sparse_algo"] == _abi.SPARSE_DENSE
        xs, ps, als, bis = run(svm)
    with dense_svm("rbf", Xd, yc, g, dtype, epsilon=eps) as svm:
        xd, pd, ald, bid = run(svm)
    assert np.array_equal(ps, pd) and np.array_equal(ps, [n - 1, n - 2, n - 8])
    full, _ = ref.direct_subset(K, y64, np.zeros(n, dtype=bool), diag)
    for k in range(3):
        t, R, Q, b, q, QA = ref.pivot_system(K, y64, H[k], diag)
        step, _, _ = ref.cg(Q, b, 0.0, 1)
        scale1 = np.abs(step).max()
        e_s, e_d = np.abs(xs[k][R] - step).max() / scale1, np.abs(xd[k][R] - step).max() / scale1
        e_sd = np.abs(xs[k][R] - xd[k][R]).max() / scale1
        assert np.all(xs[k][H[k]] == 0.0) and np.all(als[k][H[k]] == 0.0)
        a_ref, b_ref = ref.direct_subset(K, y64, H[k], diag)
        scale = np.abs(a_ref).max()
        x, _, _ = ref.cg(Q.astype(dtype), b.astype(dtype), eps, IMAX)
        a_np, b_np = ref.lane_from_x(n, y64, t, R, q, QA, x)
        own = max(np.abs(a_np - a_ref).max(), abs(b_np - b_ref)) / scale
        sep = np.abs(full[~H[k]] - a_ref[~H[k]]).max() / scale
        err_s = max(np.abs(als[k] - a_ref).max(), abs(bis[k] - b_ref)) / scale
        err_d = max(np.abs(ald[k] - a_ref).max(), abs(bid[k] - b_ref)) / scale
        print(f"lane {k}: one step within {e_s:.3e} (densified) / {e_d:.3e} (dense) of numpy, {e_sd:.3e} of each other (bar "
              f"{tol:.0e}); solve error {err_s:.3e} / {err_d:.3e} of max|alpha|, numpy's own {own:.3e}, full-data model {sep:.3f} away")
        assert e_s <= tol and e_d <= tol and e_sd <= tol
        assert 0 < 10 * own <= 0.05 and 10 * own <= 0.5 * sep
        assert err_s <= 10 * own and err_d <= 10 * own


# ---- 8. the command line ---------------------------------------------------------------------------------------------
def write_libsvm(path, X, labels):
    with open(path, "w") as f:
        for row, lab in zip(X, labels):
            f.write(f"{lab:g} " + " ".join(f"{k}:{v!r}" for k, v in enumerate(row.tolist())) + "\n")


def run_train(args):
    r = subprocess.run([TRAIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def test_cli_cross_validation(tmp_path):
    n, d = 301, 12
    X, y, g, _ = ref.blobs_case(n, d, np.float64, "rbf", True)
    f = tmp_path / "cv.libsvm"
    write_libsvm(f, X, y)
    common = ["-t", "2", "-g", repr(g), "-c", "4", "-e", "1e-10", "--max_iter", IMAX]
    p = pm.Parameter("rbf", gamma=g, cost=4.0, epsilon=1e-10)
    p.data, p.labels = np.array(X), np.array(y)
    with pm.CSVM(p) as svm:
        acc, _, _ = svm.cross_validate(5, imax=IMAX)
        grid, _, _ = svm.cross_validate(5, [0.25, 4.0, 64.0], imax=IMAX)
    # weight 5 on the positives: numpy's direct subset solves give 88.37% against 89.04% unweighted, every held-out
    # |value| above 9e-3 (weight 3 happens to leave the accuracy where it is)
    pw = pm.Parameter("rbf", gamma=g, cost=4.0, epsilon=1e-10, class_weight={1: 5.0})
    pw.data, pw.labels = np.array(X), np.array(y)
    with pm.CSVM(pw) as svm:
        acc_w, _, _ = svm.cross_validate(5, imax=IMAX)
    code, out, err = run_train(common + ["-v", "5", f])
    assert code == 0, err
    assert f"Cross Validation Accuracy = {100 * acc[0]:g}%" in out.splitlines(), out
    assert not os.path.exists(str(f) + ".model") and os.listdir(tmp_path) == ["cv.libsvm"]
    code, out, err = run_train(common + ["-v", "5", "--cv_costs", "0.25,4,64", f])
    assert code == 0, err
    lines = [l for l in out.splitlines() if l.startswith("C = ")]
    assert lines == [f"C = {c:g}: Cross Validation Accuracy = {100 * a:g}%" for c, a in zip([0.25, 4.0, 64.0], grid)], out
    best = [0.25, 4.0, 64.0][int(np.argmax(grid))]  # argmax: the first, the smaller cost, on a tie
    assert f"Best C = {best:g}" in out.splitlines()[-1]
    code, out, err = run_train(common + ["-v", "5", "--class_weights", "1:5", f])
    assert code == 0, err
    assert f"Cross Validation Accuracy = {100 * acc_w[0]:g}%" in out.splitlines(), out
    assert acc_w[0] != acc[0], "the case must be one whose accuracy the weights change"
    assert os.listdir(tmp_path) == ["cv.libsvm"]
    code, out, err = run_train(common + ["-v", n + 1, f])
    assert code == 1 and "points" in err and os.listdir(tmp_path) == ["cv.libsvm"]
