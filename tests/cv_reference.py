"""Float64 / same-type numpy statements of held-out training (plssvm_mi_learn_held), shared by
tests/test_cv_cpu.py (which pins them against the bordered direct solve) and tests/test_gpu_cv.py (which uses them as
the reference of the GPU results).

Lane k trains on T = the points not held out. Its pivot t = max T takes the last point's part: R = T without t,
Q~_ij = k_ij + QA - q_i - q_j + delta_ij diag_i on R with q_i = k(x_i, x_t), QA = k_tt + diag_t, b_i = y_i - y_t; the
reference CG from x0 = 1; alpha_t = -sum alpha, bias = y_t + QA sum alpha - q . alpha, alpha = 0 on held-out points."""
import functools

import numpy as np


def kernel_matrix(kernel, X, gamma):
    X = np.asarray(X, dtype=np.float64)
    if kernel == "laplacian":
        D = np.empty((X.shape[0], X.shape[0]))
        for a in range(0, X.shape[0], 64):
            D[a:a + 64] = np.abs(X[a:a + 64, None, :] - X[None, :, :]).sum(-1)
        return np.exp(-gamma * D)
    G = X @ X.T
    if kernel == "linear":
        return G
    nrm = np.diag(G)
    return np.exp(-gamma * np.maximum(nrm[:, None] + nrm[None, :] - 2 * G, 0.0))


@functools.lru_cache(maxsize=None)
def blobs_case(n, d, dtype, kernel, unbalanced=False):
    """Two Gaussian blobs at +-1 per feature, the labels shuffled; gamma = 1/d as float32 rounds it; K in float64 from
    the rounded X. unbalanced: a quarter of the points positive, the blobs closer (0.35 per feature)."""
    rng = np.random.default_rng(0)
    y = np.where(rng.permutation(n) % (4 if unbalanced else 2) == 0, 1.0, -1.0)
    X = (rng.normal(size=(n, d)) + (0.35 if unbalanced else 1.0) * y[:, None]).astype(dtype)
    g = float(np.float32(1.0 / d))
    K = kernel_matrix(kernel, X, g)
    for a in (X, y, K):
        a.setflags(write=False)
    return X, y.astype(dtype), g, K


def hold_patterns(n):
    """The issue's hold rows: (a) i mod 5 == k for k = 0 .. 4, (b) rows 128 .. 255 and a few others, (c) the last 7
    points, (d) nothing."""
    i = np.arange(n)
    rows = {f"a{k}": i % 5 == k for k in range(5)}
    b = (i >= 128) & (i < 256)
    b[[3, 77, 127, 256, n - 2]] = True
    rows["b"] = b
    rows["c"] = i >= n - 7
    rows["d"] = np.zeros(n, dtype=bool)
    return rows


def diagonal(cost, s, n, dtype):
    """(1/C)(1/s_i) as the real type rounds it, in float64 (s None: 1/C)."""
    t = np.dtype(dtype).type
    cinv = t(1) / t(cost)
    if s is None:
        return np.full(n, float(cinv))
    return (cinv * (t(1) / np.asarray(s, dtype=dtype))).astype(np.float64)


def pivot_system(K, y, hold, diag):
    """t, R, Q~ on R, b, q (on R) and QA of a lane, all float64."""
    train = np.flatnonzero(~np.asarray(hold, dtype=bool))
    t = int(train[-1])
    R = train[:-1]
    q = K[R, t]
    QA = K[t, t] + diag[t]
    Q = K[np.ix_(R, R)] + QA - q[:, None] - q[None, :] + np.diag(diag[R])
    b = np.asarray(y, dtype=np.float64)[R] - float(y[t])
    return t, R, Q, b, q, QA


def cg(Q, b, eps, imax):
    """The reference recurrence in Q's dtype from x0 = 1, explicit residual every 50th iteration: x, trace, iterations."""
    t = Q.dtype.type
    x = np.ones(Q.shape[0], dtype=Q.dtype)
    r = b - Q @ x
    dv = r.copy()
    delta = r @ r
    d0 = delta
    trace = [float(delta)]
    it = 0
    while it < imax:
        Ad = Q @ dv
        a = delta / (dv @ Ad)
        x = x + a * dv
        r = b - Q @ x if it % 50 == 49 else r - a * Ad
        dn = r @ r
        it += 1
        trace.append(float(dn))
        if dn <= t(eps) ** 2 * d0:
            break
        dv = dn / delta * dv + r
        delta = dn
    return x, np.array(trace), it


def lane_from_x(n, y, t, R, q, QA, x):
    """alpha [n] and the bias from the solution x on R."""
    x = np.asarray(x, dtype=np.float64)
    alpha = np.zeros(n)
    alpha[R] = x
    alpha[t] = -x.sum()
    return alpha, float(y[t]) + QA * x.sum() - q @ x


def direct_subset(K, y, hold, diag):
    """The bordered system [[K_TT + diag, 1], [1^T, 0]] [alpha; b] = [y_T; 0] on the training points: alpha [n] (0 on
    held-out points) and the bias."""
    T = np.flatnonzero(~np.asarray(hold, dtype=bool))
    k = T.size
    A = np.zeros((k + 1, k + 1))
    A[:k, :k] = K[np.ix_(T, T)] + np.diag(diag[T])
    A[:k, k] = A[k, :k] = 1.0
    z = np.linalg.solve(A, np.concatenate([np.asarray(y, dtype=np.float64)[T], [0.0]]))
    alpha = np.zeros(K.shape[0])
    alpha[T] = z[:k]
    return alpha, z[k]
