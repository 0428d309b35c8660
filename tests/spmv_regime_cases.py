"""Shapes, data and references of the factored sparse-linear regime tests (test_spmv_regimes_cpu.py on the CPU,
test_gpu_spmv_regimes.py on the GPU). No GPU is touched here.

The plan builders of csrc/spmv.hpp switch regime on sizes: the panel plan of a pass (build_spmv_plan: LDS panels of
the gathered vector with 16-bit indices, P of them, or one panel of 32-bit global indices; the panel reduction is
split at P >= 16) and the row-block plan of the one-GPU CG (build_rowblock_plan: P panels per workgroup, RBK rows per
workgroup, more than 1024 rows = a second round of the finalize loop). panel_rule / rowblock_rule restate them;
TABLE is the regime every case was built for, and both tests hold the data to it.

Cases (n counts the last point, m = n - 1 rows of Q~; the last point is an empty row, so q = 0 and QA_cost = 1 / C):

    case         n, d, entries per row   CSC pass w = X^T p     CSR pass raw = X w      row blocks of the CG
    wide         3001, 45001, 40         P = 1                  P = 3 / 2 (fp64 / 32)   P = 3 / 2, RBK 64, 47 blocks
    wide_ragged  as wide, rows changed   as wide                as wide                 as wide
    tall         70001, 300, 8           P = 4 / 2 (unsplit)    P = 1                   P = 1, RBK 320
    tall_split   720897, 200, 3          P = 36 / 18 (split)    P = 1                   P = 1, RBK 2048 (the cap), 352
                                                                                        blocks / RBK 2816, 256 blocks
    global       4001, 100000, 6         global indices         global indices          P = 6 / 3 on LDS panels

Data: values U(-1, 1); row 0 of wide and global also holds a value in the columns W - 1, W, 2 W - 1, 2 W of every panel
width (EDGE_WIDTHS: the panel plan's and the row-block plan's, both types) and in column d - 1. wide_ragged: every
97th row empty (row 0 among them), row 5 with 5000 entries over every panel, rows = 1 (mod 3) with all their entries
in the last panel (columns from 40960, the last panel of all four widths), the others 39 and 41 entries in turn, one
column (EMPTY_COLUMN) empty. global: every 97th row after row 0 is empty as well, which keeps the entry count below
3 (m + 1) 2 = 24006, the float CSR pass's threshold for LDS panels, with room for row 0's edge columns. tall_split:
row 2 i + 1 = - row 2 i (column sums exactly zero), values times 2^-5.

References, np.longdouble from the values already rounded to the context's type (FP22: packed and decoded):
kp_reference (Q~ p = X (X^T p) + QA sum(p) + p / C through scipy.sparse), kp_scale (the term-wise S of
test_gpu_sparse_envelope; with more than SCALE_EXACT_ROWS rows the m x m matrix |k_ij| cannot be formed and the
off-diagonal |k_ij| |p_j| terms are left out of S: a smaller S, so a bound that is no looser) and cg (a plain CG from
x = 1 as cg_begin / cg_step run it, in any dtype, with an optional altered product for the CPU test's teeth).
numpy_cg_errors runs that CG in the context's type over CG_ORDERS summation orders; the GPU's CG bounds are 10 x its
largest error (NUMPY_CG_ERR, NUMPY_TRACE_ERR).
"""
import functools

import numpy as np

LD = np.longdouble
DTYPES = {"f64": np.float64, "f32": np.float32}
KP_TOL = {"f64": 1e-12, "f32": 1e-4}  # the project's K.p contract, of S (test_gpu_kernel_envelope.KP_TOL)

LDS_BYTES = 163840  # SELL_XBYTES: the LDS panel of a pass
RB_ACC_BYTES = 16384  # the row-block pass's row accumulator
TARGET_BLOCKS = 256  # sell_target_blocks()
RED_BLOCKS = 512  # the row-block plan refuses above this many workgroups
SPLIT_PANELS = 16  # panel_reduce_kernel splits its panel loop from here
FIN_ROWS_PER_ROUND = 1024  # rows the fused finalize covers per round of its loop (one per thread)
SCALE_EXACT_ROWS = 5000


# ---- the plan rules of csrc/spmv.hpp, restated ----------------------------------------------------------------------
def panel_width(size):
    return LDS_BYTES // size


def rowblock_width(size):
    return (LDS_BYTES - RB_ACC_BYTES) // size // 1024 * 1024


def panel_rule(nseg, xn, nnz, size):
    """build_spmv_plan: a pass over nseg segments gathering a vector of xn elements, nnz entries."""
    W = panel_width(size)
    P_lds = max(1, -(-max(xn, 1) // W))
    ldsx = P_lds * (nseg + 1) * 2 <= max(nnz, 1)
    P = P_lds if ldsx else 1
    return dict(P=P, ldsx=int(ldsx), W=W if ldsx else max(xn, 1), nchunks=P * -(-nseg // 64))


def rowblock_rule(m, d, size):
    """build_rowblock_plan: m rows gathering a vector of d elements."""
    W = rowblock_width(size)
    cap = RB_ACC_BYTES // size
    RBK = min(cap, -(-(-(-m // TARGET_BLOCKS)) // 64) * 64)
    nblk = -(-m // RBK)
    if nblk > RED_BLOCKS:
        return dict(P=0, W=0, RBK=0, nblk=0)
    return dict(P=max(1, -(-max(d, 1) // W)), W=W, RBK=RBK, nblk=nblk)


def plan_rule(m, d, nnz, dt, fp22=False, rows=None, single=True):
    """What CSVM.spmv_plan() must report (nblocks aside: at least 1, at most min(TARGET_BLOCKS, nchunks)). rows: the
    (r0, r1) of a simulated rank's CSR pass with its entry count nnz_rows = rows[2]; single: one GPU (row blocks)."""
    size = np.dtype(DTYPES[dt]).itemsize
    csc = panel_rule(d, m, nnz, size)
    csr = panel_rule(m, d, nnz, size) if rows is None else panel_rule(rows[1] - rows[0], d, rows[2], size)
    for p in (csc, csr):
        p["f22"] = int(fp22)
    rb = rowblock_rule(m, d, size) if single else dict(P=0, W=0, RBK=0, nblk=0)
    return dict(csc=csc, csr=csr, rb=rb)


def plan_matches(got, want):
    """The reported plan against the rule; returns the list of differences."""
    bad = []
    for side in ("csc", "csr"):
        for k, v in want[side].items():
            if got[side][k] != v:
                bad.append((side, k, got[side][k], v))
        if not 1 <= got[side]["nblocks"] <= min(TARGET_BLOCKS, want[side]["nchunks"]):
            bad.append((side, "nblocks", got[side]["nblocks"]))
    if got["rb"] != want["rb"]:
        bad.append(("rb", got["rb"], want["rb"]))
    return bad


# (P, ldsx) of the CSC and the CSR pass, (P, RBK, nblk) of the row blocks; fp64 / fp32
TABLE = {
    "wide": {"f64": dict(csc=(1, 1), csr=(3, 1), rb=(3, 64, 47)), "f32": dict(csc=(1, 1), csr=(2, 1), rb=(2, 64, 47))},
    "tall": {"f64": dict(csc=(4, 1), csr=(1, 1), rb=(1, 320, 219)), "f32": dict(csc=(2, 1), csr=(1, 1), rb=(1, 320, 219))},
    "tall_split": {"f64": dict(csc=(36, 1), csr=(1, 1), rb=(1, 2048, 352)),
                   "f32": dict(csc=(18, 1), csr=(1, 1), rb=(1, 2816, 256))},
    "global": {"f64": dict(csc=(1, 0), csr=(1, 0), rb=(6, 64, 63)), "f32": dict(csc=(1, 0), csr=(1, 0), rb=(3, 64, 63))},
}
TABLE["wide_ragged"] = TABLE["wide"]
SHAPES = {"wide": (3001, 45001, 40), "wide_ragged": (3001, 45001, 40), "tall": (70001, 300, 8),
          "tall_split": (720897, 200, 3), "global": (4001, 100000, 6)}
COST = {"wide": 3000.0, "wide_ragged": 3000.0, "global": 3000.0, "tall": 1.0, "tall_split": 1024.0}
EDGE_WIDTHS = tuple(sorted({f(s) for f in (panel_width, rowblock_width) for s in (8, 4)}))  # 18432, 20480, 36864, 40960
EMPTY_COLUMN = 12345
LAST_PANEL_FROM = 40960  # wide: columns from here lie in the last panel of every plan and type
FP22_CASES = ("wide", "tall", "global")


def edge_columns(d):
    cols = {d - 1}
    for W in EDGE_WIDTHS:
        cols.update(c for c in (W - 1, W, 2 * W - 1, 2 * W) if c < d)
    return sorted(cols)


# ---- data ------------------------------------------------------------------------------------------------------------
def _draw_rows(rng, counts, lo, hi, banned=()):
    """Sorted distinct columns in [lo_i, hi) per row, counts[i] of them; a banned column is redrawn."""
    out = []
    for k, a in zip(counts, lo):
        if k == 0:
            out.append(np.zeros(0, np.int64))
            continue
        while True:
            c = np.unique(rng.integers(a, hi, size=2 * int(k) + 8))
            c = c[~np.isin(c, banned)]
            if c.size >= k:
                break
        out.append(np.sort(rng.choice(c, size=int(k), replace=False)))
    return out


@functools.lru_cache(maxsize=None)
def master(case):
    """(rowptr, col, val float64, n, d) before the rounding to the context's type; the last row is empty."""
    n, d, k = SHAPES[case]
    m = n - 1
    rng = np.random.default_rng({"wide": 31, "wide_ragged": 32, "tall": 33, "tall_split": 34, "global": 35}[case])
    if case in ("tall", "tall_split"):
        half = m // 2 if case == "tall_split" else m
        c = np.sort(rng.integers(0, d, size=(half, k)), axis=1)
        while True:  # redraw the rows with a repeated column
            dup = np.nonzero((np.diff(c, axis=1) == 0).any(axis=1))[0]
            if dup.size == 0:
                break
            c[dup] = np.sort(rng.integers(0, d, size=(dup.size, k)), axis=1)
        v = rng.uniform(-1.0, 1.0, (half, k))
        if case == "tall_split":  # row 2 i + 1 = - row 2 i, everything times 2^-5
            assert m % 2 == 0
            c = np.repeat(c, 2, axis=0)
            v = np.repeat(v, 2, axis=0) * 2.0 ** -5
            v[1::2] *= -1.0
        rowptr = np.concatenate([np.arange(0, m * k + 1, k), [m * k]]).astype(np.int64)
        return rowptr, c.reshape(-1).astype(np.int32), v.reshape(-1), n, d
    counts = np.full(m, k)
    lo = np.zeros(m, np.int64)
    banned = ()
    if case == "wide_ragged":
        counts = np.where(np.arange(m) % 2 == 0, k - 1, k + 1)
        lo[1::3] = LAST_PANEL_FROM
        counts[1::3] = k
        counts[::97] = 0
        banned = (EMPTY_COLUMN,)
    elif case == "global":
        counts[97::97] = 0
    rows = _draw_rows(rng, counts, lo, d, banned)
    if case in ("wide", "global"):
        rows[0] = np.union1d(rows[0], edge_columns(d))
    if case == "wide_ragged":  # row 5: 5000 entries, evenly over the whole width
        rows[5] = np.setdiff1d(np.unique(np.linspace(0, d - 1, 5003).astype(np.int64)), banned)[:5000]
    lens = np.array([r.size for r in rows] + [0])
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, col.size)
    return rowptr, col, val, n, d


@functools.lru_cache(maxsize=None)
def inputs(case, dt, fp22=False):
    """The data as the context sees it: csr (the tuple for Parameter.csr; FP22: packed words), X (scipy CSR of the m
    rows of Q~ in longdouble from the rounded values), XT (X in the context's type), cost, m, d, nnz."""
    return inputs_from(master(case), dt, fp22, COST[case])


def inputs_from(csr, dt, fp22, cost):
    import scipy.sparse as sp

    T = DTYPES[dt]
    rowptr, col, val, n, d = csr
    v = val.astype(T)
    words = None
    if fp22:
        from plssvm_sparse_fp22_amd import fp22 as codec

        assert T == np.float32
        words = codec.pack(v)
        v = codec.unpack(words, v.size).astype(T)
    m = n - 1
    X = sp.csr_matrix((v.astype(LD), col, rowptr[: m + 1]), shape=(m, d))
    XT = sp.csr_matrix((v, col, rowptr[: m + 1]), shape=(m, d))
    assert X.dtype == LD and XT.dtype == T
    return dict(csr=(rowptr, col, words if fp22 else v, n, d), X=X, Xt=X.T.tocsr(), XT=XT, XTt=XT.T.tocsr(),
                cost=cost, m=m, d=d, n=n, nnz=int(rowptr[m]), dtype=T)


# ---- the K.p reference -------------------------------------------------------------------------------------------------
def kp_reference(inp, p):
    """Q~ p in longdouble: X (X^T p) + QA sum(p) + p / C with q = 0, QA = 1 / C (the last point is empty)."""
    p = np.asarray(p).astype(LD)
    cinv = LD(1) / LD(inp["cost"])
    return inp["X"] @ (inp["Xt"] @ p) + cinv * p.sum() + cinv * p


def kp_scale(inp, p):
    """S = max_i [ sum_j (|k_ij| + |QA| + |q_i| + |q_j|) |p_j| + |p_i| / C ] with q = 0; above SCALE_EXACT_ROWS rows
    without the off-diagonal |k_ij| |p_j| (a smaller S)."""
    ap = np.abs(np.asarray(p).astype(LD))
    cinv = LD(1) / LD(inp["cost"])
    X = inp["X"]
    if inp["m"] <= SCALE_EXACT_ROWS:
        kabs = abs(X @ X.T) @ ap
    else:
        kabs = np.asarray(X.multiply(X).sum(axis=1)).ravel() * ap
    return (kabs + cinv * ap.sum() + cinv * ap).max()


def unit_rows(m):
    rows = {0, 63, 64, m - 1}
    for W in (panel_width(8), panel_width(4)):
        rows.update(r for r in (W - 1, W, 2 * W - 1, 2 * W) if r < m)
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def kp_vectors(case, dt):
    """[3 + units][m] in the context's type: U(1, 2); N(0, 1) on a 2^-10 grid summing to exactly zero; sign 10^U(-6, 0);
    the unit vectors of unit_rows."""
    T = DTYPES[dt]
    m = SHAPES[case][0] - 1
    rng = np.random.default_rng(11)
    rows = unit_rows(m)
    P = np.zeros((3 + len(rows), m))
    P[0] = rng.uniform(1.0, 2.0, m)
    P[1] = grid_normal(rng, m)
    P[2] = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-6.0, 0.0, m)
    P[3 + np.arange(len(rows)), rows] = 1.0
    P = P.astype(T)
    assert P[1].astype(LD).sum() == 0
    P.setflags(write=False)
    return P


def grid_normal(rng, m):
    """N(0, 1) rounded to multiples of 2^-10, the last entry set so that the sum is exactly zero (in any order and
    either type: every partial sum is a multiple of 2^-10 far below 2^13)."""
    g = np.round(rng.standard_normal(m) * 1024.0) / 1024.0
    g[-1] -= g.sum()
    assert abs(g[-1]) < 8192 and g.sum() == 0
    return g


# ---- the CG ------------------------------------------------------------------------------------------------------------
CG_STEPS = {"wide": 4, "wide_ragged": 4, "global": 4, "tall_split": 3}


def gpu_steps(case, dt):
    """Steps the GPU test compares: tall_split in fp32 stops at 2 (the same-type CG's third step is at 1e-3 of the step, its delta at 0.9)."""
    return 2 if (case, dt) == ("tall_split", "f32") else CG_STEPS[case]


@functools.lru_cache(maxsize=None)
def cg_rhs(case, dt, fp22=False):
    """b = Q~ 1 + g in the context's type, g ~ N(0, 1) (tall_split: on the 2^-10 grid with sum(g) = 0 exactly)."""
    inp = inputs(case, dt, fp22)
    rng = np.random.default_rng(21)
    g = grid_normal(rng, inp["m"]) if case == "tall_split" else rng.standard_normal(inp["m"])
    b = (kp_reference(inp, np.ones(inp["m"])) + g.astype(LD)).astype(inp["dtype"])
    b.setflags(write=False)
    return b


def product(inp, dtype):
    """v -> Q~ v in dtype (LD: the reference; the context's type: the same-type CG the bounds come from)."""
    X, Xt = (inp["X"], inp["Xt"]) if dtype is LD else (inp["XT"], inp["XTt"])
    assert X.dtype == dtype
    cinv = dtype(1) / dtype(inp["cost"])

    def mul(v):
        return (X @ (Xt @ v) + cinv * v.sum(dtype=dtype) + cinv * v).astype(dtype)

    return mul


def cg(inp, b, steps, dtype, ad=None):
    """x_0 = 1, r = b - Q~ x, d = r; per step alpha = delta / d.Ad, x += alpha d, r -= alpha Ad, beta = delta' / delta,
    d = r + beta d (no explicit residual: steps < 50). ad(d, k): the product of step k (default Q~ d); it may return
    (Ad, d.Ad) to model a kernel whose fused d.Ad partials differ from its Ad. Returns ([x_0 .. x_steps], [delta_0 ..])."""
    mul = product(inp, dtype)
    b = np.asarray(b).astype(dtype)
    x = np.ones(inp["m"], dtype)
    r = (b - mul(x)).astype(dtype)
    d = r.copy()
    delta = (r * r).sum(dtype=dtype)
    xs, deltas = [x.copy()], [delta]
    for k in range(steps):
        Ad = mul(d) if ad is None else ad(d, k)
        dAd = None
        if isinstance(Ad, tuple):
            Ad, dAd = Ad
        if dAd is None:
            dAd = (d * Ad).sum(dtype=dtype)
        alpha = dtype(delta / dAd)
        x = (x + alpha * d).astype(dtype)
        r = (r - alpha * Ad).astype(dtype)
        new = (r * r).sum(dtype=dtype)
        beta = dtype(new / delta)
        delta = new
        d = (r + beta * d).astype(dtype)
        xs.append(x.copy())
        deltas.append(delta)
    return xs, deltas


@functools.lru_cache(maxsize=None)
def cg_reference(case, dt, fp22=False):
    inp = inputs(case, dt, fp22)
    return cg(inp, cg_rhs(case, dt, fp22), CG_STEPS[case], LD)


def cg_metric(xs, ref_xs):
    """Per step k >= 1: max |x_k - x_k^LD| / max |x_k^LD - x_(k-1)^LD| (the error as a fraction of the step)."""
    return [float(np.abs(np.asarray(xs[k]).astype(LD) - ref_xs[k]).max() / np.abs(ref_xs[k] - ref_xs[k - 1]).max())
            for k in range(1, len(xs))]


def trace_metric(deltas, ref_deltas):
    return [float(abs(LD(deltas[k]) / ref_deltas[k] - 1)) for k in range(1, len(deltas))]


# ---- the same-type numpy CG: where the GPU's bounds come from ----------------------------------------------------------
CG_ORDERS = 8


def _shuffled(A, rng):
    """A with the entries of every row in a random order: scipy's product adds them as stored."""
    import scipy.sparse as sp

    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    o = np.lexsort((rng.random(A.nnz), rows))
    return sp.csr_matrix((A.data[o], A.indices[o], A.indptr.copy()), shape=A.shape)


def numpy_cg_errors(case, dt, fp22=False):
    """cg_metric and trace_metric of the numpy CG in the context's type against the longdouble CG, once per summation
    order: order 0 adds the entries of a row of X and of X^T as they are stored, orders 1 .. CG_ORDERS - 1 in seeded
    random orders. Returns two arrays [CG_ORDERS][steps]."""
    inp = dict(inputs(case, dt, fp22))
    ref_x, ref_d = cg_reference(case, dt, fp22)
    b = cg_rhs(case, dt, fp22)
    XT, XTt = inp["XT"], inp["XTt"]
    ex, et = [], []
    for order in range(CG_ORDERS):
        if order:
            rng = np.random.default_rng(100 + order)
            inp["XT"], inp["XTt"] = _shuffled(XT, rng), _shuffled(XTt, rng)
        xs, ds = cg(inp, b, CG_STEPS[case], inp["dtype"])
        ex.append(cg_metric(xs, ref_x))
        et.append(trace_metric(ds, ref_d))
    return np.array(ex), np.array(et)


# The numpy CG's error per step, measured by test_spmv_regimes_cpu.py (which reruns the measurement and holds it to these
# figures): the largest of numpy_cg_errors over the CG_ORDERS summation orders, rounded up to two digits. One order
# alone is no measurement: where a single long row carries the error (wide_ragged: row 5 and its 5000 products) the
# figure of one order is one draw of that row's rounding, and the orders differ by a factor 17 in x and 370 in delta
# at step 4 in fp32, 30 in x on tall_split; the first version of these tables held the stored order only, which at
# that step is the smallest of the eight. The GPU bounds are 10 x these figures: the margin for the device's own
# summation order, the factor the trace tests use over the oracle's spread. Never filled in from the GPU's output.
NUMPY_CG_ERR = {
    ("wide", "f64", False): [3.8e-15, 1.6e-14, 4.2e-14, 9.5e-14],
    ("wide", "f32", False): [2.2e-06, 7.1e-06, 1.9e-05, 4.4e-05],
    ("wide_ragged", "f64", False): [1.4e-12, 4.3e-13, 2.8e-14, 1.1e-12],
    ("wide_ragged", "f32", False): [0.00059, 0.00019, 8.3e-06, 0.00085],
    ("global", "f64", False): [4.1e-16, 6.4e-16, 5.8e-16, 6.4e-16],
    ("global", "f32", False): [2.1e-07, 3.7e-07, 6e-07, 5e-07],
    ("tall_split", "f64", False): [1.9e-15, 2.1e-15, 2.4e-12],
    ("tall_split", "f32", False): [5.6e-07, 9.7e-07, 0.0011],
    ("wide", "f32", True): [2.1e-06, 7.9e-06, 2.1e-05, 4.8e-05],
}
NUMPY_TRACE_ERR = {
    ("wide", "f64", False): [5.2e-16, 9.7e-16, 1.2e-15, 1.5e-15],
    ("wide", "f32", False): [3e-07, 3.5e-07, 4.4e-07, 5.5e-07],
    ("wide_ragged", "f64", False): [1.3e-11, 6.9e-13, 7.5e-16, 9.5e-16],
    ("wide_ragged", "f32", False): [0.0059, 0.00031, 7e-07, 0.0018],
    ("global", "f64", False): [2.9e-16, 2.5e-16, 5.4e-16, 7.9e-16],
    ("global", "f32", False): [2.1e-07, 2.4e-07, 3.2e-07, 4.3e-07],
    ("tall_split", "f64", False): [2.6e-15, 6.7e-14, 7.4e-14],
    ("tall_split", "f32", False): [1.6e-06, 4e-05, 0.89],
    ("wide", "f32", True): [2.2e-07, 3.9e-07, 5.4e-07, 4.3e-07],
}
GPU_FACTOR = 10.0


def x_bound(case, dt, fp22, k):
    """The GPU's bound on cg_metric at step k >= 1."""
    return GPU_FACTOR * NUMPY_CG_ERR[case, dt, fp22][k - 1]


def trace_bound(case, dt, fp22, k):
    """The GPU's bound on |delta_k / delta_k^LD - 1|: ten times the numpy figure, which is floored at 4 eps of the type
    (a figure below that is one summation order's luck, not the precision of a sum of m squares in the type)."""
    return GPU_FACTOR * max(NUMPY_TRACE_ERR[case, dt, fp22][k - 1], 4 * float(np.finfo(DTYPES[dt]).eps))
