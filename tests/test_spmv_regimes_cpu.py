"""CPU side of the factored sparse-linear regime tests (tests/spmv_regime_cases.py): the shapes sit in
the regimes they were built for, the longdouble reference agrees with the oracle, the bounds of the GPU's CG test are
what a same-type numpy CG measures against the longdouble CG, and those bounds have teeth: a product altered the way a
broken row-block kernel would alter it exceeds them at least tenfold.
"""
import numpy as np
import pytest

import spmv_regime_cases as sc

LD = sc.LD
CG_RUNS = [(c, dt, False) for c in sc.CG_STEPS for dt in ("f64", "f32")] + [("wide", "f32", True)]
CG_IDS = [f"{c}-{dt}{'-fp22' if f else ''}" for c, dt, f in CG_RUNS]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(sc.SHAPES))
def test_case_sits_in_its_regime(case, dt):
    n, d, _ = sc.SHAPES[case]
    rowptr = sc.master(case)[0]
    m = n - 1
    assert rowptr[m] == rowptr[n], "the last point is an empty row"
    r = sc.plan_rule(m, d, int(rowptr[m]), dt)
    want = sc.TABLE[case][dt]
    assert (r["csc"]["P"], r["csc"]["ldsx"]) == want["csc"], r
    assert (r["csr"]["P"], r["csr"]["ldsx"]) == want["csr"], r
    assert (r["rb"]["P"], r["rb"]["RBK"], r["rb"]["nblk"]) == want["rb"], r
    size = np.dtype(sc.DTYPES[dt]).itemsize
    if case == "tall":  # the unsplit reduction, more than one panel
        assert 1 < r["csc"]["P"] < sc.SPLIT_PANELS
    if case == "tall_split":  # the split reduction; a second round of the finalize loop; fp64 at the cap
        assert r["csc"]["P"] >= sc.SPLIT_PANELS and r["rb"]["RBK"] > sc.FIN_ROWS_PER_ROUND and m > 16 * 40960
        assert (r["rb"]["RBK"] == sc.RB_ACC_BYTES // size) == (dt == "f64")
    if case in ("wide", "wide_ragged"):  # a ragged last panel in both plans
        assert d % sc.panel_width(size) == 4041 and d % sc.rowblock_width(size) != 0


def test_data_is_what_the_cases_promise():
    rowptr, col, _, n, d = sc.master("wide")
    assert set(sc.edge_columns(d)) <= set(col[rowptr[0]:rowptr[1]])
    rowptr, col, _, n, d = sc.master("global")
    assert set(sc.edge_columns(d)) <= set(col[rowptr[0]:rowptr[1]])
    rowptr, col, val, n, d = sc.master("wide_ragged")
    lens = np.diff(rowptr)
    m = n - 1
    assert (lens[:m:97] == 0).all() and lens[5] == 5000 and sc.EMPTY_COLUMN not in set(col)
    for r in (1, 4, 7, 2998):
        assert col[rowptr[r]:rowptr[r + 1]].min() >= sc.LAST_PANEL_FROM
    assert {39, 41} <= set(lens[:m]) and len({int(c) // 18432 for c in col[rowptr[5]:rowptr[6]]}) == 3
    rowptr, col, val, n, d = sc.master("tall_split")
    v = val.reshape(-1, 3)
    assert np.array_equal(v[0::2], -v[1::2]) and (n - 1) == 11 * 2 ** 16
    X = sc.inputs("tall_split", "f32")["X"]
    assert not np.asarray(X.sum(axis=0)).any()  # column sums exactly zero


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_reference_agrees_with_the_oracle(oracle, dt):
    """300 x 500, 6 entries per row, the last row empty: the longdouble K.p within the oracle's own contract."""
    T = sc.DTYPES[dt]
    rng = np.random.default_rng(5)
    n, d, k = 301, 500, 6
    cols = np.sort(np.argsort(rng.random((n - 1, d)), axis=1)[:, :k], axis=1)
    rowptr = np.concatenate([np.arange(0, (n - 1) * k + 1, k), [(n - 1) * k]]).astype(np.int64)
    csr = (rowptr, cols.reshape(-1).astype(np.int32), rng.uniform(-1, 1, (n - 1) * k), n, d)
    inp = sc.inputs_from(csr, dt, False, 10.0)
    data = oracle.Data(rowptr=rowptr, col=csr[1], val=inp["csr"][2], n=n, d=d, dtype=T)
    q = oracle.generate_q("linear", data)
    assert not q.any()
    P = np.stack([rng.uniform(1, 2, n - 1), sc.grid_normal(rng, n - 1), np.eye(n - 1)[63]]).astype(T)
    for v, add in ((0, 1.0), (1, -1.0), (2, 1.0)):
        got = oracle.kp("linear", data, q, T(0.1), T(10.0), add, P[v])
        ref = LD(add) * sc.kp_reference(inp, P[v])
        assert np.abs(got - ref).max() <= sc.KP_TOL[dt] * sc.kp_scale(inp, P[v]), v
    assert np.abs(got - ref).max() <= sc.KP_TOL[dt] * np.abs(ref).max()  # a column of Q~ against its own size


@pytest.mark.parametrize("case,dt,fp22", CG_RUNS, ids=CG_IDS)
def test_numpy_cg_sets_the_gpu_bounds(case, dt, fp22):
    """The same-type numpy CG against the longdouble CG over CG_ORDERS summation orders: the recorded figures
    (NUMPY_CG_ERR, NUMPY_TRACE_ERR) are the largest of this measurement rounded up, and not more than 8 times it."""
    ex, et = sc.numpy_cg_errors(case, dt, fp22)
    mx, mt = ex.max(0), et.max(0)
    print(f"({case!r}, {dt!r}, {fp22}): x {['%.2e' % v for v in mx]} (smallest order {['%.2e' % v for v in ex.min(0)]}) "
          f"trace {['%.2e' % v for v in mt]} (smallest order {['%.2e' % v for v in et.min(0)]})")
    rec_x, rec_t = sc.NUMPY_CG_ERR[case, dt, fp22], sc.NUMPY_TRACE_ERR[case, dt, fp22]
    assert len(rec_x) == len(mx) and len(rec_t) == len(mt)
    for k, (got, rec) in enumerate(zip(mx, rec_x)):
        assert rec / 8 <= got <= rec, ("x", k + 1, got, rec)
    for k, (got, rec) in enumerate(zip(mt, rec_t)):
        assert got <= rec, ("trace", k + 1, got, rec)


def test_one_summation_order_is_no_measurement():
    """Why the figures are taken over several orders: on wide_ragged in fp32 the orders of the same numpy CG differ by
    more than the GPU's whole margin of 10 at step 4 (row 5's 5000 products carry the error; one order is one draw)."""
    ex, et = sc.numpy_cg_errors("wide_ragged", "f32")
    assert ex[:, 3].max() > sc.GPU_FACTOR * ex[:, 3].min()
    assert et[:, 3].max() > sc.GPU_FACTOR * et[:, 3].min()


# ---- teeth -------------------------------------------------------------------------------------------------------------
def _altered(inp, dt, kind):
    """Q~ d as a broken sell_rowblock_fin_kernel would form it, in the context's type."""
    T = inp["dtype"]
    size = np.dtype(T).itemsize
    rb = sc.rowblock_rule(inp["m"], inp["d"], size)
    W, RBK = rb["W"], rb["RBK"]
    mul = sc.product(inp, T)
    XT, XTt = inp["XT"], inp["XTt"]
    state = {}

    def ad(d, k):
        out = mul(d)
        if kind == "panel_dropped":  # row 0 (an entry in every panel) without its panel-1 sum
            w = XTt @ d
            row = XT[0]
            sel = (row.indices >= W) & (row.indices < 2 * W)
            assert sel.any()
            out[0] -= T((row.data[sel] * w[row.indices[sel]]).sum())
            return out
        if kind == "racc_carried":  # one row of block 1 starts from block 0's accumulator
            raw = XT @ (XTt @ d)
            out[RBK + 3] += raw[3]
            return out
        assert kind == "unfinalized" and RBK > sc.FIN_ROWS_PER_ROUND
        stale = np.arange(RBK + sc.FIN_ROWS_PER_ROUND, 2 * RBK)  # rows t >= 1024 of block 1: Ad keeps its old content
        out[stale] = state.get("Ad", np.zeros(inp["m"], T))[stale]
        state["Ad"] = out.copy()
        keep = np.ones(inp["m"], bool)
        keep[stale] = False
        return out, (d[keep] * out[keep]).sum(dtype=T)

    return ad


TEETH = [("wide", "f64", "panel_dropped"), ("wide", "f32", "panel_dropped"), ("wide", "f64", "racc_carried"),
         ("wide", "f32", "racc_carried"), ("tall_split", "f64", "racc_carried"),
         ("tall_split", "f64", "unfinalized"), ("tall_split", "f32", "unfinalized")]
# Not in the list: a single carried-over row on tall_split in fp32. Its two steps show it at 1.3e-5 of the step, which
# is 1.3 times the GPU bound there (9.7e-6), not ten times: the step's largest entry dwarfs one row's share. The carried
# row has its teeth in fp32 on wide (8.8 against 4.4e-4) and on tall_split's plan in fp64 (1.2e-2 against 2.4e-11).


@pytest.mark.parametrize("case,dt,kind", TEETH)
def test_bounds_have_teeth(case, dt, kind):
    """Each alteration of the fused pass's product is ten times past the GPU bound on x at the last step."""
    inp = sc.inputs(case, dt)
    ref_x, _ = sc.cg_reference(case, dt)
    steps = sc.gpu_steps(case, dt)
    xs, _ = sc.cg(inp, sc.cg_rhs(case, dt), steps, inp["dtype"], ad=_altered(inp, dt, kind))
    m = sc.cg_metric(xs, ref_x[: steps + 1])
    bound = [sc.GPU_FACTOR * v for v in sc.NUMPY_CG_ERR[case, dt, False][:steps]]
    print(case, dt, kind, ["%.2e" % v for v in m], "bounds", ["%.2e" % v for v in bound])
    assert m[-1] >= 10 * bound[-1], (m, bound)
