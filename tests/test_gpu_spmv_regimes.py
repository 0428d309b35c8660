"""The factored sparse-linear SpMV passes and the fused row-block CG pass in every plan regime, against longdouble
references (cases, data, references and bounds: tests/spmv_regime_cases.py).

Every test first holds CSVM.spmv_plan() to the restated plan rule, so a case that drifted out of its regime fails
rather than passing on the one-panel path.

K.p (sell_spmv_kernel MODE 0, panel_reduce_kernel): all five cases in fp64 and fp32, FP22 input on wide, tall and
global; vectors U(1, 2), a zero-sum grid vector with add = -1, sign 10^U(-6, 0) and unit vectors at rows 0, 63, 64,
W - 1, W, 2 W - 1, 2 W (both types' W, where below m) and m - 1; bound 1e-12 / 1e-4 of the term-wise scale S
(kp_scale). generate_q is exactly zero and QA_cost = 1 / C (the last point is empty); update_w against longdouble
X^T alpha (tall, tall_split: the CSC plan through predict.hip) at the same constants of max_f sum_i |x_if| |alpha_i|;
three simulated ranks on wide sum to the full K.p (a CSR pass at raw + r0 with P > 1).

Fused CG pass (sell_rowblock_fin_kernel): cg_begin(b, eps = 1e-30), cg_step(k, force = True), cg_result(k + 1) for
k = 1 .. 4 on wide, wide_ragged, global (fp64, fp32; wide also FP22 and cg_variant = "one_reduction"), k = 1 .. 2 (fp32)
and 1 .. 3 (fp64) on tall_split; x_k elementwise against the longdouble CG as a fraction of the step
max |x_k - x_(k-1)|, trace[k] against its delta_k. Bounds: 10 x the error of a same-type numpy CG against the same
reference (spmv_regime_cases.NUMPY_CG_ERR / NUMPY_TRACE_ERR, re-measured by test_spmv_regimes_cpu.py), e.g.
wide fp64 step 4: numpy 9.5e-14, bound 9.5e-13; tall_split fp32 step 2: numpy 9.7e-7, bound 9.7e-6. One graph block
on wide: delta_50 is the longdouble |b - Q~ x_50|^2 within 4 sqrt(m) u || M |x_50| ||, delta_49 < 1e-2 delta_0.

MEASURED on an MI355X (fp64 / fp32; every plan assertion hit; the 31 tests take 6.2 s together, the slowest 1.1 s):

    K.p, worst vector, of S   wide 3.1e-16 / 1.7e-7, wide_ragged 2.4e-16 / 2.1e-7, tall 2.5e-16 / 9.6e-8,
                              tall_split 2.6e-16 / 2.0e-7, global 3.3e-16 / 9.0e-8; FP22 wide 1.7e-7, tall 9.9e-8,
                              global 8.7e-8; three simulated ranks 1.4e-16 / 9.6e-8
    update_w                  tall 7.8e-17 / 7.3e-8, tall_split 2.3e-17 / 1.7e-8
    graph block (wide)        |sqrt(delta_50) - explicit| 2.8e-14 / 2.5e-5 (bounds 5.5e-11 / 3.0e-2)

    CG, x_k as a fraction of the step, steps 1 .. : GPU (numpy same-type CG, the largest of 8 summation orders; the
    bound is 10 x the latter)
    wide fp64            2.2e-15 (3.8e-15)  8.1e-15 (1.6e-14)  2.1e-14 (4.2e-14)  5.0e-14 (9.5e-14)
    wide fp32            1.5e-6 (2.2e-6)    5.5e-6 (7.1e-6)    1.6e-5 (1.9e-5)    3.6e-5 (4.4e-5)
    wide fp32 FP22       1.9e-6 (2.1e-6)    7.2e-6 (7.9e-6)    2.0e-5 (2.1e-5)    4.3e-5 (4.8e-5)
    wide fp64 one-red.   2.2e-15            8.1e-15            2.1e-14            5.0e-14
    wide_ragged fp64     4.8e-14 (1.4e-12)  2.0e-14 (4.3e-13)  1.2e-14 (2.8e-14)  1.1e-12 (1.1e-12)
    wide_ragged fp32     1.0e-4 (5.9e-4)    3.1e-5 (1.9e-4)    1.1e-5 (8.3e-6)    1.2e-3 (8.5e-4)
    global fp64          4.1e-16 (4.1e-16)  4.9e-16 (6.4e-16)  5.7e-16 (5.8e-16)  5.4e-16 (6.4e-16)
    global fp32          1.6e-7 (2.1e-7)    2.5e-7 (3.7e-7)    3.0e-7 (6.0e-7)    1.7e-7 (5.0e-7)
    tall_split fp64      1.1e-16 (1.9e-15)  1.2e-16 (2.1e-15)  9.1e-15 (2.4e-12)
    tall_split fp32      5.7e-8 (5.6e-7)    2.3e-7 (9.7e-7)
    delta_k: at most 1.5e-15 / 2.2e-7 of the reference on wide, global and tall_split (fp32 step 2 there: 1.3e-6,
    numpy 4.0e-5); wide_ragged 4.7e-13 / 3.6e-3 (numpy 1.3e-11 / 5.9e-3).

The numpy figures are the largest over eight summation orders of the same numpy CG (spmv_regime_cases.numpy_cg_errors).
With the stored order alone wide_ragged in fp32 missed at step 4 (x 1.2e-3 against 10 x 4.9e-5): there row 5's 5000
products carry the error, the figure of one order is a single draw of that row's rounding, and the eight orders give
4.9e-5 .. 8.5e-4 in x and 4.9e-6 .. 1.8e-3 in delta (test_one_summation_order_is_no_measurement). The same kernel on
the same plan in fp64 is at 1.1e-12 against numpy's 1.1e-12.
"""
import functools

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
import spmv_regime_cases as sc
from plssvm_sparse_fp22_amd import _abi

pytestmark = pytest.mark.gpu
LD = sc.LD

KP_RUNS = [(c, dt, False) for c in sc.SHAPES for dt in ("f64", "f32")] + [(c, "f32", True) for c in sc.FP22_CASES]
CG_RUNS = [(c, dt, False) for c in sc.CG_STEPS for dt in ("f64", "f32")] + [("wide", "f32", True)]


def _ids(runs):
    return [f"{c}-{dt}{'-fp22' if f else ''}" for c, dt, f in runs]


def _make(case, dt, fp22, **kw):
    inp = sc.inputs(case, dt, fp22)
    p = pm.Parameter("linear", cost=inp["cost"], real_type=sc.DTYPES[dt])
    p.csr = inp["csr"]
    if fp22:
        p.val_fmt = _abi.VAL_FP22
    svm = pm.CSVM(p, **kw)
    svm.setup_data_on_device()
    return svm


def _assert_plan(svm, case, dt, fp22, **kw):
    inp = sc.inputs(case, dt, fp22)
    got, want = svm.spmv_plan(), sc.plan_rule(inp["m"], inp["d"], inp["nnz"], dt, fp22, **kw)
    assert not sc.plan_matches(got, want), (got, want)
    if not kw:
        t = sc.TABLE[case][dt]
        assert (got["csc"]["P"], got["csc"]["ldsx"]) == t["csc"] and (got["csr"]["P"], got["csr"]["ldsx"]) == t["csr"]
        assert (got["rb"]["P"], got["rb"]["RBK"], got["rb"]["nblk"]) == t["rb"]
    return got


@functools.lru_cache(maxsize=None)
def _kp(case, dt, fp22):
    T = sc.DTYPES[dt]
    P = sc.kp_vectors(case, dt)
    with _make(case, dt, fp22) as svm:
        _assert_plan(svm, case, dt, fp22)
        q = svm.generate_q().copy()
        out = [svm.run_device_kernel(None, np.zeros(P.shape[1], T), P[v], -1.0 if v == 1 else 1.0).copy()
               for v in range(P.shape[0])]
        return q, svm.QA_cost, out


@pytest.mark.parametrize("case,dt,fp22", KP_RUNS, ids=_ids(KP_RUNS))
def test_kp_in_every_regime(case, dt, fp22):
    inp, P = sc.inputs(case, dt, fp22), sc.kp_vectors(case, dt)
    q, qa, out = _kp(case, dt, fp22)
    assert not q.any()  # k(x_i, x_m) with the last point empty: exactly zero
    assert abs(LD(qa) - LD(1) / LD(inp["cost"])) <= sc.KP_TOL[dt] / inp["cost"]
    failures, worst = [], 0.0
    for v, got in enumerate(out):
        add = LD(-1.0 if v == 1 else 1.0)
        assert np.isfinite(got).all(), v
        r = float(np.abs(got.astype(LD) - add * sc.kp_reference(inp, P[v])).max() / sc.kp_scale(inp, P[v]))
        worst = max(worst, r)
        if not r <= sc.KP_TOL[dt]:
            failures.append((v, r))
    print(f"\n[kp {case}-{dt}{'-fp22' if fp22 else ''}] worst {worst:.2e} of S (tolerance {sc.KP_TOL[dt]:g})")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", ["tall", "tall_split"])
def test_update_w_through_the_csc_plan(case, dt):
    inp = sc.inputs(case, dt)
    alpha = np.random.default_rng(3).standard_normal(inp["n"]).astype(sc.DTYPES[dt])
    with _make(case, dt, False) as svm:
        _assert_plan(svm, case, dt, False)
        w = svm.update_w(alpha).copy()
    a = alpha[: inp["m"]].astype(LD)  # the last point is an empty row
    ref, scale = inp["Xt"] @ a, (abs(inp["Xt"]) @ np.abs(a)).max()
    r = float(np.abs(w.astype(LD) - ref).max() / scale)
    print(f"\n[update_w {case}-{dt}] {r:.2e} of max_f sum |x| |alpha| (tolerance {sc.KP_TOL[dt]:g})")
    assert r <= sc.KP_TOL[dt]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_simulated_ranks_sum_to_the_full_kp(dt):
    case, world = "wide", 3
    inp, T = sc.inputs(case, dt), sc.DTYPES[dt]
    p = sc.kp_vectors(case, dt)[0]
    full = sc.plan_rule(inp["m"], inp["d"], inp["nnz"], dt)
    total = np.zeros(inp["m"], LD)
    slots = 0
    for r in range(world):
        with _make(case, dt, False, sim_rank=(r, world)) as svm:
            got = svm.spmv_plan()
            # a rank's CSR pass covers its own rows with the full pass's panels; no row blocks outside one real GPU
            assert got["rb"] == dict(P=0, W=0, RBK=0, nblk=0), got
            assert {k: got["csc"][k] for k in full["csc"]} == full["csc"], got
            assert (got["csr"]["P"], got["csr"]["ldsx"], got["csr"]["W"]) == (full["csr"]["P"], 1, full["csr"]["W"]), got
            assert got["csr"]["P"] > 1 and got["csr"]["nchunks"] < full["csr"]["nchunks"]
            slots += got["csr"]["nchunks"] // got["csr"]["P"] * 64
            svm.generate_q()
            total += svm.run_device_kernel(None, np.zeros(inp["m"], T), p, 1.0).astype(LD)
    r = float(np.abs(total - sc.kp_reference(inp, p)).max() / sc.kp_scale(inp, p))
    assert slots >= inp["m"]  # the ranks' rows cover every row
    print(f"\n[simulated ranks wide-{dt}] {r:.2e} of S")
    assert r <= sc.KP_TOL[dt]


def _cg_check(case, dt, fp22, **kw):
    inp = sc.inputs(case, dt, fp22)
    b = sc.cg_rhs(case, dt, fp22)
    ref_x, ref_d = sc.cg_reference(case, dt, fp22)
    failures = []
    with _make(case, dt, fp22, **kw) as svm:
        plan = _assert_plan(svm, case, dt, fp22)
        assert plan["rb"]["nblk"] > 0  # the fused pass is the one the CG runs
        svm.generate_q()
        for k in range(1, sc.gpu_steps(case, dt) + 1):
            svm.cg_begin(b, eps=1e-30)
            it, _ = svm.cg_step(k, force=True)
            assert it == k
            x, tr, _ = svm.cg_result(k + 1)
            assert len(tr) == k + 1 and np.isfinite(x).all()
            ex = float(np.abs(x.astype(LD) - ref_x[k]).max() / np.abs(ref_x[k] - ref_x[k - 1]).max())
            et = float(abs(LD(tr[k]) / ref_d[k] - 1))
            bx, bt = sc.x_bound(case, dt, fp22, k), sc.trace_bound(case, dt, fp22, k)
            print(f"[cg {case}-{dt}{'-fp22' if fp22 else ''}{' one_reduction' if kw else ''}] step {k}: x {ex:.2e} (bound {bx:.2e}), "
                  f"delta {et:.2e} (bound {bt:.2e})")
            if not ex <= bx:
                failures.append(("x", k, ex, bx))
            if not et <= bt:
                failures.append(("delta", k, et, bt))
    assert not failures, failures


@pytest.mark.parametrize("case,dt,fp22", CG_RUNS, ids=_ids(CG_RUNS))
def test_fused_cg_pass_against_the_longdouble_cg(case, dt, fp22):
    print()
    _cg_check(case, dt, fp22)


def test_fused_cg_pass_one_reduction_variant():
    print()
    _cg_check("wide", "f64", False, cg_variant="one_reduction")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_graph_block_ends_on_the_explicit_residual(dt):
    case = "wide"
    inp, T = sc.inputs(case, dt), sc.DTYPES[dt]
    b = sc.cg_rhs(case, dt)
    with _make(case, dt, False) as svm:
        _assert_plan(svm, case, dt, False)
        svm.generate_q()
        svm.cg_begin(b, eps=1e-30)
        it, _ = svm.cg_step(50, force=True)
        assert it == 50
        x, tr, _ = svm.cg_result(51)
    assert len(tr) == 51
    xl = x.astype(LD)
    r = b.astype(LD) - sc.kp_reference(inp, xl)
    cinv = LD(1) / LD(inp["cost"])
    ax = np.abs(xl)
    M_ax = abs(inp["X"] @ inp["Xt"]) @ ax + cinv * ax.sum() + cinv * ax  # the magnitudes of Q~'s terms, q = 0
    u = np.finfo(T).eps / 2
    bound = 4 * np.sqrt(inp["m"]) * u * float(np.sqrt(M_ax @ M_ax))
    got, true = float(np.sqrt(tr[50])), float(np.sqrt(r @ r))
    print(f"\n[graph block wide-{dt}] sqrt(delta_50) {got:.6e}, explicit {true:.6e}, bound {bound:.2e}; "
          f"delta_49 / delta_0 {tr[49] / tr[0]:.2e}")
    assert abs(got - true) <= bound
    assert tr[49] < 1e-2 * tr[0]
