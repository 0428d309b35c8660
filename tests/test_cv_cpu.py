"""k-fold cross-validation without a device: the two new ABI symbols, stratified_folds, the
re-pivoted arithmetic of held-out lanes in numpy against the bordered direct solve (tests/cv_reference.py, the
reference of tests/test_gpu_cv.py), and what plssvm-train -v refuses from its options alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cv_reference as ref
import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "plssvm_mi355x.h")
TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")
NEW = {"plssvm_mi_learn_held": 16, "plssvm_mi_train_values": 7}


def header_arity(name):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"PLSSVM_MI_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_abi_and_library_agree(name):
    assert name in _abi.EXPORTS
    L = _abi.lib()
    fn = getattr(L, name)
    assert fn.restype is ctypes.c_int
    assert header_arity(name) == NEW[name] == len(fn.argtypes)


def test_a_null_context_is_err_arg():
    L = _abi.lib()
    buf = np.zeros(4)
    hold = np.zeros(4, dtype=np.uint8)
    it = np.zeros(1, dtype=np.int64)
    assert L.plssvm_mi_learn_held(None, pm._ptr(buf), 1, 4, None, None, 0, pm._ptr(hold), 4, 1, 1e-3, pm._ptr(buf), pm._ptr(buf),
                                  None, pm._ptr(it), None) == -1
    assert L.plssvm_mi_train_values(None, pm._ptr(buf), 1, 4, pm._ptr(buf), pm._ptr(buf), 4) == -1


def test_info_keeps_its_size():
    assert ctypes.sizeof(_abi.Info) == 232  # plssvm_mi_info's size before the two calls were added


@pytest.mark.parametrize("nfold", [2, 3, 5, 7])
def test_stratified_folds_spread_every_label_evenly(nfold):
    rng = np.random.default_rng(nfold)
    labels = rng.choice([-1.0, 1.0, 3.0], size=103, p=[0.6, 0.3, 0.1])
    folds = pm.stratified_folds(labels, nfold)
    assert folds.shape == (103,) and folds.min() == 0 and folds.max() == nfold - 1
    for lab in np.unique(labels):
        c = int((labels == lab).sum())
        per = np.bincount(folds[labels == lab], minlength=nfold)
        assert per.min() >= c // nfold and per.max() <= -(-c // nfold), (lab, per)
        # the rule itself: rank among the label's points, in index order, mod nfold
        assert np.array_equal(folds[labels == lab], np.arange(c) % nfold)
    assert np.array_equal(folds, pm.stratified_folds(labels.copy(), nfold)), "the folds are not deterministic"


def test_stratified_folds_bounds():
    labels = np.array([1.0, -1.0, 1.0, -1.0])
    for bad in (1, 0, -3, 5):
        with pytest.raises(ValueError):
            pm.stratified_folds(labels, bad)
    assert np.array_equal(pm.stratified_folds(labels, 4), [0, 0, 1, 1])
    with pytest.raises(ValueError):
        pm.stratified_folds(np.array([]), 2)


@pytest.mark.parametrize("kernel", ["rbf", "laplacian", "linear"])
def test_repivoted_masked_cg_is_the_direct_subset_solve(kernel):
    """The arithmetic of a held-out lane, run by numpy in float64 at epsilon 1e-10 on 301 x 12 for every hold pattern of
    the GPU tests: the principal submatrix of Q~ on the active rows with the pivot's q and QA, the CG from x0 = 1,
    the tail. Against the bordered direct solve on the training points: within 1e-5 of max|alpha| (the recurrence
    leaves 4e-12 .. 4e-7 there), zeros on the held-out points, the full-data model at least 0.04 away."""
    n, d = 301, 12
    X, y, g, K = ref.blobs_case(n, d, np.float64, kernel)
    diag = ref.diagonal(4.0, None, n, np.float64)
    full, _ = ref.direct_subset(K, y, np.zeros(n, dtype=bool), diag)
    for name, hold in ref.hold_patterns(n).items():
        t, R, Q, b, q, QA = ref.pivot_system(K, y, hold, diag)
        assert t == np.flatnonzero(~hold)[-1] and t not in R and not hold[R].any()
        x, trace, it = ref.cg(Q, b, 1e-10, 2000)
        alpha, bias = ref.lane_from_x(n, y, t, R, q, QA, x)
        a_ref, b_ref = ref.direct_subset(K, y, hold, diag)
        scale = np.abs(a_ref).max()
        err = max(np.abs(alpha - a_ref).max(), abs(bias - b_ref)) / scale
        assert 0 < it < 2000 and trace.size == it + 1
        assert err <= 1e-5, (name, err)
        assert np.all(alpha[hold] == 0.0) and abs(alpha.sum()) <= 1e-9 * np.abs(alpha).sum()
        if hold.any():
            assert np.abs(full[~hold] - a_ref[~hold]).max() / scale > 0.04, name
            # the held-out decisions of both are the same to the solve's accuracy
            f_cg, f_ref = K[hold] @ alpha + bias, K[hold] @ a_ref + b_ref
            assert np.abs(f_cg - f_ref).max() <= 1e-5 * scale * np.abs(K).sum(axis=1).max()
    names = list(ref.hold_patterns(n))
    assert names == ["a0", "a1", "a2", "a3", "a4", "b", "c", "d"]


def test_repivoting_with_point_weights():
    n, d = 301, 12
    X, y, g, K = ref.blobs_case(n, d, np.float64, "rbf", True)
    s = np.where(y > 0, 3.0, 1.0)
    diag = ref.diagonal(4.0, s, n, np.float64)
    hold = ref.hold_patterns(n)["c"]
    t, R, Q, b, q, QA = ref.pivot_system(K, y, hold, diag)
    assert t == n - 8 and QA == K[t, t] + diag[t]
    x, _, _ = ref.cg(Q, b, 1e-10, 2000)
    alpha, bias = ref.lane_from_x(n, y, t, R, q, QA, x)
    a_ref, b_ref = ref.direct_subset(K, y, hold, diag)
    assert max(np.abs(alpha - a_ref).max(), abs(bias - b_ref)) <= 1e-5 * np.abs(a_ref).max()


def run_train(*args):
    r = subprocess.run([TRAIN] + list(args), capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout, r.stderr


def test_help_lists_the_cross_validation_options():
    code, out, _ = run_train("--help")
    assert code == 0
    assert re.search(r"^\s+-v, --cross_validation arg", out, flags=re.M) and re.search(r"^\s+--cv_costs arg", out, flags=re.M)


@pytest.mark.parametrize("args,word", [(["-v", "1"], "n >= 2"), (["-v", "0"], "n >= 2"), (["-v", "x"], "n >= 2"),
                                       (["-v", "5", "--multiclass"], "--multiclass"),
                                       (["-v", "5", "--devices", "0,1"], "one device"),
                                       (["--cv_costs", "1,10"], "needs -v"),
                                       (["-v", "5", "--cv_costs", "1,-2"], "--cv_costs"),
                                       (["-v", "5", "--cv_costs", "1,,2"], "--cv_costs")],
                         ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_refusals_from_the_options_alone(args, word, tmp_path):
    missing = str(tmp_path / "no_such_file.libsvm")
    code, out, err = run_train(*args, missing)
    assert code == 1
    assert word in err, err
    assert "find file" not in err and "find file" not in out, "the file was opened before the options were refused"
    assert os.listdir(tmp_path) == []
