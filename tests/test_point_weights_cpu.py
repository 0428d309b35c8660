"""CPU tests of the point-weight and cost-lane surface that need no device: the two C ABI symbols in the header, the
Python table and the library; their argument validation (a NULL context never reaches the GPU); the host-side checks
of class_weight; plssvm-train's --class_weights in --help and its three malformed uses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")
HEADER = os.path.join(ROOT, "include", "plssvm_mi355x.h")
NEW = ("plssvm_mi_set_point_weights", "plssvm_mi_learn_lanes")


def test_header_table_and_library_agree_on_the_new_symbols():
    with open(HEADER) as f:
        declared = set(re.findall(r"PLSSVM_MI_API\s+[\w\s\*]+?\b(plssvm_mi_\w+)\s*\(", f.read()))
    L = _abi.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _abi.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    assert len(L.plssvm_mi_learn_lanes.argtypes) == 13 and len(L.plssvm_mi_set_point_weights.argtypes) == 2


def test_abi_rejects_bad_arguments_without_a_device():
    L = _abi.lib()
    buf = np.ones(8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    it = np.zeros(2, np.int64).ctypes.data_as(ctypes.c_void_p)
    assert L.plssvm_mi_set_point_weights(None, p) == -1
    assert L.plssvm_mi_set_point_weights(None, None) == -1
    assert L.plssvm_mi_learn_lanes(None, p, 2, 4, p, p, 4, 3, 1e-3, p, None, None, it) == -1
    assert L.plssvm_mi_learn_lanes(None, p, 0, 4, None, None, 0, 3, 1e-3, p, None, None, it) == -1


def test_class_point_weights():
    y = np.array([1.0, -1.0, 1.0, -1.0, -1.0])
    assert np.array_equal(pm.class_point_weights(y, {1: 4.0}), [4, 1, 4, 1, 1])
    assert np.array_equal(pm.class_point_weights(y, {1: 4.0, -1: 0.5}, np.float32), np.float32([4, .5, 4, .5, .5]))
    S = pm.one_vs_all_weights(np.array([3, 7, 3, 9]), {3: 2.0, 9: 5.0})
    assert np.array_equal(S, [[2, 1, 2, 1], [1, 1, 1, 1], [1, 1, 1, 5]])


@pytest.mark.parametrize("bad", [{1: 0.0}, {1: -2.0}, {1: float("nan")}, {1: float("inf")}, {}, [1, 2]])
def test_non_positive_weights_are_rejected(bad):
    with pytest.raises(ValueError):
        pm.Parameter("rbf", class_weight=bad)
    with pytest.raises(ValueError):
        pm.class_point_weights(np.array([1.0, -1.0]), bad)
    with pytest.raises(ValueError):
        pm.one_vs_all_weights(np.array([1, 2, 3]), bad)


def test_parameter_rejects_a_label_the_data_lacks():
    p = pm.Parameter("linear", class_weight={2: 3.0})
    p.data, p.labels = np.zeros((3, 2)), np.array([1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="does not have"):
        p.point_weights()
    p.class_weight = {1: 3.0}
    assert np.array_equal(p.point_weights(), [3, 1, 3])
    assert pm.Parameter("linear").point_weights() is None


def test_learn_multi_rejects_bad_class_weight_before_the_device():
    """learn_multi checks class_weight before it touches the device: a context object without one is enough."""
    p = pm.Parameter("linear")
    p.data = np.zeros((4, 2))
    svm = pm.CSVM.__new__(pm.CSVM)
    svm.params, svm.dtype, svm.num_data_points, svm.num_features = p, np.dtype(np.float64), 4, 2
    svm._ctx, svm._on_device = ctypes.c_void_p(), False
    labels = np.array([1, 2, 3, 1])
    with pytest.raises(ValueError, match="does not have"):
        svm.learn_multi(labels, class_weight={4: 2.0})
    with pytest.raises(ValueError, match="> 0"):
        svm.learn_multi(labels, class_weight={1: 0.0})


def test_train_help_lists_class_weights():
    out = subprocess.run([TRAIN, "--help"], capture_output=True, text=True, check=True).stdout
    assert "--class_weights" in out


@pytest.mark.parametrize("extra", [[], ["--multiclass"]], ids=["binary", "multiclass"])
@pytest.mark.parametrize("arg,reads_file", [("1:2,3", False), ("1:0", False), ("1:-1.5", False), ("5:2", True)],
                         ids=["malformed", "zero", "negative", "missing-label"])
def test_train_rejects_bad_class_weights(tmp_path, arg, reads_file, extra):
    """Syntax and sign are rejected before the file is read (the file named here does not exist); a label the file
    lacks once it has been read, before any device is touched."""
    f = tmp_path / "t.libsvm"
    if reads_file:
        f.write_text("1 0:0.5 1:1\n2 0:1 1:0.25\n3 0:0.1 1:0.2\n1 0:0.3 1:0.9\n")
    model = tmp_path / "t.model"
    r = subprocess.run([TRAIN, "-q", *extra, "--class_weights", arg, str(f), str(model)], capture_output=True, text=True)
    assert r.returncode == 1
    assert "--class_weights" in r.stderr
    assert not model.exists()
