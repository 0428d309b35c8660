"""CPU tests of the multi-class surface that need no device: the one-vs-all coding, host-side argument checks and the
C ABI's argument validation (a NULL context never reaches the GPU)."""
import ctypes

import numpy as np
import pytest

import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_vs_all(dtype):
    labels = np.array([3, -1, 3, 7, -1, 3])
    classes, Y = pm.one_vs_all(labels, dtype)
    assert np.array_equal(classes, [-1, 3, 7])
    assert Y.dtype == dtype and Y.shape == (3, 6) and Y.flags.c_contiguous
    assert np.array_equal(Y, [[-1, 1, -1, -1, 1, -1], [1, -1, 1, -1, -1, 1], [-1, -1, -1, 1, -1, -1]])
    assert np.array_equal(Y.sum(axis=0), np.full(6, 2 - 3))  # every point is in exactly one class


def test_one_vs_all_float_labels_and_errors():
    classes, Y = pm.one_vs_all(np.array([0.5, 2.5, 0.5]))
    assert np.array_equal(classes, [0.5, 2.5]) and np.array_equal(Y, [[1, -1, 1], [-1, 1, -1]])
    for bad in (np.array([]), np.zeros((2, 2)), np.array(["a", "b"]), np.array([1.0, np.nan])):
        with pytest.raises(ValueError):
            pm.one_vs_all(bad)


def test_rows_helper_checks_the_leading_dimension():
    a = pm._rows(np.arange(5.0), np.float64, 5, "P")
    assert a.shape == (1, 5)
    with pytest.raises(ValueError, match="at least 6"):
        pm._rows(np.zeros((2, 5)), np.float64, 6, "P")


def test_abi_rejects_bad_arguments_without_a_device():
    L = _abi.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    it = np.zeros(2, np.int64).ctypes.data_as(ctypes.c_void_p)
    assert L.plssvm_mi_kp_multi(None, None, p, p, 1, 8, 1.0) == -1
    assert L.plssvm_mi_solve_cg_multi(None, p, 1, 8, None, 3, 1e-3, p, None, it) == -1
    assert L.plssvm_mi_learn_multi(None, p, 2, 4, 3, 1e-3, p, None, None, it) == -1
    assert L.plssvm_mi_time_kp_multi(None, 1, 1, None) == -1
    assert _abi.OPT_MULTI_WIDTH == 7 and "multi_width" in [f[0] for f in _abi.Info._fields_]
