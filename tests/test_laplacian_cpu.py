"""The Laplacian kernel k(x, z) = exp(-gamma ||x - z||_1) on the CPU side: its id in the C ABI and in the Python
mirror, model files with `kernel_type laplacian` through the Python and the C++ readers and writers, the CLI's help
text, and the refusal of sparse data before any GPU call. No device is needed.

io.write_model writes one-vs-all models only (tests/test_model_multi.py pins its refusal of two classes), so the
two-class layout is checked on a file written out here, the one-vs-all layout through write_model.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import _abi
from plssvm_sparse_fp22_amd import io as pio

DTYPES = {"float": np.float32, "double": np.float64}
TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")
HOST = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "host")

TWO_CLASS = """svm_type c_svc
kernel_type {kernel}
gamma 0.125
nr_class 2
total_sv 3
rho 0.25
label 1 -1
nr_sv 2 1
SV
0.5 0:1.000000e+00 2:-2.500000e-01
-1.5 1:5.000000e-01
1 0:-7.500000e-01 2:2.000000e+00
"""


def _driver(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp("drv") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", HOST, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def parse_driver(tmp_path_factory):
    return _driver(tmp_path_factory, "parse_driver")


@pytest.fixture(scope="module")
def multi_driver(tmp_path_factory):
    return _driver(tmp_path_factory, "model_multi_driver")


def test_kernel_id_agrees_with_the_header():
    text = open(os.path.join(ROOT, "include", "plssvm_mi355x.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PLSSVM_MI_KERNEL_(\w+) (\d+)", text)}
    assert ids == {"LINEAR": 0, "POLYNOMIAL": 1, "RBF": 2, "LAPLACIAN": 4}
    assert _abi.KERNELS["laplacian"] == ids["LAPLACIAN"] == 4
    assert "sigmoid" not in _abi.KERNELS and 3 not in _abi.KERNELS.values()
    with pytest.raises(ValueError, match="Unknown kernel type 'sigmoid'"):
        pm.Parameter("sigmoid")


def test_create_accepts_id_4_and_still_rejects_3():
    """plssvm_mi_create checks the kernel id before it looks for a device: without one, an accepted id ends in
    ERR_NODEV (or succeeds where a device is present), a rejected one in ERR_UNSUPPORTED either way."""
    L = _abi.lib()
    for rb in (4, 8):
        ctx = ctypes.c_void_p()
        rc = L.plssvm_mi_create(rb, 4, 3, 0.5, 0.0, 1.0, 0, ctypes.byref(ctx))
        assert rc in (0, -7), rc  # OK or PLSSVM_MI_ERR_NODEV: not refused for its id
        if rc == 0:
            L.plssvm_mi_destroy(ctx)
        for bad in (3, 5, -1):
            ctx = ctypes.c_void_p()
            assert L.plssvm_mi_create(rb, bad, 3, 0.5, 0.0, 1.0, 0, ctypes.byref(ctx)) == -5  # PLSSVM_MI_ERR_UNSUPPORTED
            assert not ctx.value
    # degree and coef0 mean nothing to this kernel: a negative degree is the polynomial kernel's error alone
    ctx = ctypes.c_void_p()
    rc = L.plssvm_mi_create(8, 4, -1, 0.5, 7.0, 1.0, 0, ctypes.byref(ctx))
    assert rc in (0, -7), rc
    if rc == 0:
        L.plssvm_mi_destroy(ctx)


@pytest.mark.parametrize("name", ["laplacian", "4"])
@pytest.mark.parametrize("tname", ["float", "double"])
def test_two_class_model_file(parse_driver, tname, name, tmp_path):
    dt = DTYPES[tname]
    path = tmp_path / "two.model"
    path.write_text(TWO_CLASS.format(kernel=name))
    m = pio.parse_model(str(path), dtype=dt)
    assert m["kernel"] == "laplacian" and dt(m["gamma"]) == dt(0.125) and dt(m["rho"]) == dt(0.25)
    np.testing.assert_array_equal(m["alpha"], np.array([0.5, -1.5, 1.0], dtype=dt))
    np.testing.assert_array_equal(m["SV"], np.array([[1, 0, -0.25], [0, 0.5, 0], [-0.75, 0, 2]], dtype=dt))
    # the C++ reader, through tests/test_parsers.py's driver
    out = subprocess.run([parse_driver, "model", tname, str(path)], capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert lines[0].split()[0] != "ERROR", lines[0]
    kern = next(ln.split() for ln in lines if ln.startswith("KERNEL "))
    assert kern[1] == "laplacian" and dt(float(kern[3])) == dt(0.125)
    rho = next(ln.split() for ln in lines if ln.startswith("RHO "))
    assert dt(float(rho[1])) == dt(0.25)


@pytest.mark.parametrize("tname", ["float", "double"])
def test_one_vs_all_model_round_trip_and_cpp_writer(multi_driver, tname, tmp_path):
    dt = DTYPES[tname]
    rng = np.random.default_rng(7)
    n, d, K = 11, 5, 3
    X = rng.standard_normal((n, d)).astype(dt)
    X[:, d - 1] = np.where(np.arange(n) == 0, 1.0, X[:, d - 1])  # the last feature is present: d survives the file
    classes = np.array([-1.0, 0.5, 4.0], dtype=dt)
    labels = classes[np.arange(n) % K]
    p = pm.Parameter("laplacian", gamma=float(dt(1.0 / 3.0)), real_type=dt)
    p.data, p.labels = X, labels
    A = rng.standard_normal((K, n)).astype(dt)
    b = rng.standard_normal(K).astype(dt)
    path = str(tmp_path / "ova.model")
    pio.write_model(path, p, classes, A, b)
    head = open(path).read().split("SV\n")[0].splitlines()
    assert head[:3] == ["svm_type c_svc", "kernel_type laplacian", "gamma " + pio.shortest(dt(1.0 / 3.0), dt)]
    m = pio.parse_model(path, dtype=dt)
    order = np.argsort(np.searchsorted(classes, labels), kind="stable")
    assert m["kernel"] == "laplacian" and dt(m["gamma"]) == dt(1.0 / 3.0)
    np.testing.assert_array_equal(m["labels"], classes)
    np.testing.assert_array_equal(m["rho"], -b)
    np.testing.assert_array_equal(m["alpha"], A[:, order])
    # the C++ reader sees the same model, and the C++ writer emits the same bytes
    out = subprocess.run([multi_driver, "parse", tname, path], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split()[:2] == ["OK", "3"], out[0]
    kern = out[4].split()
    assert kern[1] == "laplacian" and dt(float(kern[3])) == dt(1.0 / 3.0)
    again = str(tmp_path / "cpp.model")
    subprocess.run([multi_driver, "rewrite", tname, path, again], check=True)
    assert open(again, "rb").read() == open(path, "rb").read()


def test_sigmoid_stays_unrecognised_in_model_files(tmp_path):
    path = tmp_path / "s.model"
    for name in ("sigmoid", "3"):
        path.write_text(TWO_CLASS.format(kernel=name))
        with pytest.raises(pio.InvalidFileFormat, match=f"Unrecognized kernel type '{name}'!"):
            pio.parse_model(str(path))


def test_train_help_lists_the_kernel_and_sparse_is_refused(tmp_path):
    out = subprocess.run([TRAIN, "--help"], capture_output=True, text=True, check=True).stdout
    assert "4 -- laplacian: exp(-gamma*|u-v|_1)" in out
    # refused from the options alone: the training file does not even exist
    for flag in ("4", "laplacian"):
        r = subprocess.run([TRAIN, "-t", flag, "--sparse", str(tmp_path / "missing.libsvm")], capture_output=True, text=True)
        assert r.returncode == 1 and "dense" in r.stderr and "--sparse" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([TRAIN, "-t", "sigmoid", str(tmp_path / "missing.libsvm")], capture_output=True, text=True)
    assert r.returncode != 0 and "Unrecognized kernel type 'sigmoid'!" in r.stderr


@pytest.mark.parametrize("form", ["csr", "coo"])
def test_csvm_refuses_sparse_data(form):
    p = pm.Parameter("laplacian", gamma=0.5)
    rowptr = np.array([0, 1, 2, 3], dtype=np.int64)
    col = np.array([0, 1, 0], dtype=np.int32)
    val = np.array([1.0, 2.0, 3.0])
    if form == "csr":
        p.csr = (rowptr, col, val, 3, 2)
    else:
        p.coo = (np.array([0, 1, 2], dtype=np.int64), col, val, 3, 2)
    p.labels = np.array([1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="Laplacian kernel takes dense data"):  # before plssvm_mi_create: no device needed
        pm.CSVM(p)
