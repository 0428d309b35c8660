"""plssvm-train -t 4 / -t laplacian and plssvm-predict on the GPU: the CLIs go through the same library calls as the
Python API, so the labels they predict are the Python API's on the same data, the model file names the kernel, and
plssvm-predict recognises it by itself."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import io as pio

pytestmark = pytest.mark.gpu

TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")
PRED = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-predict")


def write_libsvm(path, X, labels):
    with open(path, "w") as f:
        for x, y in zip(X, labels):
            f.write(pio.shortest(y, np.float64) + " " + " ".join(f"{k}:{float(v)!r}" for k, v in enumerate(x) if v != 0) + "\n")


def blob_file(path, classes, seed):
    """150 x 6 count-like features around one centre per class"""
    rng = np.random.default_rng(seed)
    K = len(classes)
    centres = rng.uniform(0.0, 4.0, size=(K, 6))
    cls = rng.permutation(np.arange(150) % K)
    X = np.round(np.abs(centres[cls] + 0.5 * rng.standard_normal((150, 6))), 6)
    X[:, 5] = np.where(np.arange(150) == 0, 0.5, X[:, 5])  # the last feature is present
    write_libsvm(path, X, np.asarray(classes)[cls])


def read_labels(path):
    return np.array([float(ln) for ln in open(path).read().split()])


def test_train_and_predict_two_classes(tmp_path):
    src, model, out = tmp_path / "train.libsvm", tmp_path / "train.model", tmp_path / "train.predict"
    blob_file(src, [1.0, -1.0], seed=201)
    r = subprocess.run([TRAIN, "-t", "4", "-e", "1e-6", str(src), str(model)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "kernel type: laplacian -> exp(-gamma*|u-v|_1)" in r.stdout
    head = open(model).read().split("SV\n")[0].splitlines()
    assert head[0] == "svm_type c_svc" and head[1] == "kernel_type laplacian" and head[2].startswith("gamma ")
    m = pio.parse_model(str(model))
    assert m["kernel"] == "laplacian" and m["gamma"] == 1.0 / 6
    r = subprocess.run([PRED, str(src), str(model), str(out)], capture_output=True, text=True)  # no kernel option
    assert r.returncode == 0, r.stderr
    assert "kernel type: laplacian" in r.stdout
    p = pm.Parameter("laplacian", epsilon=1e-6).parse_train_file(str(src))
    with pm.CSVM(p) as svm:
        svm.learn()
        want = svm.predict(p.data)
        acc = svm.accuracy()
    got = read_labels(out)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert acc > 0.9  # separable blobs: the model is not degenerate


def test_train_and_predict_multiclass(tmp_path):
    src, model, out = tmp_path / "three.libsvm", tmp_path / "three.model", tmp_path / "three.predict"
    blob_file(src, [0.0, 1.0, 2.5], seed=202)
    r = subprocess.run([TRAIN, "--multiclass", "-t", "laplacian", "-q", str(src), str(model)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(model).read()
    assert text.startswith("svm_type c_svc\nkernel_type laplacian\ngamma ") and "\nnr_class 3\nlabel 0 1 2.5\n" in text
    r = subprocess.run([PRED, "-q", str(src), str(model), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = pm.Parameter("laplacian").parse_train_file(str(src), multiclass=True)
    with pm.CSVM(p) as svm:
        svm.learn_multi()
        want = svm.predict_multi(p.data)
    got = read_labels(out)
    assert np.array_equal(got, want)
    assert np.mean(got == p.labels) > 0.9


def test_sparse_is_refused_by_both_tools(tmp_path):
    src, model = tmp_path / "train.libsvm", tmp_path / "train.model"
    blob_file(src, [1.0, -1.0], seed=203)
    r = subprocess.run([TRAIN, "-t", "4", "--sparse", str(src), str(model)], capture_output=True, text=True)
    assert r.returncode == 1 and "--sparse" in r.stderr and not model.exists()
    subprocess.run([TRAIN, "-t", "4", "-q", str(src), str(model)], check=True)
    r = subprocess.run([PRED, "--sparse", str(src), str(model), str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 1 and "--sparse" in r.stderr
