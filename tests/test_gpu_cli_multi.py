"""plssvm-train --multiclass and plssvm-predict on one-vs-all models, on the GPU: the CLIs go through
plssvm::mi355x::csvm<T>::learn_multi / predict_label_multi, i.e. the same library calls as CSVM.learn_multi /
predict_values_multi, so a model file equals the Python result value for value (the shortest form round-trips) and the
C++ writer's file equals io.write_model's byte for byte. Without --multiclass nothing changes: the binary model of
5x4.libsvm is the file written before the flag existed (tests/golden/multiclass/5x4.libsvm.binary[.sparse].model, the
output of plssvm-train [--sparse] of the commit before this one on an MI355X)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, fixture_path
import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import datagen
from plssvm_sparse_fp22_amd import io as pio

pytestmark = pytest.mark.gpu

TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")
PRED = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-predict")


def write_libsvm(path, X, labels):
    with open(path, "w") as f:
        for x, y in zip(X, labels):
            f.write(pio.shortest(y, np.float64) + " " + " ".join(f"{k}:{float(v)!r}" for k, v in enumerate(x) if v != 0) + "\n")


def three_class_file(path):
    """150 x 4, three blobs with the labels 0, 1 and 2.5"""
    rng = np.random.default_rng(101)
    centres = np.array([[1.0, 0.0, -1.0, 0.5], [-1.0, 1.0, 0.0, -0.5], [0.0, -1.0, 1.0, 1.0]])
    cls = rng.permutation(np.arange(150) % 3)
    X = np.round(centres[cls] + 0.4 * rng.standard_normal((150, 4)), 6)
    write_libsvm(path, X, np.array([0.0, 1.0, 2.5])[cls])


def five_class_sparse_file(path):
    """300 x 64 at 8 entries per row, five classes"""
    csr, _ = datagen.sparse_csr(300, 64, 8, seed=102, dtype=np.float64)
    X = np.round(datagen.densify(csr), 6)
    X[:, 63] = np.where(np.arange(300) == 0, 0.5, X[:, 63])  # the last feature is present
    cls = np.random.default_rng(103).permutation(np.arange(300) % 5)
    write_libsvm(path, X, np.array([-2.0, -1.0, 0.0, 3.0, 7.0])[cls])


def learn_multi(path, dtype, sparse):
    p = pm.Parameter("rbf", real_type=dtype).parse_train_file(str(path), sparse=sparse, multiclass=True)
    svm = pm.CSVM(p)
    svm.learn_multi()
    return p, svm


# (extra flags, real type, sparse)
VARIANTS = {"dense": ([], np.float64, False), "sparse": (["--sparse"], np.float64, True),
            "single": (["--single"], np.float32, False), "two-ranks": (["--devices", "0,0"], np.float64, False)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("data", ["three", "five"])
def test_train_multiclass_reproduces_learn_multi(tmp_path, data, variant):
    extra, dtype, sparse = VARIANTS[variant]
    src, model = tmp_path / "train.libsvm", tmp_path / "train.model"
    (three_class_file if data == "three" else five_class_sparse_file)(src)
    r = subprocess.run([TRAIN, "--multiclass", "-t", "2", *extra, str(src), str(model)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p, svm = learn_multi(src, dtype, sparse)
    with svm:
        m = pio.parse_model(str(model), dtype=dtype)
        K = svm.classes.size
        assert K == (3 if data == "three" else 5)
        cls = np.searchsorted(svm.classes, p.labels)
        order = np.argsort(cls, kind="stable")
        text = open(model).read()
        assert f"\nnr_class {K}\nlabel " + " ".join(pio.shortest(c, dtype) for c in svm.classes) + "\n" in text
        assert list(m["nr_sv"]) == list(np.bincount(cls, minlength=K))
        np.testing.assert_array_equal(m["labels"], svm.classes)
        print(f"{data} {variant}: max |rho + bias| {np.abs(m['rho'] + svm.biases).max():.3e}, "
              f"max |alpha diff| {np.abs(m['alpha'] - svm.alphas[:, order]).max():.3e}")
        np.testing.assert_array_equal(m["rho"], -svm.biases)
        np.testing.assert_array_equal(m["alpha"], svm.alphas[:, order])
        # one summary line per class instead of the per-iteration lines
        assert "Start Iteration" not in r.stdout
        for k, c in enumerate(svm.classes):
            assert f"Class {pio.shortest(c, dtype)}: finished after {svm.iters_multi[k]} iterations" in r.stdout
        # the C++ writer's file is io.write_model's, byte for byte
        py = tmp_path / "py.model"
        pio.write_model(str(py), p, svm.classes, svm.alphas, svm.biases)
        assert open(py, "rb").read() == open(model, "rb").read()


@pytest.mark.parametrize("extra", [[], ["--sparse"], ["--single"]])
@pytest.mark.parametrize("data", ["three", "five"])
def test_predict_writes_predict_multis_labels(tmp_path, data, extra):
    dtype = np.float32 if "--single" in extra else np.float64
    src, model, out = tmp_path / "train.libsvm", tmp_path / "train.model", tmp_path / "train.predict"
    (three_class_file if data == "three" else five_class_sparse_file)(src)
    subprocess.run([TRAIN, "-q", "--multiclass", "-t", "2", *extra, str(src), str(model)], check=True)
    r = subprocess.run([PRED, *extra, str(src), str(model), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the same route in Python: the model's support vectors as the context's data, all classes in one call
    m = pio.parse_model(str(model), dtype=dtype)
    sparse = "--sparse" in extra
    Z, y = pio.parse_libsvm(str(src), dtype=dtype, sparse=sparse, multiclass=True)
    p = pm.Parameter("rbf", gamma=m["gamma"], real_type=dtype)
    if sparse:
        SV = m["SV"]
        rowptr = np.concatenate([[0], np.cumsum((SV != 0).sum(axis=1))]).astype(np.int64)
        rr, cc = np.nonzero(SV)
        p.csr = (rowptr, cc.astype(np.int32), SV[rr, cc], SV.shape[0], SV.shape[1])
    else:
        p.data = m["SV"]
    with pm.CSVM(p) as svm:
        svm.classes, svm.alphas, svm.biases = m["labels"], m["alpha"], -m["rho"]
        want = svm.predict_multi(Z)
    got = open(out).read()
    assert not got.endswith("\n")
    assert got.split("\n") == [pio.shortest(v, dtype) for v in want]
    correct = int(np.sum(want == y))
    acc = pio.shortest(dtype(correct) / dtype(len(y)) * dtype(100), dtype)
    assert f"Accuracy = {acc}% ({correct}/{len(y)}) (classification)" in r.stdout
    assert set(want) <= set(m["labels"])
    if data == "three":  # blobs of sigma 0.4 whose centres lie more than 1.9 apart: nearly all points are recovered
        assert correct > 0.9 * len(y)


@pytest.mark.parametrize("extra", [[], ["--sparse"]])
def test_binary_model_is_unchanged(tmp_path, extra):
    out = tmp_path / "5x4.model"
    subprocess.run([TRAIN, "-q", *extra, fixture_path("5x4.libsvm"), str(out)], check=True)
    want = os.path.join(ROOT, "tests", "golden", "multiclass", "5x4.libsvm.binary.sparse.model" if extra else "5x4.libsvm.binary.model")
    assert open(out, "rb").read() == open(want, "rb").read()
