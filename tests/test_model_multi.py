"""One-vs-all model files (nr_class >= 3; build-defined, the reference is binary only) in both readers and both
writers, and the --multiclass flag of plssvm-train up to the point where a GPU is needed. CPU only.

* tests/golden/multiclass/3class.model (hand-written) parses to the expected labels, rhos, alphas and support vectors in
  the Python reader (io.parse_model) and in the C++ reader (parameter<T>::parse_model_file through
  tests/cpp/model_multi_driver.cpp, compiled here with g++);
* every malformed variant raises the same message in both readers;
* io.write_model -> io.parse_model round-trips exactly, the C++ writer's text equals io.write_model's bytes, and
  io.shortest equals std::to_chars; two classes are refused (they are a binary model);
* the reference's binary fixtures parse as before;
* parse_libsvm / parse_train_file with multiclass keep the label values;
* plssvm-train --help lists --multiclass, and --multiclass on a two-label file exits 1 before any GPU work.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, fixture_path
import plssvm_sparse_fp22_amd as pm
from plssvm_sparse_fp22_amd import io as pio

DTYPES = {"float": np.float32, "double": np.float64}
FIXTURE = os.path.join(ROOT, "tests", "golden", "multiclass", "3class.model")
TRAIN = os.path.join(ROOT, "plssvm_sparse_fp22_amd", "bin", "plssvm-train")

LABELS = [0.0, 1.0, 2.5]
RHO = ["0.125", "-0.5", "0.001"]
NR_SV = [2, 1, 3]
ALPHA = [["0.5", "-1.5", "0.25", "0.375", "1e-05", "0.375"],
         ["-0.25", "0.75", "1", "-2", "0.5", "-0.5"],
         ["-0.125", "0.0625", "-0.03125", "1.5", "-1", "-0.40625"]]
SV = [["1", "0", "0", "-0.25"], ["0", "0.5", "0.125", "0"], ["-0.75", "0", "0", "0"], ["0", "0", "2", "1"],
      ["0.1", "0.2", "0.3", "0.4"], ["0", "0", "0", "0"]]


def as_type(rows, dt):
    return np.array([[dt(float(v)) for v in r] for r in rows], dtype=dt)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("drv") / "model_multi_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "plssvm_sparse_fp22_amd", "host"),
                    os.path.join(ROOT, "tests", "cpp", "model_multi_driver.cpp"), "-o", exe], check=True)
    return exe


class ParseError(Exception):
    def __init__(self, kind, msg):
        super().__init__(f"{kind}: {msg}")
        self.kind, self.msg = kind, msg


def read_cpp(driver, tname, path):
    out = subprocess.run([driver, "parse", tname, path], capture_output=True, text=True, check=True).stdout.splitlines()
    if out[0].startswith("ERROR "):
        kind, msg = out[0][len("ERROR "):].split(": ", 1)
        raise ParseError(kind, msg)
    dt = DTYPES[tname]
    K, n, d = (int(v) for v in out[0].split()[1:])
    rows = np.array([[float(v) for v in ln.split()] for ln in out[5:5 + n]]).reshape(n, K + d)
    kern = out[4].split()
    return dict(labels=np.array(out[1].split()[1:], dtype=float).astype(dt), rho=np.array(out[2].split()[1:], dtype=float).astype(dt),
                nr_sv=[int(v) for v in out[3].split()[1:]], kernel=kern[1], gamma=float(kern[3]),
                alpha=rows[:, :K].T.astype(dt), SV=rows[:, K:].astype(dt))


def read_py(_driver, tname, path):
    try:
        return pio.parse_model(path, dtype=DTYPES[tname])
    except pio.InvalidFileFormat as e:
        raise ParseError("invalid_file_format", str(e)) from None


READERS = {"cpp": read_cpp, "python": read_py}


@pytest.mark.parametrize("tname", ["float", "double"])
@pytest.mark.parametrize("reader", list(READERS))
def test_fixture_parses(driver, reader, tname):
    dt = DTYPES[tname]
    m = READERS[reader](driver, tname, FIXTURE)
    np.testing.assert_array_equal(m["labels"], np.array(LABELS, dtype=dt))
    np.testing.assert_array_equal(m["rho"], np.array([dt(float(v)) for v in RHO], dtype=dt))
    np.testing.assert_array_equal(m["alpha"], as_type(ALPHA, dt))
    np.testing.assert_array_equal(m["SV"], as_type(SV, dt))
    assert m["alpha"].shape == (3, 6) and m["alpha"].dtype == dt
    assert list(m["nr_sv"]) == NR_SV and m["kernel"] == "rbf" and m["gamma"] == 0.25


# (original, altered, message)
MALFORMED = [
    ("nr_class 3", "nr_class 1", "The number of classes must be at least 2, but is 1!"),
    ("nr_class 3", "nr_class 0", "The number of classes must be at least 2, but is 0!"),
    ("nr_class 3", "nr_class 4", "Can only use 3 classes, but 4 were given!"),
    ("label 0 1 2.5", "label 0 1", "Can only use 2 classes, but 3 were given!"),
    ("rho 0.125 -0.5 0.001", "rho 0.125 -0.5", "The number of rho values must match the number of classes, but 2 != 3!"),
    ("nr_sv 2 1 3", "nr_sv 2 1 2 1",
     "The number of support vector counts must match the number of classes, but 4 != 3!"),
    ("label 0 1 2.5", "label 0 1 1", "The labels must be distinct, but 'label 0 1 1' were given!"),
    ("label 0 1 2.5", "label 0 1 inf", "The labels must be finite, but 'label 0 1 inf' were given!"),
    ("label 0 1 2.5", "label 0 nan 2.5", "The labels must be finite, but 'label 0 nan 2.5' were given!"),
    ("0.25 1 -0.03125 0:", "0.25 1 0:", "Every support vector needs 3 alpha values, but support vector 3 has 2!"),
    ("0.375 -0.5 -0.40625 ", "0.375 ", "Every support vector needs 3 alpha values, but support vector 6 has 1!"),
    ("nr_sv 2 1 3", "nr_sv 2 1 4",
     "The number of support vectors per class doesn't add up to the total number: 2 + 1 + 4 != 6!"),
    ("total_sv 6", "total_sv 7",
     "The number of support vectors per class doesn't add up to the total number: 2 + 1 + 3 != 7!"),
    ("label 0 1 2.5\n", "", "Missing labels!"),
    ("rho 0.125 -0.5 0.001\n", "", "Missing rho value!"),
    ("nr_sv 2 1 3\n", "", "Missing number of support vectors per class!"),
    ("SV", "SV_wrong", "Unrecognized header entry 'SV_wrong'! Maybe SV is missing?"),
]


@pytest.mark.parametrize("tname", ["float", "double"])
@pytest.mark.parametrize("reader", list(READERS))
@pytest.mark.parametrize("case", range(len(MALFORMED)))
def test_malformed(driver, reader, tname, case, tmp_path):
    correct, altered, msg = MALFORMED[case]
    text = open(FIXTURE).read()
    assert text.count(correct) == 1
    path = tmp_path / "bad.model"
    path.write_text(text.replace(correct, altered))
    with pytest.raises(ParseError) as e:
        READERS[reader](driver, tname, str(path))
    assert e.value.kind == "invalid_file_format"
    assert e.value.msg == msg


def _random_model(dtype, kernel, sparse, seed):
    rng = np.random.default_rng(seed)
    n, d, K = 23, 7, 4
    X = (rng.standard_normal((n, d)) * 10.0 ** rng.integers(-6, 6, size=(n, d))).astype(dtype)
    X[rng.random((n, d)) < 0.4] = 0
    X[5] = 0  # a support vector without features
    X[:, d - 1] = np.where(np.arange(n) == 0, 1.0, X[:, d - 1])  # the last feature is present: d survives the file
    classes = np.array([-3.0, 0.5, 2.0, 1e6], dtype=dtype)
    labels = classes[rng.integers(0, K, size=n)]
    labels[:K] = classes
    p = pm.Parameter(kernel, degree=2, gamma=float(dtype(1.0 / 3.0)), coef0=float(dtype(0.1)), real_type=dtype)
    if sparse:
        rowptr = np.concatenate([[0], np.cumsum((X != 0).sum(axis=1))]).astype(np.int64)
        rr, cc = np.nonzero(X)
        p.csr = (rowptr, cc.astype(np.int32), X[rr, cc], n, d)
    else:
        p.data = X
    p.labels = labels
    A = (rng.standard_normal((K, n)) * 10.0 ** rng.integers(-8, 8, size=(K, n))).astype(dtype)
    b = rng.standard_normal(K).astype(dtype)
    return p, X, classes, labels, A, b


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("kernel", ["linear", "polynomial", "rbf"])
@pytest.mark.parametrize("tname", ["float", "double"])
def test_write_model_round_trips_and_equals_the_cpp_writer(driver, tname, kernel, sparse, tmp_path):
    dt = DTYPES[tname]
    p, X, classes, labels, A, b = _random_model(dt, kernel, sparse, seed=5)
    path = str(tmp_path / "w.model")
    pio.write_model(path, p, classes, A, b)
    m = pio.parse_model(path, dtype=dt)
    order = np.argsort(np.searchsorted(classes, labels), kind="stable")  # grouped by class, file order inside
    np.testing.assert_array_equal(m["labels"], classes)
    np.testing.assert_array_equal(m["rho"], -b)
    np.testing.assert_array_equal(m["alpha"], A[:, order])
    # features are written with 7 significant digits ("%e"), like the binary writer's
    np.testing.assert_array_equal(m["SV"], np.array([[dt(float("%e" % float(v))) for v in r] for r in X[order]], dtype=dt))
    assert list(m["nr_sv"]) == list(np.bincount(np.searchsorted(classes, labels), minlength=4))
    assert m["kernel"] == kernel
    if kernel != "linear":
        assert dt(m["gamma"]) == dt(1.0 / 3.0)
    head = open(path).read().split("SV\n")[0].splitlines()
    assert head[-4].startswith("label -3 0.5 2 1e+06") and head[-5] == "nr_class 4" and head[-3] == "total_sv 23"
    # the C++ writer: parse and write again -> the same bytes
    out = str(tmp_path / "cpp.model")
    subprocess.run([driver, "rewrite", tname, path, out], check=True)
    assert open(out, "rb").read() == open(path, "rb").read()
    # the C++ reader reads what the Python reader reads
    c = read_cpp(driver, tname, path)
    for key in ("labels", "rho", "alpha", "SV"):
        np.testing.assert_array_equal(c[key], m[key])


def test_fixture_is_what_the_writers_write(driver, tmp_path):
    out = str(tmp_path / "re.model")
    subprocess.run([driver, "rewrite", "double", FIXTURE, out], check=True)
    want = "".join(ln for ln in open(FIXTURE).readlines() if not ln.startswith("#"))
    assert open(out).read() == want


def test_write_model_refuses_two_classes(tmp_path):
    p = pm.Parameter("linear")
    p.data = np.eye(4)
    p.labels = np.array([1.0, -1.0, 1.0, -1.0])
    with pytest.raises(ValueError, match="at least 3 classes, but 2 were given"):
        pio.write_model(str(tmp_path / "x.model"), p, np.array([-1.0, 1.0]), np.zeros((2, 4)), np.zeros(2))
    assert not os.path.exists(tmp_path / "x.model")


@pytest.mark.parametrize("name", ["5x4.libsvm.model", "5x4.libsvm.polynomial.model", "5x4.libsvm.rbf.model",
                                  "500x200.libsvm.rbf.model"])
def test_binary_fixtures_parse_as_before(driver, name):
    m = pio.parse_model(fixture_path(name))
    assert m["alpha"].ndim == 1 and m["alpha"].shape[0] == m["SV"].shape[0]
    assert isinstance(m["rho"], float) and m["labels"] == (1.0, -1.0) and len(m["nr_sv"]) == 2
    out = subprocess.run([driver, "parse", "double", fixture_path(name)], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["BINARY", str(m["SV"].shape[0]), str(m["SV"].shape[1])]


def test_multiclass_keeps_the_label_values(driver, tmp_path):
    path = tmp_path / "m.libsvm"
    path.write_text("2.5 0:1 3:2\n0 1:1\n-1 0:0.5\n2.5 2:1\n1e3 3:1\n")
    for sparse in (False, True):
        _, y = pio.parse_libsvm(str(path), sparse=sparse, multiclass=True)
        np.testing.assert_array_equal(y, [2.5, 0.0, -1.0, 2.5, 1000.0])
        _, y = pio.parse_libsvm(str(path), sparse=sparse)
        np.testing.assert_array_equal(y, [1, -1, -1, 1, 1])
    p = pm.Parameter("linear").parse_train_file(str(path), multiclass=True)
    np.testing.assert_array_equal(p.labels, [2.5, 0.0, -1.0, 2.5, 1000.0])
    out = subprocess.run([driver, "labels", "double", str(path)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["LABELS 2.5 0 -1 2.5 1000", "SIGNS 1 -1 -1 1 1"]


def test_shortest_is_to_chars():
    cases = {np.float64: [(1e-5, "1e-05"), (1e-4, "1e-04"), (1e-3, "0.001"), (1e5, "1e+05"), (123456.0, "123456"),
                          (1 / 3, "0.3333333333333333"), (2.5, "2.5"), (0.0, "0"), (-0.0, "-0"), (1e22, "1e+22"),
                          (123456789012345678.0, "123456789012345680"), (-7e-7, "-7e-07")],
             np.float32: [(1 / 3, "0.33333334"), (123456789.125, "123456792"), (1e-5, "1e-05"), (16777218.0, "16777218")]}
    for dt, rows in cases.items():
        for v, want in rows:
            assert pio.shortest(v, dt) == want, (dt, v)


def test_train_help_lists_multiclass():
    out = subprocess.run([TRAIN, "--help"], capture_output=True, text=True, check=True).stdout
    assert "--multiclass" in out


def test_multiclass_needs_three_labels(tmp_path):
    r = subprocess.run([TRAIN, "--multiclass", fixture_path("5x4.libsvm"), str(tmp_path / "m.model")], capture_output=True,
                       text=True)
    assert r.returncode == 1
    assert r.stderr.strip() == ("--multiclass needs at least 3 distinct labels, but 2 were given! "
                                "Train without it for two classes.")
    assert not os.path.exists(tmp_path / "m.model")
