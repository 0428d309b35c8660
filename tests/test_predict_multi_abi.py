"""CPU test of the multi-class predict boundary: include/plssvm_mi355x.h declares plssvm_mi_predict_multi_dense / _csr
and the PLSSVM_MI_PREDICT_* constants, and _abi.py carries the same values and signatures."""
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "plssvm_mi355x.h")
NAMES = ("NONE", "LINEAR", "GEMM", "TILES", "EXPANSION", "BRUTE")


def _defines():
    txt = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+PLSSVM_MI_PREDICT_(\w+)\s+(\d+)", txt)}


def test_header_declares_the_entry_points():
    txt = re.sub(r"\s+", " ", open(HEADER).read())
    assert re.search(r"PLSSVM_MI_API int plssvm_mi_predict_multi_dense\(plssvm_mi_ctx \*ctx, const void \*ALPHA, "
                     r"int64_t nclass, int64_t lda, const double \*bias, const void \*Z, int64_t np, int64_t d, "
                     r"void \*OUT, int64_t ldo\);", txt)
    assert re.search(r"PLSSVM_MI_API int plssvm_mi_predict_multi_csr\(plssvm_mi_ctx \*ctx, const void \*ALPHA, "
                     r"int64_t nclass, int64_t lda, const double \*bias, const int64_t \*rowptr, const int32_t \*col, "
                     r"const void \*val, int val_fmt, int64_t np, int64_t d, void \*OUT, int64_t ldo\);", txt)
    assert re.search(r"int predict_algo;[^}]*\} plssvm_mi_info;", txt)  # the struct's last field but one


def test_constants_match_the_binding():
    from plssvm_sparse_fp22_amd import _abi

    got = _defines()
    assert [got[k] for k in NAMES] == [0, 1, 2, 3, 4, 5]
    for k in NAMES:
        assert getattr(_abi, "PREDICT_" + k) == got[k], k
    assert _abi.PREDICT_SEG_TILES == got["SEG_TILES"]
    assert [f[0] for f in _abi.Info._fields_[-2:]] == ["predict_algo", "rbf_shift"]  # appended after it, same offset


def test_library_exports_the_entry_points():
    from plssvm_sparse_fp22_amd import _abi

    L = _abi.lib()
    for name, nargs in (("plssvm_mi_predict_multi_dense", 10), ("plssvm_mi_predict_multi_csr", 13)):
        assert name in _abi.EXPORTS
        assert len(getattr(L, name).argtypes) == nargs
