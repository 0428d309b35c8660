"""CPU test of the gamma-lane predict entry point: the header declares it with the documented signature and the ctypes
binding carries it with its 11 arguments."""
import os
import re

from conftest import ROOT


def test_header_and_binding_agree():
    from plssvm_sparse_fp22_amd import _abi

    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "plssvm_mi355x.h")).read())
    assert ("PLSSVM_MI_API int plssvm_mi_predict_gammas_dense(plssvm_mi_ctx *ctx, const double *gammas, const void *ALPHA, "
            "int64_t nlane, int64_t lda, const double *bias, const void *Z, int64_t np, int64_t d, void *OUT, int64_t ldo);") in txt
    assert "plssvm_mi_predict_gammas_dense" in _abi.EXPORTS
    fn = _abi.lib().plssvm_mi_predict_gammas_dense
    assert len(fn.argtypes) == 11 and fn(None, None, None, 0, 0, None, None, 0, 0, None, 0) == -1  # ERR_ARG, no GPU needed
