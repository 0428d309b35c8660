"""ctypes binding of libplssvm_mi355x.so (C ABI: include/plssvm_mi355x.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (``make -C
plssvm_sparse_fp22_amd/csrc``). There is no fallback: if the library is missing or cannot be
loaded, :func:`lib` raises, so nothing silently runs on the CPU.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PLSSVM_MI_LIB: an alternative build of the same library (A/B measurements of compile-time variants,
# tools/variants.sh); never a CPU stand-in — every build behind this name is the gfx950 HIP path
LIB_PATH = os.environ.get("PLSSVM_MI_LIB") or os.path.join(_HERE, "libplssvm_mi355x.so")

OK = 0
ERR = {-1: "ERR_ARG", -2: "ERR_HIP", -3: "ERR_RCCL", -4: "ERR_OOM", -5: "ERR_UNSUPPORTED", -6: "ERR_STATE",
       -7: "ERR_NODEV"}
KERNELS = {"linear": 0, "polynomial": 1, "poly": 1, "rbf": 2, "laplacian": 4}  # 3 (upstream's sigmoid) is not offered
VAL_REAL, VAL_FP22 = 0, 1
KP_AUTO, KP_PAIRWISE, KP_FACTORED = 0, 1, 2
OPT_KP_MODE = 1
UNIQUE_ID_BYTES = 128

# every symbol include/plssvm_mi355x.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "plssvm_mi_device_count", "plssvm_mi_create", "plssvm_mi_destroy", "plssvm_mi_last_error",
    "plssvm_mi_set_option", "plssvm_mi_set_cost", "plssvm_mi_set_qa_cost", "plssvm_mi_get_unique_id",
    "plssvm_mi_comm_init", "plssvm_mi_setup_dense", "plssvm_mi_setup_csr", "plssvm_mi_generate_q", "plssvm_mi_kp",
    "plssvm_mi_solve_cg", "plssvm_mi_cg_begin", "plssvm_mi_cg_step", "plssvm_mi_cg_result", "plssvm_mi_learn",
    "plssvm_mi_time_kp", "plssvm_mi_get_info", "plssvm_mi_partition",
    "plssvm_mi_update_w", "plssvm_mi_predict_dense", "plssvm_mi_predict_csr", "plssvm_mi_setup_coo",
    "plssvm_mi_comm_init_host", "plssvm_mi_kp_part", "plssvm_mi_set_progress", "plssvm_mi_comm_abort",
    "plssvm_mi_kp_multi", "plssvm_mi_solve_cg_multi", "plssvm_mi_learn_multi", "plssvm_mi_time_kp_multi",
    "plssvm_mi_predict_multi_dense", "plssvm_mi_predict_multi_csr", "plssvm_mi_get_predict_stats",
    "plssvm_mi_get_kp_cache_narrow_tiles", "plssvm_mi_get_spmv_plan",
    "plssvm_mi_set_point_weights", "plssvm_mi_learn_lanes", "plssvm_mi_learn_held", "plssvm_mi_train_values",
)
# the one entry point a PLSSVM_MI_LIB build may lack (a build from before the narrow record form, loaded for an A/B
# run): CSVM.info() then reports kp_cache_narrow_tiles = 0, which is what such a build stores
OPTIONAL_EXPORTS = ("plssvm_mi_get_kp_cache_narrow_tiles",)
OPT_SIM_RANK = 2
OPT_RBF_FORM = 3
OPT_SPARSE_ALGO = 4
OPT_CG_VARIANT = 5
OPT_KP_CACHE = 6
OPT_MULTI_WIDTH = 7
OPT_KP_PACK = 8
SPARSE_AUTO, SPARSE_PATTERN, SPARSE_EXPANSION, SPARSE_DENSE, SPARSE_ONTHEFLY = 0, 1, 2, 3, 4
PART_KERNEL, PART_OVERLAP, PART_REMAINDER = 0, 1, 2
XCHG_ALLREDUCE, XCHG_ALLGATHER = 0, 1
# Info.predict_algo: the path of the last predict call (PLSSVM_MI_PREDICT_*)
PREDICT_NONE, PREDICT_LINEAR, PREDICT_GEMM, PREDICT_TILES, PREDICT_EXPANSION, PREDICT_BRUTE = 0, 1, 2, 3, 4, 5
PREDICT_SEG_TILES = 16  # support-vector tiles per workgroup segment of the fused predict kernel
# int fn(void *buf, int64_t count, int real_bytes, int op, void *user)   (plssvm_mi_exchange_fn)
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                               ctypes.c_void_p)
# void fn(int64_t first, int64_t count, const double *deltas, double target, double batch_ms, void *user)
PROGRESS_FN = ctypes.CFUNCTYPE(None, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_double), ctypes.c_double,
                               ctypes.c_double, ctypes.c_void_p)


class Info(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int64) for k in ("n", "d", "m", "n_pad", "d_pad", "nnz", "tiles_total", "tiles_local",
                                              "tile_rows", "tile_cols", "device_bytes", "pairs")] + \
               [(k, ctypes.c_int) for k in ("kp_mode", "rank", "world_size", "real_bytes", "kernel", "is_sparse",
                                            "val_fmt", "rbf_factored")] + [("pair_slots", ctypes.c_int64), ("spmv_bytes", ctypes.c_int64)] + \
               [("rbf_small_args", ctypes.c_int), ("sparse_algo", ctypes.c_int), ("exp_terms", ctypes.c_int),
                ("exp_waves", ctypes.c_int), ("exp_chunks", ctypes.c_int64), ("exp_hbytes", ctypes.c_int),
                ("exp_layout", ctypes.c_int), ("exp_dot2", ctypes.c_int), ("centered", ctypes.c_int),
                ("exp_lt", ctypes.c_int), ("kp_cache_tiles", ctypes.c_int64), ("kp_cache_bytes", ctypes.c_int64),
                ("multi_width", ctypes.c_int), ("kp_cache_packed_tiles", ctypes.c_int64),
                ("predict_algo", ctypes.c_int), ("rbf_shift", ctypes.c_int)]


class BackendError(RuntimeError):
    """plssvm::hip::backend_exception equivalent raised for a non-zero ABI return code."""

    def __init__(self, code, msg):
        super().__init__(f"{ERR.get(code, code)}: {msg}")
        self.code = code


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                              "(make -C plssvm_sparse_fp22_amd/csrc); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        _declare(L)
        _lib = L
    return _lib


def _declare(L):
    P, I64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    PP = ctypes.POINTER(ctypes.c_void_p)
    PD, PI64, PI = ctypes.POINTER(D), ctypes.POINTER(I64), ctypes.POINTER(I)
    sig = {
        "plssvm_mi_device_count": ([], I),
        "plssvm_mi_create": ([I, I, I, D, D, D, I, PP], I),
        "plssvm_mi_destroy": ([P], None),
        "plssvm_mi_last_error": ([P], ctypes.c_char_p),
        "plssvm_mi_set_option": ([P, I, I64], I),
        "plssvm_mi_set_cost": ([P, D], I),
        "plssvm_mi_set_qa_cost": ([P, D], I),
        "plssvm_mi_get_unique_id": ([P], I),
        "plssvm_mi_comm_init": ([P, I, I, P], I),
        "plssvm_mi_setup_dense": ([P, P, I64, I64], I),
        "plssvm_mi_setup_csr": ([P, P, P, P, I, I64, I64], I),
        "plssvm_mi_setup_coo": ([P, P, P, P, I, I64, I64, I64], I),
        "plssvm_mi_generate_q": ([P, P, PD], I),
        "plssvm_mi_kp": ([P, P, P, P, D], I),
        "plssvm_mi_solve_cg": ([P, P, P, I64, D, P, P, PI64], I),
        "plssvm_mi_cg_begin": ([P, P, P, D, PD], I),
        "plssvm_mi_cg_step": ([P, I64, I, PI64, PI], I),
        "plssvm_mi_cg_result": ([P, P, P, I64, PI64], I),
        "plssvm_mi_learn": ([P, P, I64, D, P, PD, P, PI64], I),
        "plssvm_mi_update_w": ([P, P, P], I),
        "plssvm_mi_predict_dense": ([P, P, D, P, I64, I64, P], I),
        "plssvm_mi_predict_csr": ([P, P, D, P, P, P, I, I64, I64, P], I),
        "plssvm_mi_time_kp": ([P, I, PD, PD], I),
        "plssvm_mi_get_info": ([P, ctypes.POINTER(Info)], I),
        "plssvm_mi_partition": ([I64, I, I, PI64], I),
        "plssvm_mi_comm_init_host": ([P, I, I, EXCHANGE_FN, P], I),
        "plssvm_mi_kp_part": ([P, P, P, I], I),
        "plssvm_mi_comm_abort": ([P], I),
        "plssvm_mi_set_progress": ([P, PROGRESS_FN, P], I),
        "plssvm_mi_kp_multi": ([P, P, P, P, I64, I64, D], I),
        "plssvm_mi_solve_cg_multi": ([P, P, I64, I64, P, I64, D, P, P, P], I),
        "plssvm_mi_learn_multi": ([P, P, I64, I64, I64, D, P, P, P, P], I),
        "plssvm_mi_time_kp_multi": ([P, I64, I, PD], I),
        "plssvm_mi_set_point_weights": ([P, P], I),
        "plssvm_mi_learn_lanes": ([P, P, I64, I64, P, P, I64, I64, D, P, P, P, P], I),
        "plssvm_mi_learn_held": ([P, P, I64, I64, P, P, I64, P, I64, I64, D, P, P, P, P, P], I),
        "plssvm_mi_train_values": ([P, P, I64, I64, P, P, I64], I),
        "plssvm_mi_predict_multi_dense": ([P, P, I64, I64, P, P, I64, I64, P, I64], I),
        "plssvm_mi_predict_multi_csr": ([P, P, I64, I64, P, P, P, P, I, I64, I64, P, I64], I),
        "plssvm_mi_get_predict_stats": ([P, PI64], I),
        "plssvm_mi_get_kp_cache_narrow_tiles": ([P, PI64], I),
        "plssvm_mi_get_spmv_plan": ([P, PI64], I),
    }
    for name, (args, res) in sig.items():
        if name in OPTIONAL_EXPORTS and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res


def check(code, ctx=None):
    if code != OK:
        msg = lib().plssvm_mi_last_error(ctx)
        raise BackendError(code, msg.decode() if msg else "")
