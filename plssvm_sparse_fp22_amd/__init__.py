"""plssvm_sparse_fp22_amd — MI355X-native PLSSVM CG hot path (implicit Q~·p), host-side mirror.

Mirrors the reference's C++ surface for this path so tests read like the reference's own:

* :class:`Parameter` ~ ``plssvm::parameter<T>`` (include/plssvm/parameter.hpp:181-194 defaults:
  C = 1, epsilon = 1e-3, degree = 3, gamma = 1/d, coef0 = 0);
* :class:`CSVM` ~ ``plssvm::hip::csvm<T>`` / ``detail::gpu_csvm<T, ...>``
  (include/plssvm/csvm.hpp:33-278, include/plssvm/backends/gpu_csvm.hpp:37-190) including the
  protected-for-mock hooks of ``mock_hip_csvm`` (tests/backends/HIP/mock_hip_csvm.hpp:24-51):
  ``setup_data_on_device``, ``generate_q``, ``run_device_kernel`` (+ reduction), ``solver_CG``,
  ``set_cost``, ``set_QA_cost``.

Everything computes in libplssvm_mi355x.so (hand-written gfx950 HIP kernels) through the C ABI
``include/plssvm_mi355x.h``; this module only marshals host buffers.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _abi
from ._abi import BackendError, KERNELS
from . import io as _io
from .io import parse_libsvm, parse_model, read_binary, write_binary, write_model

__all__ = ["Parameter", "CSVM", "BackendError", "parse_libsvm", "parse_model", "read_binary", "write_binary",
           "device_count", "unique_id", "partition", "torch_exchange", "one_vs_all", "class_point_weights",
           "one_vs_all_weights"]


def device_count() -> int:
    return int(_abi.lib().plssvm_mi_device_count())


def unique_id() -> bytes:
    """RCCL unique id for a row-block group (rank 0 creates it and shares it out of band)."""
    buf = ctypes.create_string_buffer(_abi.UNIQUE_ID_BYTES)
    _abi.check(_abi.lib().plssvm_mi_get_unique_id(buf))
    return buf.raw


def partition(m, rank, world_size):
    """Work split of the implicit matrix (host-only): (first super-block, end super-block,
    total tiles, tiles owned by rank); see plssvm_mi_partition in include/plssvm_mi355x.h."""
    out = (ctypes.c_int64 * 4)()
    _abi.check(_abi.lib().plssvm_mi_partition(m, rank, world_size, out))
    return tuple(out)


def torch_exchange(dist, group=None):
    """Host-staged exchange (plssvm_mi_comm_init_host) over torch.distributed, e.g. gloo: every rank
    all-gathers the buffers and sums them in rank order 0..G-1, so all ranks get the same bits — the
    reference's device_reduction, which sums devices 0..G-1 on the host (gpu_csvm.cpp:366-386).

    Failure protocol: each payload carries one status element. A rank whose local step fails still
    takes part in the collective (sending the failure flag), and then every rank raises, so the whole
    group returns PLSSVM_MI_ERR_RCCL together instead of the peers waiting forever in the collective."""
    import torch

    def fn(buf, op, local_error=None):
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        count = buf.size // world if op == _abi.XCHG_ALLGATHER else buf.size
        dt = torch.from_numpy(buf[:0]).dtype
        payload = torch.zeros(count + 1, dtype=dt)
        try:
            if local_error is not None:
                raise local_error
            src = buf[rank * count:(rank + 1) * count] if op == _abi.XCHG_ALLGATHER else buf
            payload[:count] = torch.from_numpy(src.copy())
        except Exception as e:  # noqa: BLE001 — still join the collective, flagged
            payload.zero_()
            payload[count] = 1
            err = e
        else:
            err = None
        parts = [torch.empty(count + 1, dtype=dt) for _ in range(world)]
        dist.all_gather(parts, payload, group=group)
        failed = [r for r in range(world) if float(parts[r][count]) != 0.0]
        if failed:
            raise RuntimeError(f"host exchange failed on rank(s) {failed}") from err
        if op == _abi.XCHG_ALLGATHER:
            for r in range(world):
                buf[r * count:(r + 1) * count] = parts[r][:count].numpy()
        else:
            acc = parts[0][:count].numpy().copy()
            for r in range(1, world):
                acc += parts[r][:count].numpy()
            buf[:] = acc

    return fn


def one_vs_all(labels, dtype=np.float64):
    """One-vs-all coding of integer or float class labels: (classes, Y) with the sorted unique labels and the
    [K][n] matrix of +1 (the point is of class k) / -1 in the real type ``dtype`` — plssvm_mi_learn_multi's Y."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0:
        raise ValueError("labels must be a non-empty 1-D array")
    if not (np.issubdtype(labels.dtype, np.integer) or np.issubdtype(labels.dtype, np.floating)):
        raise ValueError("class labels must be integers or floats")
    if np.issubdtype(labels.dtype, np.floating) and not np.isfinite(labels).all():
        raise ValueError("class labels must be finite")
    classes = np.unique(labels)
    one = np.dtype(dtype).type(1)
    Y = np.where(labels[None, :] == classes[:, None], one, -one).astype(dtype)
    return classes, np.ascontiguousarray(Y)


def _check_class_weight(class_weight):
    """{label: weight} with finite weights > 0, or None."""
    if class_weight is None:
        return None
    if not isinstance(class_weight, dict) or not class_weight:
        raise ValueError("class_weight must be a non-empty {label: weight} dict")
    for lab, w in class_weight.items():
        if not (np.isfinite(w) and w > 0):
            raise ValueError(f"class_weight: the weight of label {lab!r} must be a finite number > 0, not {w!r}")
    return dict(class_weight)


def class_point_weights(labels, class_weight, dtype=np.float64):
    """Point weights s [n] of a {label: weight} dict (LIBSVM's -wi): s_i = the weight of point i's label, 1 for a label
    the dict does not name. A label in the dict that the data lacks is a ValueError."""
    cw = _check_class_weight(class_weight)
    labels = np.asarray(labels)
    s = np.ones(labels.shape[0], dtype=dtype)
    for lab, w in cw.items():
        hit = labels == lab
        if not hit.any():
            raise ValueError(f"class_weight names the label {lab!r}, which the data does not have")
        s[hit] = w
    return s


def one_vs_all_weights(labels, class_weight, dtype=np.float64):
    """The weight rows S [K][n] of one-vs-all training with weighted positives: row c weighs the points of class c by
    class_weight[c] and every other point by 1 (classes the dict does not name: all 1)."""
    cw = _check_class_weight(class_weight)
    classes, _ = one_vs_all(labels, dtype)
    labels = np.asarray(labels)
    S = np.ones((classes.size, labels.shape[0]), dtype=dtype)
    for lab, w in cw.items():
        hit = np.flatnonzero(classes == lab)
        if hit.size == 0:
            raise ValueError(f"class_weight names the label {lab!r}, which the data does not have")
        S[hit[0], labels == lab] = w
    return np.ascontiguousarray(S)


def stratified_folds(labels, nfold):
    """Fold of every point for k-fold cross-validation: point i goes to fold (its rank among the points of its label, in
    index order) mod nfold. Every fold gets floor(c / nfold) or ceil(c / nfold) points of a label with c points. No
    random numbers: the same labels give the same folds (plssvm-train -v uses the same rule)."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size == 0:
        raise ValueError("labels must be a non-empty 1-D array")
    nfold = int(nfold)
    if nfold < 2 or nfold > labels.size:
        raise ValueError(f"nfold must be between 2 and the number of points ({labels.size}), not {nfold}")
    folds = np.empty(labels.size, dtype=np.int64)
    for lab in np.unique(labels):
        idx = np.flatnonzero(labels == lab)
        folds[idx] = np.arange(idx.size) % nfold
    return folds


def _rows(a, dtype, m, what):
    """[R][ld] row-major matrix of the real type with ld >= m (a 1-D vector counts as one row)."""
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=dtype)
    if a.ndim != 2 or a.shape[0] < 1:
        raise ValueError(f"{what} must be a [vectors][length] matrix with at least one vector")
    if a.shape[1] < m:
        raise ValueError(f"{what} rows must have at least {m} entries")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Parameter:
    """plssvm::parameter<T> subset used by the hot path."""

    def __init__(self, kernel="linear", degree=3, gamma=0.0, coef0=0.0, cost=1.0, epsilon=1e-3,
                 real_type=np.float64, print_info=False, class_weight=None):
        if kernel not in KERNELS:
            raise ValueError(f"Unknown kernel type {kernel!r}")
        # {label: weight}: learn() trains the points of `label` at cost C * weight (binary labels; learn_multi takes
        # its own class_weight)
        self.class_weight = _check_class_weight(class_weight)
        self.kernel = kernel
        self.degree = int(degree)
        self.gamma = gamma
        self.coef0 = coef0
        self.cost = cost
        self.epsilon = epsilon
        self.real_type = np.dtype(real_type)
        self.print_info = print_info
        self.data = None  # dense [n][d]
        self.csr = None  # (rowptr, col, val, n, d); val real or packed FP22 words
        self.coo = None  # (row, col, val, n, d) triplets in any order; val real or packed FP22 words
        self.val_fmt = _abi.VAL_REAL
        self.labels = None

    def parse_train_file(self, path, sparse=False, multiclass=False):
        """multiclass: keep the label values as written (learn_multi's classes) instead of their signs."""
        try:
            with open(path, "rb") as f:
                binary = f.read(8) == _io.BIN_MAGIC
        except FileNotFoundError:  # file_not_found_exception (src/plssvm/detail/file_reader.cpp:104-108)
            raise FileNotFoundError(f"Couldn't find file: '{path}'!") from None
        if binary:  # PLSSVMB1 binary CSR / FP22 file (io.write_binary): always sparse
            csr, y, fmt = _io.read_binary(path, dtype=self.real_type)
            self.csr, self.data, self.labels = csr, None, y
            self.val_fmt = _abi.VAL_FP22 if fmt == _io.BIN_FP22 else _abi.VAL_REAL
            if self.gamma == 0:
                self.gamma = float(self.real_type.type(1) / self.real_type.type(csr[4]))
            return self
        X, y = parse_libsvm(path, dtype=self.real_type, sparse=sparse, multiclass=multiclass)
        if sparse:
            self.csr, self.data = X, None
            d = X[4]
        else:
            self.data, self.csr = X, None
            d = X.shape[1]
        self.labels = y
        if self.gamma == 0:  # parameter.cpp:150-152
            self.gamma = float(self.real_type.type(1) / self.real_type.type(d))
        return self

    def point_weights(self):
        """The point weights of class_weight on this parameter's labels (None without class_weight)."""
        if self.class_weight is None:
            return None
        if self.labels is None:
            raise ValueError("class_weight needs labels")
        return class_point_weights(self.labels, self.class_weight, self.real_type)

    @property
    def num_features(self):
        if self.data is not None:
            return self.data.shape[1]
        return int((self.csr if self.csr is not None else self.coo)[4])

    @property
    def num_data_points(self):
        if self.data is not None:
            return self.data.shape[0]
        return int((self.csr if self.csr is not None else self.coo)[3])


class CSVM:
    """One MI355X context (one GPU, one HIP stream). ``world_size > 1`` joins a row-block group."""

    def __init__(self, params: Parameter, device=0, rank=0, world_size=1, uid=None, kp_mode="auto",
                 sim_rank=None, rbf_form=0, exchange=None, sparse_algo="auto", cg_variant=None, kp_cache=None,
                 multi_width=None, kp_pack=None):
        if params.data is None and params.csr is None and params.coo is None:
            raise ValueError("No data points provided!")
        if params.data is not None:
            if params.data.ndim != 2 or params.data.shape[0] == 0:
                raise ValueError("Data set is empty!")
            if params.data.shape[1] == 0:
                raise ValueError("No features provided for the data points!")
        if KERNELS[params.kernel] == KERNELS["laplacian"] and params.data is None:
            raise ValueError("The Laplacian kernel takes dense data: parse the file with sparse=False (there is no sparse "
                             "L1-distance K.p)")
        self.params = params
        self.dtype = params.real_type
        self.num_data_points = params.num_data_points
        self.num_features = params.num_features
        gamma = params.gamma if params.gamma != 0 else 1.0 / self.num_features
        self._ctx = ctypes.c_void_p()
        L = _abi.lib()
        _abi.check(L.plssvm_mi_create(self.dtype.itemsize, KERNELS[params.kernel], params.degree, float(gamma),
                                      float(params.coef0), float(params.cost), device, ctypes.byref(self._ctx)))
        mode = {"auto": _abi.KP_AUTO, "pairwise": _abi.KP_PAIRWISE, "factored": _abi.KP_FACTORED}[kp_mode]
        if mode != _abi.KP_AUTO:
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_KP_MODE, mode))
        if rbf_form:  # 1 = direct RBF pair form on sparse data, see PLSSVM_MI_OPT_RBF_FORM
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_RBF_FORM, rbf_form))
        algo = {"auto": _abi.SPARSE_AUTO, "pattern": _abi.SPARSE_PATTERN, "expansion": _abi.SPARSE_EXPANSION,
                "dense": _abi.SPARSE_DENSE, "onthefly": _abi.SPARSE_ONTHEFLY}[sparse_algo]
        if algo != _abi.SPARSE_AUTO:  # sparse poly/rbf K·p algorithm, see PLSSVM_MI_OPT_SPARSE_ALGO
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_SPARSE_ALGO, algo))
        if cg_variant is not None:  # "reference" | "one_reduction" | "auto", see PLSSVM_MI_OPT_CG_VARIANT
            v = {"reference": 0, "one_reduction": 1, "auto": 2}[cg_variant]
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_CG_VARIANT, v))
        if kp_cache is not None:  # False: never store kernel-matrix tiles, see PLSSVM_MI_OPT_KP_CACHE
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_KP_CACHE, 0 if kp_cache else 1))
        if kp_pack is not None:  # False: stored fp64 tiles keep their raw 8-byte records; "wide": 7-byte records but no
            # 53-bit ones; True: the default, see PLSSVM_MI_OPT_KP_PACK
            if isinstance(kp_pack, str) and kp_pack != "wide":
                raise ValueError(f"kp_pack must be True, False or 'wide', not {kp_pack!r}")
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_KP_PACK, 2 if kp_pack == "wide" else (0 if kp_pack else 1)))
        if multi_width is not None:  # 0 auto, 1 one vector at a time, n: at most n lanes, see PLSSVM_MI_OPT_MULTI_WIDTH
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_MULTI_WIDTH, int(multi_width)))
        if sim_rank is not None:  # (rank, world): single-GPU test hook, see PLSSVM_MI_OPT_SIM_RANK
            self._check(L.plssvm_mi_set_option(self._ctx, _abi.OPT_SIM_RANK, sim_rank[0] | (sim_rank[1] << 16)))
        if exchange is not None:  # host-staged group: fn(numpy buffer, op) combines in place (torch_exchange)
            self._xchg = _abi.EXCHANGE_FN(self._exchange_cb(exchange, world_size))
            self._check(L.plssvm_mi_comm_init_host(self._ctx, rank, world_size, self._xchg, None))
        elif world_size > 1 or uid is not None:  # a single-rank group (uid given) also runs its collectives on RCCL
            if uid is None:
                raise ValueError("world_size > 1 needs the group's unique id (rank 0: plssvm_sparse_fp22_amd.unique_id())")
            self._uid = ctypes.create_string_buffer(uid, _abi.UNIQUE_ID_BYTES)
            self._check(L.plssvm_mi_comm_init(self._ctx, rank, world_size, self._uid))
        self.world_size = world_size
        self.rank = rank
        self.QA_cost = None
        self.w = None
        self.alpha = None
        self.bias = None
        self.trace = None
        self.iters = None
        self.classes = None  # learn_multi: sorted class labels, alphas [K][n], biases [K]
        self.alphas = None
        self.biases = None
        self.iters_multi = None
        self.traces = None
        self.pivots = None  # learn_held: each lane's largest training index
        self.cv_iters = None  # cross_validate: iterations per lane (lane = cost * nfold + fold)
        self._on_device = False
        self._cw_applied = False  # the context's weights are those of Parameter.class_weight (learn / learn_costs)

    @staticmethod
    def _exchange_cb(exchange, world_size):
        # exchange(buf, op) must be collective even when it fails: torch_exchange flags a local failure
        # inside its collective so every rank raises (a custom exchange that raises before its collective
        # leaves the peers waiting in theirs)
        def cb(ptr, count, real_bytes, op, user):
            try:
                n = count * (world_size if op == _abi.XCHG_ALLGATHER else 1)
                ct = ctypes.c_float if real_bytes == 4 else ctypes.c_double
                buf = np.ctypeslib.as_array((ct * n).from_address(ptr))
                exchange(buf, op)
                return 0
            except Exception:  # noqa: BLE001 — reported as PLSSVM_MI_ERR_RCCL by the library
                import traceback

                traceback.print_exc()
                return -1

        return cb

    # ---- lifetime ----
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            _abi.lib().plssvm_mi_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, code):
        _abi.check(code, self._ctx)

    @property
    def m(self):
        return self.num_data_points - 1

    # ---- gpu_csvm hot-path surface ----
    def setup_data_on_device(self):
        L = _abi.lib()
        p = self.params
        if p.data is not None:
            X = np.ascontiguousarray(p.data, dtype=self.dtype)
            self._check(L.plssvm_mi_setup_dense(self._ctx, _ptr(X), X.shape[0], X.shape[1]))
        elif p.csr is not None:
            rowptr, col, val, n, d = p.csr
            rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
            col = np.ascontiguousarray(col, dtype=np.int32)
            val = np.ascontiguousarray(val, dtype=np.uint32 if p.val_fmt == _abi.VAL_FP22 else self.dtype)
            self._check(L.plssvm_mi_setup_csr(self._ctx, _ptr(rowptr), _ptr(col), _ptr(val), p.val_fmt, n, d))
        else:
            row, col, val, n, d = p.coo
            row = np.ascontiguousarray(row, dtype=np.int64)
            col = np.ascontiguousarray(col, dtype=np.int32)
            val = np.ascontiguousarray(val, dtype=np.uint32 if p.val_fmt == _abi.VAL_FP22 else self.dtype)
            self._check(L.plssvm_mi_setup_coo(self._ctx, _ptr(row), _ptr(col), _ptr(val), p.val_fmt, row.size, n, d))
        self._on_device = True
        self._cw_applied = False  # a setup clears the context's weights

    def generate_q(self):
        q = np.zeros(max(self.m, 1), dtype=self.dtype)
        qa = ctypes.c_double()
        self._check(_abi.lib().plssvm_mi_generate_q(self._ctx, _ptr(q), ctypes.byref(qa)))
        self.QA_cost = self.dtype.type(qa.value)
        return q[: self.m]

    def set_cost(self, cost):
        self._check(_abi.lib().plssvm_mi_set_cost(self._ctx, float(cost)))

    def set_point_weights(self, s):
        """Point i is trained at cost C * s[i] (s: n finite reals > 0, the last point included; None clears them). They
        hold for every later K.p, CG solve and learn of this context until cleared or the next setup."""
        if not self._on_device:
            self.setup_data_on_device()
        if s is not None:
            s = np.ascontiguousarray(s, dtype=self.dtype)
            if s.shape != (self.num_data_points,):
                raise ValueError(f"the point weights must have {self.num_data_points} entries")
        self._check(_abi.lib().plssvm_mi_set_point_weights(self._ctx, _ptr(s)))
        self._cw_applied = False

    def _apply_class_weight(self, s):
        """The weights of Parameter.class_weight (s; None: none) for a learn: set, or — where an earlier learn applied
        some — cleared. Weights the caller set with set_point_weights stay."""
        if s is not None:
            self.set_point_weights(s)
            self._cw_applied = True
        elif self._cw_applied:
            self.set_point_weights(None)

    def set_QA_cost(self, qa):
        self._check(_abi.lib().plssvm_mi_set_qa_cost(self._ctx, float(qa)))
        self.QA_cost = self.dtype.type(qa)

    def run_device_kernel(self, q, ret, d, add):
        """ret += add * Q~ d (run_device_kernel + device_reduction); q=None uses the device q."""
        assert ret.dtype == self.dtype and ret.flags.c_contiguous
        qq = None if q is None else np.ascontiguousarray(q, dtype=self.dtype)
        dd = np.ascontiguousarray(d, dtype=self.dtype)
        self._check(_abi.lib().plssvm_mi_kp(self._ctx, _ptr(qq), _ptr(dd), _ptr(ret), float(add)))
        return ret

    def kp_part(self, p, part="kernel"):
        """Test hook (plssvm_mi_kp_part): 'kernel' = sum_j k(x_i, x_j) p_j; 'overlap' = the sparse
        poly/rbf overlap sum (the per-pair work of the sparse kernels only); 'remainder' = the kernel
        expansion's stored remainder stream alone (pairs sharing >= 2 features, in the stored layout)."""
        pp = np.ascontiguousarray(p, dtype=self.dtype)
        out = np.zeros(max(self.m, 1), dtype=self.dtype)
        code = {"kernel": _abi.PART_KERNEL, "overlap": _abi.PART_OVERLAP, "remainder": _abi.PART_REMAINDER}[part]
        self._check(_abi.lib().plssvm_mi_kp_part(self._ctx, _ptr(pp), _ptr(out), code))
        return out[: self.m]

    def solver_CG(self, b, imax, eps, q=None):
        b = np.ascontiguousarray(b, dtype=self.dtype)
        qq = None if q is None else np.ascontiguousarray(q, dtype=self.dtype)
        x = np.zeros(max(self.m, 1), dtype=self.dtype)
        trace = np.full(imax + 1, np.nan)
        it = ctypes.c_int64()
        self._check(_abi.lib().plssvm_mi_solve_cg(self._ctx, _ptr(b), _ptr(qq), imax, float(eps), _ptr(x),
                                                  _ptr(trace), ctypes.byref(it)))
        self.iters = it.value
        self.trace = trace[: it.value + 1]
        return x[: self.m]

    def learn(self, imax=-1):
        """csvm<T>::learn(): setup, q, QA_cost, CG with imax = num_features, bias, alpha[m] = -sum."""
        if self.params.labels is None:
            raise ValueError("No labels given for training! Maybe the data is only usable for prediction?")
        s = self.params.point_weights()  # class_weight (checked before the device is touched)
        if not self._on_device:
            self.setup_data_on_device()
        self._apply_class_weight(s)
        y = np.ascontiguousarray(self.params.labels, dtype=self.dtype)
        alpha = np.zeros(self.num_data_points, dtype=self.dtype)
        bias = ctypes.c_double()
        im = self.num_features if imax < 0 else imax
        trace = np.full(im + 1, np.nan)
        it = ctypes.c_int64()
        self._check(_abi.lib().plssvm_mi_learn(self._ctx, _ptr(y), im, float(self.params.epsilon), _ptr(alpha),
                                               ctypes.byref(bias), _ptr(trace), ctypes.byref(it)))
        self.alpha = alpha
        self.bias = self.dtype.type(bias.value)
        self.rho = -self.bias
        self.iters = it.value
        self.trace = trace[: it.value + 1]
        return self

    # ---- several right-hand sides / classes at once (plssvm_mi_*_multi) ----
    def run_device_kernel_multi(self, q, RET, P, add):
        """RET[c] += add * Q~ P[c] for every row c; rows may be longer than m (the tail is never touched). Each row is
        bitwise run_device_kernel of that row."""
        assert RET.dtype == self.dtype and RET.flags.c_contiguous and RET.ndim == 2
        qq = None if q is None else np.ascontiguousarray(q, dtype=self.dtype)
        PP = _rows(P, self.dtype, self.m, "P")
        if PP.shape != RET.shape:
            raise ValueError("P and RET must have the same shape")
        self._check(_abi.lib().plssvm_mi_kp_multi(self._ctx, _ptr(qq), _ptr(PP), _ptr(RET), PP.shape[0], PP.shape[1],
                                                  float(add)))
        return RET

    def solver_CG_multi(self, B, imax, eps, q=None):
        """solver_CG for every row of B[R][>= m]; returns X[R][m] and sets iters_multi [R] and traces (R arrays)."""
        BB = _rows(B, self.dtype, self.m, "B")
        R, ld = BB.shape
        qq = None if q is None else np.ascontiguousarray(q, dtype=self.dtype)
        X = np.zeros((R, ld), dtype=self.dtype)
        trace = np.full((R, imax + 1), np.nan)
        it = np.zeros(R, dtype=np.int64)
        self._check(_abi.lib().plssvm_mi_solve_cg_multi(self._ctx, _ptr(BB), R, ld, _ptr(qq), imax, float(eps), _ptr(X),
                                                        _ptr(trace), _ptr(it)))
        self.iters_multi = it
        self.traces = [trace[c, : it[c] + 1].copy() for c in range(R)]
        return X[:, : self.m]

    def _learn_lanes(self, Y, costs, S, imax, hold=None):
        """plssvm_mi_learn_lanes on Y [K][n]: costs [K] or None, S [K][n] / [n] (one row for all) or None; with hold
        (uint8 [K][n]) plssvm_mi_learn_held, which also sets pivots."""
        K, n = Y.shape
        im = self.num_features if imax < 0 else imax
        alphas = np.zeros((K, n), dtype=self.dtype)
        biases = np.zeros(K, dtype=np.float64)
        trace = np.full((K, im + 1), np.nan)
        it = np.zeros(K, dtype=np.int64)
        cc = None if costs is None else np.ascontiguousarray(costs, dtype=np.float64)
        SS = None if S is None else np.ascontiguousarray(S, dtype=self.dtype)
        if cc is not None and cc.shape != (K,):
            raise ValueError(f"costs must have {K} entries")
        if SS is not None and SS.shape not in ((K, n), (n,)):
            raise ValueError(f"the weights must be [{K}][{n}] or one row of {n}")
        lds = 0 if SS is None or SS.ndim == 1 else SS.shape[1]
        out = (im, float(self.params.epsilon), _ptr(alphas), _ptr(biases), _ptr(trace), _ptr(it))
        if hold is None:
            self._check(_abi.lib().plssvm_mi_learn_lanes(self._ctx, _ptr(Y), K, n, _ptr(cc), _ptr(SS), lds, *out))
        else:
            piv = np.zeros(K, dtype=np.int64)
            self._check(_abi.lib().plssvm_mi_learn_held(self._ctx, _ptr(Y), K, n, _ptr(cc), _ptr(SS), lds, _ptr(hold), n,
                                                        *out, _ptr(piv)))
            self.pivots = piv
        self.alphas = alphas
        self.biases = biases.astype(self.dtype)
        self.iters_multi = it
        self.traces = [trace[c, : it[c] + 1].copy() for c in range(K)]
        return self

    def learn_costs(self, costs, imax=-1):
        """learn() at every cost of `costs` (a search over C): the K systems share every kernel value and differ only in
        their diagonal, so where learn_multi's classes share a pass over the kernel matrix these do too. Row k of alphas
        [K][n], biases [K], iters_multi, traces is bitwise set_cost(costs[k]); learn(). The context's cost stays."""
        if self.params.labels is None:
            raise ValueError("No labels given for training! Maybe the data is only usable for prediction?")
        costs = np.atleast_1d(np.asarray(costs, dtype=np.float64))
        if costs.ndim != 1 or costs.size < 1 or not (np.isfinite(costs).all() and (costs > 0).all()):
            raise ValueError("costs must be a non-empty list of finite numbers > 0")
        s = self.params.point_weights()
        if not self._on_device:
            self.setup_data_on_device()
        self._apply_class_weight(s)
        y = np.ascontiguousarray(self.params.labels, dtype=self.dtype)
        Y = np.ascontiguousarray(np.tile(y, (costs.size, 1)))
        self._learn_lanes(Y, costs, None, imax)
        self.costs = costs
        return self

    def learn_held(self, hold, costs=None, S=None, imax=-1):
        """learn() on subsets, as lanes of one batched CG (plssvm_mi_learn_held): lane k leaves out the points with
        hold[k][i] true (hold: bool [K][n]) and trains at costs[k] (None: the context's cost) with the weights S ([K][n],
        one row [n] for all, or None: the context's). Sets alphas [K][n] (exactly 0 on held-out points), biases [K],
        iters_multi, traces and pivots [K] (each lane's largest training index). Parameter.class_weight applies as in
        learn_costs (a row of S replaces it for its lane); the context's cost and q stay."""
        if self.params.labels is None:
            raise ValueError("No labels given for training! Maybe the data is only usable for prediction?")
        cw = self.params.point_weights()  # class_weight (checked before the device is touched)
        n = self.num_data_points
        H = np.ascontiguousarray(np.atleast_2d(np.asarray(hold)) != 0, dtype=np.uint8)
        if H.ndim != 2 or H.shape[1] != n or H.shape[0] < 1:
            raise ValueError(f"hold must be a [lanes][{n}] matrix")
        K = H.shape[0]
        if not self._on_device:
            self.setup_data_on_device()
        self._apply_class_weight(cw)
        y = np.ascontiguousarray(self.params.labels, dtype=self.dtype)
        return self._learn_lanes(np.ascontiguousarray(np.tile(y, (K, 1))), costs, S, imax, hold=H)

    def train_values(self, alphas=None, biases=None):
        """Decision values [n][K] of K models (default: alphas, biases as the last multi-lane learn left them) on the
        context's own n points, held-out ones included, from the kernel matrix the context already holds
        (plssvm_mi_train_values): no point is uploaded again. Column k is bitwise the same whatever K."""
        alphas = self.alphas if alphas is None else alphas
        biases = self.biases if biases is None else biases
        if alphas is None:
            raise ValueError("No alphas provided!")
        n = self.num_data_points
        A = _rows(alphas, self.dtype, n, "alphas")
        K, lda = A.shape
        b = np.zeros(K, dtype=np.float64) if biases is None else np.ascontiguousarray(np.atleast_1d(biases), dtype=np.float64)
        if b.shape != (K,):
            raise ValueError(f"biases must have {K} entries")
        if not self._on_device:
            self.setup_data_on_device()
        out = np.zeros((K, n), dtype=self.dtype)
        self._check(_abi.lib().plssvm_mi_train_values(self._ctx, _ptr(A), K, lda, _ptr(b), _ptr(out), n))
        return np.ascontiguousarray(out.T)

    def cross_validate(self, nfold=5, costs=None, folds=None, imax=-1):
        """k-fold cross-validation of the binary problem at every cost of `costs` (None: the parameter's cost), the
        nfold x len(costs) subset problems as lanes of one batched CG over the setup's stored kernel matrix: learn_held,
        then train_values, then each point's value from the model that did not see it. folds [n] (values 0 .. nfold - 1;
        None: stratified_folds of the labels). Parameter.class_weight and set_point_weights apply as in learn_costs.
        Returns (accuracy [len(costs)], held-out decision values [len(costs)][n], folds [n]); a value of exactly 0
        counts as the negative label, as predict() has it. The context's cost, weights, q and the object's model
        (alpha, bias, alphas, biases, ...) are what they were before the call."""
        if self.params.labels is None:
            raise ValueError("No labels given for training! Maybe the data is only usable for prediction?")
        n = self.num_data_points
        y = np.asarray(self.params.labels)
        if folds is None:
            folds = stratified_folds(y, nfold)
        else:
            folds = np.ascontiguousarray(folds, dtype=np.int64)
            nfold = int(nfold)
            if folds.shape != (n,) or folds.min() < 0 or folds.max() >= nfold or nfold < 2:
                raise ValueError(f"folds must have {n} entries in 0 .. nfold - 1, nfold >= 2")
        nfold = int(nfold)
        cl = np.atleast_1d(np.asarray(self.params.cost if costs is None else costs, dtype=np.float64))
        if cl.ndim != 1 or cl.size < 1 or not (np.isfinite(cl).all() and (cl > 0).all()):
            raise ValueError("costs must be a non-empty list of finite numbers > 0")
        self.params.point_weights()  # class_weight is checked before the device is touched; learn_held applies it
        if not self._on_device:
            self.setup_data_on_device()
        hold = np.concatenate([folds[None, :] == np.arange(nfold)[:, None]] * cl.size, axis=0)  # lane = cost * nfold + fold
        keep = {k: getattr(self, k, None) for k in ("alphas", "biases", "iters_multi", "traces", "pivots", "classes")}
        try:
            self.learn_held(hold, costs=np.repeat(cl, nfold), imax=imax)
            vals = self.train_values()  # [n][lanes]
            cv_iters = self.iters_multi
        finally:
            for k, v in keep.items():
                setattr(self, k, v)
        self.cv_iters = cv_iters
        lane = np.arange(cl.size)[:, None] * nfold + folds[None, :]
        held = np.ascontiguousarray(vals[np.arange(n)[None, :], lane])
        pred = np.where(held > 0, 1, -1)
        acc = (pred == np.where(y > 0, 1, -1)[None, :]).mean(axis=1)
        return acc, held, folds

    def learn_multi(self, labels=None, imax=-1, class_weight=None):
        """One-vs-all training on K >= 2 classes (any integer or float labels; default: the parameter's labels): per
        class exactly learn() on the +-1 labels of that class against the rest, the K solves sharing each pass over
        the kernel matrix. Sets classes [K], alphas [K][n], biases [K], iters_multi [K], traces.
        class_weight {label: w}: class c's problem weighs its own points (the positives) by w[c], all others by 1.
        Weights set with set_point_weights apply to every class; those an earlier learn() took from
        Parameter.class_weight are cleared first."""
        labels = self.params.labels if labels is None else labels
        if labels is None:
            raise ValueError("No labels given for training! Maybe the data is only usable for prediction?")
        classes, Y = one_vs_all(labels, self.dtype)
        if Y.shape[1] != self.num_data_points:
            raise ValueError(f"labels must have {self.num_data_points} entries")
        if classes.size < 2:
            raise ValueError("learn_multi needs at least 2 classes")
        S = None if class_weight is None else one_vs_all_weights(labels, class_weight, self.dtype)
        if not self._on_device:
            self.setup_data_on_device()
        self._apply_class_weight(None)  # the binary class_weight of an earlier learn() does not reach the classes
        self._learn_lanes(Y, None, S, imax)  # S None: plssvm_mi_learn_multi's call, lanes that differ in b only
        self.classes = classes
        return self

    def predict_values_multi(self, points, val_fmt=None, alphas=None, biases=None):
        """Decision values [np][K] of the learn_multi model (or of alphas [K][n], biases [K]) in one call: on dense
        data with the polynomial / rbf kernel every class shares one pass over the kernel values; on sparse data and
        with the linear kernel the points are prepared once and up to 8 classes share each pass over the support
        vectors. Column k is bitwise predict_values with class k's alpha and bias."""
        alphas = self.alphas if alphas is None else alphas
        biases = self.biases if biases is None else biases
        if alphas is None:
            raise ValueError("No alphas provided for prediction!")
        A = _rows(alphas, self.dtype, self.num_data_points, "alphas")
        K, lda = A.shape
        b = np.zeros(K, dtype=np.float64) if biases is None else np.ascontiguousarray(biases, dtype=np.float64)
        if b.shape != (K,):
            raise ValueError(f"biases must have {K} entries")
        if not self._on_device:
            self.setup_data_on_device()
        L = _abi.lib()
        if isinstance(points, tuple):
            rowptr, col, val, npts, d = points
            fmt = _abi.VAL_REAL if val_fmt is None else val_fmt
            rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
            col = np.ascontiguousarray(col, dtype=np.int32)
            val = np.ascontiguousarray(val, dtype=np.uint32 if fmt == _abi.VAL_FP22 else self.dtype)
            out = np.zeros((K, max(npts, 1)), dtype=self.dtype)
            self._check(L.plssvm_mi_predict_multi_csr(self._ctx, _ptr(A), K, lda, _ptr(b), _ptr(rowptr), _ptr(col),
                                                      _ptr(val), fmt, npts, d, _ptr(out), out.shape[1]))
            return np.ascontiguousarray(out[:, :npts].T)
        Z = np.ascontiguousarray(points, dtype=self.dtype)
        if Z.ndim != 2:
            raise ValueError("points must be a 2-D array [np][d]")
        out = np.zeros((K, max(Z.shape[0], 1)), dtype=self.dtype)
        self._check(L.plssvm_mi_predict_multi_dense(self._ctx, _ptr(A), K, lda, _ptr(b), _ptr(Z), Z.shape[0], Z.shape[1],
                                                    _ptr(out), out.shape[1]))
        return np.ascontiguousarray(out[:, : Z.shape[0]].T)

    def predict_multi(self, points, val_fmt=None):
        """The class with the largest decision value (the lowest class index on a tie)."""
        return self.classes[np.argmax(self.predict_values_multi(points, val_fmt), axis=1)]

    def predict_stats(self):
        """[classes served per pass over the support vectors, point uploads] of the last predict call ([0, 0] before
        any): [min(K, 8), 1] when the classes share the pass, [1, K] when they ran one after another."""
        out = (ctypes.c_int64 * 2)()
        self._check(_abi.lib().plssvm_mi_get_predict_stats(self._ctx, out))
        return [int(out[0]), int(out[1])]

    def spmv_plan(self):
        """The plans of the factored sparse-linear K.p as the setup built them (plssvm_mi_get_spmv_plan): "csc" and
        "csr", the passes w = X^T p and raw = X w, each {P, ldsx, W, nblocks, nchunks, f22}, and "rb", the row-block
        CSR pass of the one-GPU CG, {P, W, RBK, nblk}; all zeros when the context is not a factored sparse one."""
        out = (ctypes.c_int64 * 16)()
        self._check(_abi.lib().plssvm_mi_get_spmv_plan(self._ctx, out))
        v = [int(x) for x in out]
        keys = ("P", "ldsx", "W", "nblocks", "nchunks", "f22")
        return {"csc": dict(zip(keys, v[0:6])), "csr": dict(zip(keys, v[6:12])),
                "rb": dict(zip(("P", "W", "RBK", "nblk"), v[12:16]))}

    def time_kp_multi(self, nrhs, reps=5):
        a = ctypes.c_double()
        self._check(_abi.lib().plssvm_mi_time_kp_multi(self._ctx, int(nrhs), reps, ctypes.byref(a)))
        return a.value

    # ---- model use: update_w / predict / accuracy (csvm.hpp:123-178, gpu_csvm.cpp:52-127,327-350) ----
    def _model(self, alpha, bias):
        alpha = self.alpha if alpha is None else alpha
        bias = self.bias if bias is None else bias
        if alpha is None:
            raise ValueError("No alphas provided for prediction!")
        alpha = np.ascontiguousarray(alpha, dtype=self.dtype)
        if alpha.shape != (self.num_data_points,):
            raise ValueError(f"alpha must have {self.num_data_points} entries")
        if not self._on_device:
            self.setup_data_on_device()
        return alpha, float(0.0 if bias is None else bias)

    def update_w(self, alpha=None):
        """w = sum_i alpha_i x_i over all points (the linear kernel's model vector)."""
        alpha, _ = self._model(alpha, 0.0)
        w = np.zeros(max(self.num_features, 1), dtype=self.dtype)
        self._check(_abi.lib().plssvm_mi_update_w(self._ctx, _ptr(alpha), _ptr(w)))
        self.w = w[: self.num_features]
        return self.w

    def predict_values(self, points, alpha=None, bias=None, val_fmt=None):
        """Decision values bias + sum_i alpha_i k(x_i, z) for dense points [np][d] or a CSR tuple
        (rowptr, col, val, np, d); defaults to the learned alpha and bias."""
        alpha, b = self._model(alpha, bias)
        L = _abi.lib()
        if isinstance(points, tuple):
            rowptr, col, val, npts, d = points
            fmt = _abi.VAL_REAL if val_fmt is None else val_fmt
            rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
            col = np.ascontiguousarray(col, dtype=np.int32)
            val = np.ascontiguousarray(val, dtype=np.uint32 if fmt == _abi.VAL_FP22 else self.dtype)
            out = np.zeros(max(npts, 1), dtype=self.dtype)
            self._check(L.plssvm_mi_predict_csr(self._ctx, _ptr(alpha), b, _ptr(rowptr), _ptr(col), _ptr(val), fmt,
                                                npts, d, _ptr(out)))
            return out[:npts]
        Z = np.ascontiguousarray(points, dtype=self.dtype)
        if Z.ndim != 2:
            raise ValueError("points must be a 2-D array [np][d]")
        out = np.zeros(max(Z.shape[0], 1), dtype=self.dtype)
        self._check(L.plssvm_mi_predict_dense(self._ctx, _ptr(alpha), b, _ptr(Z), Z.shape[0], Z.shape[1], _ptr(out)))
        return out[: Z.shape[0]]

    def predict(self, points, alpha=None, bias=None, val_fmt=None):
        """Predicted labels (+-1): plssvm::operators::sign of the decision values (operators.hpp:174-177)."""
        v = self.predict_values(points, alpha, bias, val_fmt)
        return np.where(v > 0, self.dtype.type(1), self.dtype.type(-1))

    def accuracy(self, points=None, labels=None):
        """csvm::accuracy: fraction of correctly predicted labels (defaults: the training data)."""
        if points is None:
            points = self.params.data if self.params.data is not None else self.params.csr
            labels = self.params.labels
        if labels is None:
            raise ValueError("No labels given for the accuracy calculation!")
        pred = self.predict(points)
        if pred.shape[0] != len(labels):
            raise ValueError("the number of points to predict and correct labels mismatch")
        return float(np.mean(pred == np.asarray(labels, dtype=self.dtype)))

    # ---- stepwise CG + timing (bench.py) ----
    def cg_begin(self, b, q=None, eps=None):
        b = np.ascontiguousarray(b, dtype=self.dtype)
        qq = None if q is None else np.ascontiguousarray(q, dtype=self.dtype)
        d0 = ctypes.c_double()
        e = self.params.epsilon if eps is None else eps
        self._check(_abi.lib().plssvm_mi_cg_begin(self._ctx, _ptr(b), _ptr(qq), float(e), ctypes.byref(d0)))
        return d0.value

    def cg_step(self, n, force=False):
        it = ctypes.c_int64()
        conv = ctypes.c_int()
        self._check(_abi.lib().plssvm_mi_cg_step(self._ctx, n, 1 if force else 0, ctypes.byref(it),
                                                 ctypes.byref(conv)))
        return it.value, bool(conv.value)

    def cg_result(self, trace_len=0):
        x = np.zeros(max(self.m, 1), dtype=self.dtype)
        trace = np.full(max(trace_len, 1), np.nan)
        it = ctypes.c_int64()
        self._check(_abi.lib().plssvm_mi_cg_result(self._ctx, _ptr(x), _ptr(trace), trace_len, ctypes.byref(it)))
        return x[: self.m], trace[: min(trace_len, it.value + 1)], it.value

    def time_kp(self, reps=5):
        a, b = ctypes.c_double(), ctypes.c_double()
        self._check(_abi.lib().plssvm_mi_time_kp(self._ctx, reps, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def info(self):
        inf = _abi.Info()
        self._check(_abi.lib().plssvm_mi_get_info(self._ctx, ctypes.byref(inf)))
        out = {k: getattr(inf, k) for k, _ in _abi.Info._fields_}
        # the narrow tiles among kp_cache_packed_tiles: an entry point of its own (plssvm_mi_info keeps its size); a
        # PLSSVM_MI_LIB build from before the narrow form has none and stores no such tile
        narrow = ctypes.c_int64(0)
        fn = getattr(_abi.lib(), "plssvm_mi_get_kp_cache_narrow_tiles", None)
        if fn is not None:
            self._check(fn(self._ctx, ctypes.byref(narrow)))
        out["kp_cache_narrow_tiles"] = narrow.value
        return out

    def get_num_devices(self):
        return self.world_size
