/*
 * plssvm_mi355x.h — C ABI of the MI355X-native PLSSVM CG hot path (libplssvm_mi355x.so).
 *
 * The reference exposes this path only as C++ virtuals of plssvm::csvm<T> /
 * plssvm::detail::gpu_csvm<T, device_ptr_t, queue_t>; every entry point below names the
 * reference member it replaces (paths relative to the reference repository root). The C++
 * adapter plssvm::mi355x::csvm<T> (plssvm_sparse_fp22_amd/host/csvm.hpp) maps those virtuals
 * onto these calls; ctypes/cgo/JNI bindings can call them directly.
 *
 * Conventions
 *   - Every function returns PLSSVM_MI_OK (0) or a negative PLSSVM_MI_ERR_* code; no C++
 *     exception crosses the ABI. plssvm_mi_last_error() returns the message of the last
 *     failure on that context (the text the reference would put in its backend_exception).
 *   - Host buffers are caller-owned. Calls taking host buffers are blocking: they return after
 *     results are in host memory (the reference's synchronous hipMemcpy semantics,
 *     src/plssvm/backends/HIP/detail/device_ptr.hip.cpp:40-68).
 *   - "real" buffers hold float when the context was created with real_bytes == 4 and double
 *     when real_bytes == 8 (the reference's template parameter T, include/plssvm/csvm.hpp:36).
 *   - A context owns one GPU (one HIP stream). Several contexts — one per process and GPU —
 *     form a row-block partitioned group through plssvm_mi_comm_init (RCCL over xGMI).
 *   - m = n - 1 ("dept" in the reference): the last data point is eliminated by the LS-SVM
 *     reformulation (src/plssvm/csvm.cpp:230-258).
 */
#ifndef PLSSVM_MI355X_H
#define PLSSVM_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLSSVM_MI_ABI_VERSION 1

#if defined(PLSSVM_MI_BUILDING)
#define PLSSVM_MI_API __attribute__((visibility("default")))
#else
#define PLSSVM_MI_API
#endif

/* return codes */
#define PLSSVM_MI_OK 0
#define PLSSVM_MI_ERR_ARG (-1)         /* invalid argument (plssvm::exception in the reference) */
#define PLSSVM_MI_ERR_HIP (-2)         /* HIP runtime error (plssvm::hip::backend_exception)     */
#define PLSSVM_MI_ERR_RCCL (-3)        /* RCCL error                                              */
#define PLSSVM_MI_ERR_OOM (-4)         /* device allocation failed                                */
#define PLSSVM_MI_ERR_UNSUPPORTED (-5) /* unsupported kernel/format combination                   */
#define PLSSVM_MI_ERR_STATE (-6)       /* call out of order (e.g. generate_q before setup)        */
#define PLSSVM_MI_ERR_NODEV (-7)       /* "HIP backend selected but no HIP devices were found!"   */

/* kernel types: plssvm::kernel_type (include/plssvm/kernel_types.hpp:27-34) */
#define PLSSVM_MI_KERNEL_LINEAR 0
#define PLSSVM_MI_KERNEL_POLYNOMIAL 1
#define PLSSVM_MI_KERNEL_RBF 2
/* 3 (upstream's sigmoid) is not offered: PLSSVM_MI_ERR_UNSUPPORTED */
#define PLSSVM_MI_KERNEL_LAPLACIAN 4 /* exp(-gamma * ||x - z||_1); gamma as for rbf, degree and coef0 ignored; dense data only */

/* value formats of sparse feature data (build-defined; the reference has no sparse path) */
#define PLSSVM_MI_VAL_REAL 0 /* float or double, as the context's real type */
#define PLSSVM_MI_VAL_FP22 1 /* packed FP22 words, 16 values per 11 uint32 (float contexts only) */

/* K·p algorithm selection (plssvm_mi_set_option key PLSSVM_MI_OPT_KP_MODE) */
#define PLSSVM_MI_KP_AUTO 0     /* pairwise for poly/rbf, factored for linear on sparse data      */
#define PLSSVM_MI_KP_PAIRWISE 1 /* implicit pairwise tiles (MFMA on dense data)                   */
#define PLSSVM_MI_KP_FACTORED 2 /* linear kernel only: X (X^T p) + rank-1 terms, HBM-bound         */

#define PLSSVM_MI_OPT_KP_MODE 1
/* Test hook (single GPU): value = rank | (world << 16) makes this context compute only that rank's
 * share of the implicit matrix with no collective; the rank-1 Q~ terms are added by rank 0 only,
 * so the K·p results of all simulated ranks sum to the full K·p. */
#define PLSSVM_MI_OPT_SIM_RANK 2
/* RBF pair evaluation on sparse data: 0 = auto (factored e_i e_j (exp(2 g s) - 1) when g * max |x|^2
 * keeps it in floating-point range), 1 = always direct exp(-g |x_i - x_j|^2) - e_i e_j. */
#define PLSSVM_MI_OPT_RBF_FORM 3
/* K·p algorithm of the pairwise kernels (poly, rbf) on sparse data:
 *   0 = auto: the kernel expansion when it represents the kernel to rounding (poly degree <= 16; rbf
 *       in the factored form with a Taylor degree <= 16 for the data's max |2 g x_if x_jf|), else the
 *       Gram pattern; when the chosen structure's estimated size exceeds the device-memory budget
 *       (85 % of the free memory; environment PLSSVM_MI_MEM_BUDGET = bytes overrides), or its build
 *       runs out of memory, the on-the-fly path 4 or the densified path 3, whichever the setup's
 *       estimate makes faster (the on-the-fly path below a few percent density);
 *   1 = Gram pattern: every overlapping pair (j < i) with s_ij = x_i . x_j stored at setup, the kernel
 *       function re-evaluated on each per K·p (O(sum_f c_f^2) memory and traffic);
 *   2 = kernel expansion: per-feature column moments + the stored remainder of the pairs sharing two or
 *       more features (O(nnz + #multi-feature pairs)); fails with ERR_UNSUPPORTED when not eligible;
 *   3 = densified: X densified on the device, the dense MFMA pairwise tiles (O(m d) memory, every pair
 *       recomputed from the data on each K·p as in the reference); ERR_OOM when m x d does not fit;
 *   4 = on the fly: nothing stored per pair; every K·p re-forms s_ij for the pairs sharing a feature
 *       from the CSR rows and the CSC columns (O(nnz) memory + a d x m / 2048 segment table, O(sum_f
 *       c_f^2) work per K·p, as the reference recomputes every pair). */
#define PLSSVM_MI_OPT_SPARSE_ALGO 4
#define PLSSVM_MI_SPARSE_AUTO 0
#define PLSSVM_MI_SPARSE_PATTERN 1
#define PLSSVM_MI_SPARSE_EXPANSION 2
#define PLSSVM_MI_SPARSE_DENSE 3 /* densified on the device, MFMA pairwise tiles (every pair recomputed per K·p) */
#define PLSSVM_MI_SPARSE_ONTHEFLY 4 /* s_ij re-formed from the CSR / CSC per K·p, nothing stored per pair */

/* CG recurrence of plssvm_mi_solve_cg / plssvm_mi_learn:
 *   0 = the reference's (OpenMP/csvm.cpp:82-170): two dependent inner products per iteration (d.Ad, r.r), i.e. two
 *       exposed collectives in a sharded group;
 *   1 = one-reduction CG (Chronopoulos & Gear): the same iterates in exact arithmetic, the product Q~r instead of Q~d
 *       with s = Q~d carried by a recurrence, r.r and r.Q~r summed together after ONE collective per iteration; the
 *       stop test, trace and every-50th explicit residual keep the reference's meaning (tests/test_gpu_cg1.py compares
 *       its residual curves with the oracle's over 61 iterations);
 *   2 = auto: 1 in a sharded group of several ranks, else 0. */
#define PLSSVM_MI_OPT_CG_VARIANT 5
#define PLSSVM_MI_CG_REFERENCE 0
#define PLSSVM_MI_CG_ONE_REDUCTION 1
#define PLSSVM_MI_CG_AUTO 2

/* Stored kernel-matrix tiles of the dense pairwise path (also sparse data densified on the device): the first K·p of
 * a setup stores the 128 x 128 tiles of k(x_i, x_j) it forms, as many as the device memory budget holds (85 % of the
 * free memory, PLSSVM_MI_MEM_BUDGET = bytes overrides it), every later K·p streams them from HBM instead of
 * recomputing them; tiles that do not fit stay implicit. The results are bitwise those of the implicit product.
 *   0 = auto (on where it fits), 1 = off. Environment PLSSVM_MI_KP_CACHE=0, read at setup, also turns it off. */
#define PLSSVM_MI_OPT_KP_CACHE 6

/* Width of the multi-right-hand-side calls (plssvm_mi_kp_multi, _solve_cg_multi, _learn_multi): how many vectors one
 * pass over the kernel-matrix tiles serves. 0 = auto (up to 8, halved until the lanes' device memory fits beside the
 * tile cache), 1 = always one vector at a time through the single-vector code, n >= 2 = at most n (capped at 8). More
 * right-hand sides than the width run in groups, in order. plssvm_mi_info.multi_width reports the width in use. */
#define PLSSVM_MI_OPT_MULTI_WIDTH 7

/* 7-byte records for stored fp64 tiles: a 128 x 128 tile whose values are all positive normal numbers within 16
 * binades (any RBF tile unless gamma is large) is kept as 52 mantissa bits + a 4-bit exponent offset per value below a
 * per-tile base exponent, 112 KiB instead of 128 KiB, and decoded bit-exactly while it is streamed; every other tile
 * (signs, zeros, denormals, inf, NaN, a wider span) and every fp32 tile keeps its raw record. Results are bitwise the
 * same either way. A packable tile whose exponents are E - 1 and E only (E = its largest one; any tile of values in
 * [0.5, 1], say) takes the narrow form instead: 52 mantissa bits + 1 exponent bit per value, 106 KiB.
 * 0 = auto (narrow where eligible, else 7-byte, else raw), 1 = off (every record raw), 2 = 7-byte and raw only.
 * Environment, read at setup: PLSSVM_MI_KP_PACK=0 also turns packing off, PLSSVM_MI_KP_NARROW=0 means 7-byte and raw
 * only. */
#define PLSSVM_MI_OPT_KP_PACK 8

typedef struct plssvm_mi_ctx plssvm_mi_ctx;

/* Number of visible HIP devices (>= 0), or a negative error code. */
PLSSVM_MI_API int plssvm_mi_device_count(void);

/* Replaces hip::csvm<T>::csvm(const parameter<T>&) (src/plssvm/backends/HIP/csvm.hip.cpp:38-81)
 * for the parameters the hot path reads (include/plssvm/csvm.hpp:242-277): real_bytes 4|8 (T),
 * kernel, degree, gamma, coef0, cost (C). device = HIP device ordinal this context drives. */
PLSSVM_MI_API int plssvm_mi_create(int real_bytes, int kernel, int degree, double gamma, double coef0, double cost, int device,
                     plssvm_mi_ctx **out);
PLSSVM_MI_API void plssvm_mi_destroy(plssvm_mi_ctx *ctx);
PLSSVM_MI_API const char *plssvm_mi_last_error(const plssvm_mi_ctx *ctx);
PLSSVM_MI_API int plssvm_mi_set_option(plssvm_mi_ctx *ctx, int key, int64_t value);

/* Test hooks mirroring mock_hip_csvm::set_cost / set_QA_cost (tests/backends/HIP/mock_hip_csvm.hpp:24-51). */
PLSSVM_MI_API int plssvm_mi_set_cost(plssvm_mi_ctx *ctx, double cost);
PLSSVM_MI_API int plssvm_mi_set_qa_cost(plssvm_mi_ctx *ctx, double qa_cost);

/* Multi-GPU row-block group: one context per process/GPU. rank 0 calls
 * plssvm_mi_get_unique_id, the id (PLSSVM_MI_UNIQUE_ID_BYTES bytes) is shared out of band (e.g.
 * torch.distributed), every rank calls plssvm_mi_comm_init. Replaces the feature-split device
 * list + host-staged device_reduction (src/plssvm/backends/gpu_csvm.cpp:136-139,366-386). */
#define PLSSVM_MI_UNIQUE_ID_BYTES 128
PLSSVM_MI_API int plssvm_mi_get_unique_id(void *id_out);
PLSSVM_MI_API int plssvm_mi_comm_init(plssvm_mi_ctx *ctx, int rank, int world_size, const void *unique_id);

/* Host-staged group exchange: the reference's own device_reduction semantics
 * (src/plssvm/backends/gpu_csvm.cpp:366-386: synchronise, copy the partial vector to the host,
 * combine there, copy the result back) with the combine step supplied by the caller, e.g. a
 * torch.distributed / MPI / gloo collective. Every rank of the group calls it with the same
 * world_size instead of plssvm_mi_comm_init; the engine then runs exactly the multi-rank work split
 * of the RCCL path (partition -> this rank's share -> exchange -> replicated CG) but moves each
 * exchange through `fn` on the host. Use: groups without RCCL, and several ranks sharing one GPU
 * (RCCL refuses two ranks on one device) — the multi-rank path's test transport on a 1-GPU box.
 *   fn(buf, count, real_bytes, op, user) must return 0 on success and be called collectively:
 *   op == PLSSVM_MI_XCHG_ALLREDUCE: buf[count] (real_bytes-wide reals) := sum over ranks, the same
 *                                   bits on every rank;
 *   op == PLSSVM_MI_XCHG_ALLGATHER: buf[world_size * count]: rank r's chunk [r*count, (r+1)*count)
 *                                   is valid on rank r; fill every other rank's chunk. */
#define PLSSVM_MI_XCHG_ALLREDUCE 0
#define PLSSVM_MI_XCHG_ALLGATHER 1
typedef int (*plssvm_mi_exchange_fn)(void *buf, int64_t count, int real_bytes, int op, void *user);
PLSSVM_MI_API int plssvm_mi_comm_init_host(plssvm_mi_ctx *ctx, int rank, int world_size, plssvm_mi_exchange_fn fn,
                                           void *user);

/* Group failure protocol of a one-process multi-GPU group (one host thread per context, e.g. the csvm<T> adapter
 * over every visible GPU, include/plssvm_mi355x_group.hpp): when one rank's call fails, the caller aborts every
 * context of the group from its own thread — an RCCL communicator is released with ncclCommAbort, so a rank waiting
 * in a collective returns — and every call of an aborted context (also the one in progress) fails with
 * PLSSVM_MI_ERR_RCCL. The reference ends its device threads the same way: a backend_exception on any device ends the
 * OpenMP region (src/plssvm/backends/gpu_csvm.cpp:366-386). May be called from any thread, concurrently with a call
 * on the same context; the context can then only be destroyed. */
PLSSVM_MI_API int plssvm_mi_comm_abort(plssvm_mi_ctx *ctx);

/* Host-only (no GPU needed): the work split of the implicit matrix for m = n - 1 rows.
 * out4 = { first super-block, end super-block, total tiles, tiles owned by `rank` } where a tile
 * is 128x128 of the lower triangle and a super-block 8x8 tiles (linear index I(I+1)/2 + J). */
PLSSVM_MI_API int plssvm_mi_partition(int64_t m, int rank, int world_size, int64_t *out4);

/* gpu_csvm::setup_data_on_device (src/plssvm/backends/gpu_csvm.cpp:130-157) for dense data:
 * X is row-major [n][d] host memory of the context's real type (all n points, the last one
 * included, exactly the reference's data_ptr_). */
PLSSVM_MI_API int plssvm_mi_setup_dense(plssvm_mi_ctx *ctx, const void *X, int64_t n, int64_t d);

/* Sparse setup (build-defined format): CSR with int64 rowptr[n+1],
 * int32 col[nnz] ascending per row, values in val_fmt (PLSSVM_MI_VAL_REAL: real[nnz];
 * PLSSVM_MI_VAL_FP22: uint32 packed words, orc/fp22 layout). Semantics == dense setup on the
 * densified matrix (the reference parser densifies, src/plssvm/parameter.cpp:66-87).
 * A PLSSVM_MI_KERNEL_LAPLACIAN context takes dense data only: plssvm_mi_setup_csr and plssvm_mi_setup_coo return
 * PLSSVM_MI_ERR_UNSUPPORTED on it (plssvm_mi_last_error says so) and leave the context usable, e.g. for
 * plssvm_mi_setup_dense. CSR points passed to predict on a dense Laplacian model are densified per chunk as for
 * the other kernels. */
PLSSVM_MI_API int plssvm_mi_setup_csr(plssvm_mi_ctx *ctx, const int64_t *rowptr, const int32_t *col, const void *val,
                        int val_fmt, int64_t n, int64_t d);

/* Sparse setup from COO triplets (build-defined interchange format, e.g. BASELINE configs[4]):
 * int64 row[nnz], int32 col[nnz] in any order, values in val_fmt (FP22: packed in triplet order).
 * Converted on the host to CSR (rows, then columns ascending; a duplicate (row, col) is an error) and
 * then exactly plssvm_mi_setup_csr. */
PLSSVM_MI_API int plssvm_mi_setup_coo(plssvm_mi_ctx *ctx, const int64_t *row, const int32_t *col, const void *val,
                                      int val_fmt, int64_t nnz, int64_t n, int64_t d);

/* gpu_csvm::generate_q (src/plssvm/backends/gpu_csvm.cpp:160-183) + the QA_cost line of
 * csvm::learn (src/plssvm/csvm.cpp:243): q_out[m] = k(x_i, x_last); *qa_cost_out =
 * k(x_last, x_last) + 1/C. Also stores q and QA_cost in the context for plssvm_mi_kp. */
PLSSVM_MI_API int plssvm_mi_generate_q(plssvm_mi_ctx *ctx, void *q_out, double *qa_cost_out);

/* gpu_csvm::run_device_kernel + device_reduction (src/plssvm/backends/gpu_csvm.cpp:353-386):
 * ret[m] += add * Q~ p, Q~_ij = k(x_i,x_j) + QA_cost - q_i - q_j + [i==j]/C. q may be NULL to use
 * the context's q (from generate_q); otherwise q[m] is uploaded first. All host buffers. */
PLSSVM_MI_API int plssvm_mi_kp(plssvm_mi_ctx *ctx, const void *q, const void *p, void *ret, double add);

/* Test hook (the protected-for-mock parts of run_device_kernel, tests/backends/HIP/mock_hip_csvm.hpp:
 * 24-51): out[m] = one part of Q~p for host p[m], after the group exchange:
 *   PLSSVM_MI_PART_KERNEL  : sum_{j<m} k(x_i, x_j) p_j  (Q~p without the QA_cost - q_i - q_j and 1/C
 *                            terms, which are applied analytically in O(m));
 *   PLSSVM_MI_PART_OVERLAP : sparse poly/rbf only — sum over j != i sharing a feature with i of
 *                            (k_ij - kappa_ij) p_j, kappa_ij the value non-overlapping pairs take
 *                            (e_i e_j for rbf, coef0^degree for poly): exactly the per-pair work of the
 *                            sparse K·p kernels, without the separable and diagonal terms;
 *   PLSSVM_MI_PART_REMAINDER: the sparse kernel expansion only — its stored remainder stream alone,
 *                            sum over j != i sharing >= 2 features of a_i a_j H_ij p_j (H_ij = phi(s_ij) -
 *                            sum_f phi(x_if x_jf); a = e for rbf, 1 for poly) in the stored layout (bfloat16 H
 *                            and windows where the setup chose them), without the column-moment terms. */
#define PLSSVM_MI_PART_KERNEL 0
#define PLSSVM_MI_PART_OVERLAP 1
#define PLSSVM_MI_PART_REMAINDER 2
PLSSVM_MI_API int plssvm_mi_kp_part(plssvm_mi_ctx *ctx, const void *p, void *out, int part);

/* gpu_csvm::solver_CG (src/plssvm/backends/gpu_csvm.cpp:186-324) with the OpenMP backend's
 * normative semantics (src/plssvm/backends/OpenMP/csvm.cpp:82-170; including the every-50th
 * explicit residual r = b - Q~x that the reference HIP path gets wrong on one GPU). b[m], q[m]
 * (NULL = context q); x_out[m]; delta_trace (nullable, imax+1 doubles: delta0 then delta after
 * each iteration); *iters = CG iterations run. Vectors stay device-resident throughout. */
PLSSVM_MI_API int plssvm_mi_solve_cg(plssvm_mi_ctx *ctx, const void *b, const void *q, int64_t imax, double eps, void *x_out,
                       double *delta_trace, int64_t *iters);

/* Progress of plssvm_mi_solve_cg / plssvm_mi_learn — the per-iteration output of the reference's
 * solver_CG when print_info is set (src/plssvm/backends/OpenMP/csvm.cpp:115-117,161-166;
 * gpu_csvm.cpp:233-321). The CG runs on the device and the host polls it once per batch of
 * iterations (4, 8, 16, ..., then blocks of 50); after each batch fn(first, count, deltas, target,
 * batch_ms, user) is called with the batch's iterations [first, first + count) (0-based),
 * deltas[0..count] = r^T r before iteration `first`, ..., after the batch's last iteration,
 * target = eps^2 delta0 (the stop bound) and the batch's wall time in ms. fn == NULL: no calls.
 * The callback must not call back into the context. */
typedef void (*plssvm_mi_progress_fn)(int64_t first, int64_t count, const double *deltas, double target,
                                      double batch_ms, void *user);
PLSSVM_MI_API int plssvm_mi_set_progress(plssvm_mi_ctx *ctx, plssvm_mi_progress_fn fn, void *user);

/* Stepwise CG on the same device state (used by bench.py to time single iterations):
 * begin = x0 = 1, r = b - Q~x, d = r; step runs n iterations (ignores convergence when
 * force != 0); result copies x and the trace out. */
PLSSVM_MI_API int plssvm_mi_cg_begin(plssvm_mi_ctx *ctx, const void *b, const void *q, double eps, double *delta0_out);
PLSSVM_MI_API int plssvm_mi_cg_step(plssvm_mi_ctx *ctx, int64_t n, int force, int64_t *iters_done, int *converged);
PLSSVM_MI_API int plssvm_mi_cg_result(plssvm_mi_ctx *ctx, void *x_out, double *delta_trace, int64_t trace_len, int64_t *iters);

/* csvm<T>::learn (src/plssvm/csvm.cpp:207-267) on the context's data: y[n] labels (+-1),
 * imax < 0 means num_features (the reference's imax, csvm.cpp:256). alpha_out[n] (alpha[m] =
 * -sum), *bias_out (rho = -bias), delta_trace (nullable, imax+1). */
PLSSVM_MI_API int plssvm_mi_learn(plssvm_mi_ctx *ctx, const void *y, int64_t imax, double eps, void *alpha_out, double *bias_out,
                    double *delta_trace, int64_t *iters);

/* Several right-hand sides at once (build-defined; the reference trains one binary problem per solve): the K
 * one-vs-all systems of a K-class problem share Q~ and differ only in b, so on the pairwise tile path of a single
 * GPU every CG iteration visits each kernel-matrix tile once for all of them (plssvm_mi_info.multi_width >= 2).
 * Everywhere else (stored sparse paths, the factored linear path, groups, simulated ranks, the one-reduction CG, or
 * too little free device memory for two lanes) the same calls run the vectors one after another. Either way every
 * column is BITWISE what the single-vector call returns for it, whatever the width, grouping or tile-cache state.
 * All matrices are row-major with one vector per row and leading dimension ld: vector c starts at base + c * ld
 * reals; ld >= m (>= n for the label and alpha matrices); elements past m (n) of a row are never read or written.
 * nrhs / nclass < 1, a NULL buffer or a too small ld: PLSSVM_MI_ERR_ARG. nrhs == 1 equals the single call. The
 * progress callback is not called by these entry points.
 *
 * plssvm_mi_kp_multi: RET_c += add * Q~ P_c for c < nrhs; each row as plssvm_mi_kp (q NULL = the context's q). */
PLSSVM_MI_API int plssvm_mi_kp_multi(plssvm_mi_ctx *ctx, const void *q, const void *P, void *RET, int64_t nrhs, int64_t ld,
                                     double add);
/* plssvm_mi_solve_cg_multi: plssvm_mi_solve_cg for the right-hand sides B[nrhs][ld] (q NULL = the context's q):
 * X_out[nrhs][ld]; delta_trace nullable, [nrhs][imax + 1], row c filled up to iters[c]; iters[nrhs] (nullable). Every
 * right-hand side keeps its own alpha, beta, delta, stop test and iteration count; one that has converged is frozen
 * while the others go on, and the call returns when all have converged or imax is reached. */
PLSSVM_MI_API int plssvm_mi_solve_cg_multi(plssvm_mi_ctx *ctx, const void *B, int64_t nrhs, int64_t ld, const void *q,
                                           int64_t imax, double eps, void *X_out, double *delta_trace, int64_t *iters);
/* plssvm_mi_learn_multi: plssvm_mi_learn per class of a one-vs-all label matrix Y[nclass][ldy], ldy >= n, row c
 * holding +1 for the points of class c and -1 for all others. Per class exactly plssvm_mi_learn's arithmetic
 * (b = y - y_m, the bias, alpha[m] = -sum): alpha_out[nclass][ldy], bias_out[nclass] (nullable), delta_trace
 * (nullable, [nclass][imax + 1]; with imax < 0: [nclass][num_features + 1]), iters[nclass] (nullable). The class with
 * the largest decision value bias_c + sum_i alpha_ci k(x_i, z) is the prediction (plssvm_mi_predict_multi_*: every
 * class's decision values in one call). */
PLSSVM_MI_API int plssvm_mi_learn_multi(plssvm_mi_ctx *ctx, const void *Y, int64_t nclass, int64_t ldy, int64_t imax,
                                        double eps, void *alpha_out, double *bias_out, double *delta_trace,
                                        int64_t *iters);
/* Point weights (build-defined; LIBSVM's -wi as a vector): point i is trained at cost C * s_i. In the LS-SVM system
 * only the diagonal changes: row i's 1/C becomes (1/C) * (1/s_i) and QA_cost = k(x_m, x_m) + (1/C) * (1/s_m), both
 * reciprocals and their product rounded in the real type, so s_i = 1 everywhere gives bitwise the unweighted results.
 * s: n reals of the context's type (the last point included), all finite and > 0; NULL clears the weights. They apply
 * to plssvm_mi_kp, _kp_multi, _solve_cg*, _cg_begin / _cg_step, _learn and _learn_multi (every class the same
 * weights) until they are cleared; any plssvm_mi_setup_* clears them, plssvm_mi_set_cost does not. With a q in place
 * the context's QA_cost is formed anew as above (a value from plssvm_mi_set_qa_cost is replaced). Before a setup, or
 * with an entry that is not finite and > 0: PLSSVM_MI_ERR_ARG, the context's weights unchanged. In a group every
 * rank's context gets the same call. */
PLSSVM_MI_API int plssvm_mi_set_point_weights(plssvm_mi_ctx *ctx, const void *s);
/* Lanes that differ in their diagonal: lane k is plssvm_mi_learn on the labels Y[k] (rows ldy >= n apart) at cost
 * costs[k] (costs NULL: the context's cost) with the point weights S[k] (rows lds >= n apart; lds == 0: S is one row
 * that every lane shares; S NULL: the context's weights, if any). A cost grid is nlane copies of one label row with
 * nlane costs; one-vs-all with weighted positives is plssvm_mi_learn_multi's Y with one weight row per class. The
 * lanes share each pass over the kernel matrix exactly where plssvm_mi_learn_multi's classes do (and run one after
 * another elsewhere); lane k is BITWISE plssvm_mi_set_cost(costs[k]), plssvm_mi_set_point_weights(S[k]),
 * plssvm_mi_learn(Y[k]). Outputs as plssvm_mi_learn_multi's. The context's own cost and weights are what they were
 * when the call returns. nlane < 1, ldy < n, 0 < lds < n, a cost or a weight that is not finite and > 0:
 * PLSSVM_MI_ERR_ARG. plssvm_mi_learn_multi is this call with costs = S = NULL. */
PLSSVM_MI_API int plssvm_mi_learn_lanes(plssvm_mi_ctx *ctx, const void *Y, int64_t nlane, int64_t ldy, const double *costs,
                                        const void *S, int64_t lds, int64_t imax, double eps, void *alpha_out,
                                        double *bias_out, double *delta_trace, int64_t *iters);
/* Held-out points as lanes (k-fold cross-validation; build-defined): plssvm_mi_learn_lanes whose lane k also leaves
 * out the points i with HOLD[k * ldh + i] != 0 (rows of n flags, ldh >= n apart; ldh == 0: one row serves every lane;
 * HOLD NULL: this is plssvm_mi_learn_lanes). In this order, the contract:
 *  1. The system. Lane k trains on T_k = the points not held out. With its pivot t (2.) and R_k = T_k \ {t} it solves
 *     the principal submatrix on R_k of Q~_ij = k_ij + QA - q_i - q_j + delta_ij diag_i, q_i = k(x_i, x_t),
 *     QA = k_tt + diag_t, right-hand side b_i = y_i - y_t, by the reference CG from x0 = 1 on R_k; then
 *     alpha_t = -sum alpha, bias = y_t + QA sum alpha - sum_i q_i alpha_i: plssvm_mi_learn on the subset T_k.
 *  2. The pivot t is the lane's largest training index (pivots[k], nullable output of nlane entries). t = n - 1 unless
 *     the lane holds the last point out; such lanes share one extra product K e_t that yields their q.
 *  3. alpha_out[k][i] is exactly 0 on every held-out point i.
 *  4. A lane is BITWISE the call with that lane alone at PLSSVM_MI_OPT_MULTI_WIDTH = 1, whatever its position, the
 *     other lanes, the width or the tile cache.
 *  5. A lane whose hold row is all zero is BITWISE plssvm_mi_learn_lanes' lane (alpha, bias, iterations, trace).
 *  6. Offered where the lanes share a pass over the kernel matrix: dense data (or sparse data on the densified path)
 *     with the pairwise tile kernels, on one GPU, with the reference CG. A stored sparse setup, the factored linear
 *     path, a group, a simulated rank or the one-reduction CG with a non-NULL HOLD: PLSSVM_MI_ERR_UNSUPPORTED,
 *     plssvm_mi_last_error names the setup, the context stays usable.
 * Other arguments and outputs as plssvm_mi_learn_lanes': row k of delta_trace is filled up to iters[k], as
 * plssvm_mi_solve_cg_multi fills it, and not written beyond. 0 < ldh < n, or a lane with fewer than two training points:
 * PLSSVM_MI_ERR_ARG. The context's cost, weights and q are what they were when the call returns. */
PLSSVM_MI_API int plssvm_mi_learn_held(plssvm_mi_ctx *ctx, const void *Y, int64_t nlane, int64_t ldy, const double *costs,
                                       const void *S, int64_t lds, const uint8_t *HOLD, int64_t ldh, int64_t imax,
                                       double eps, void *alpha_out, double *bias_out, double *delta_trace, int64_t *iters,
                                       int64_t *pivots);
/* Decision values of nclass models on the context's own n points (training and held-out alike):
 * OUT[c][i] = bias[c] + sum_j ALPHA[c][j] k(x_j, x_i), i < n; ALPHA[nclass][lda], OUT[nclass][ldo], lda, ldo >= n. One
 * pass over the kernel matrix per group of models where the lanes are batched, one per model elsewhere (dense and
 * sparse setups, every K.p path, on one GPU); no point is uploaded or prepared again. Row c is bitwise the same whatever
 * nclass, its position and the width. A context of a group (plssvm_mi_comm_init*) or with a simulated rank holds only
 * its share of the product: PLSSVM_MI_ERR_UNSUPPORTED, the context stays usable. If the context's q is not the one
 * plssvm_mi_generate_q forms (a caller's q from plssvm_mi_kp / _solve_cg), it is generated anew and replaces it; QA_cost
 * is kept. */
PLSSVM_MI_API int plssvm_mi_train_values(plssvm_mi_ctx *ctx, const void *ALPHA, int64_t nclass, int64_t lda,
                                         const double *bias, void *OUT, int64_t ldo);
/* Timing hook: plssvm_mi_time_kp's K·p time for the product with nrhs resident vectors (in groups of the width; one at
 * a time where nothing is batched), averaged over `reps` products, measured with hipEvents on the context's stream. */
PLSSVM_MI_API int plssvm_mi_time_kp_multi(plssvm_mi_ctx *ctx, int64_t nrhs, int reps, double *ms_per_kp);

/* gpu_csvm::update_w (src/plssvm/backends/gpu_csvm.cpp:327-350; OpenMP csvm.cpp:174-190):
 * w_out[d] = sum_i alpha_i x_i over all n points of the context's data (alpha[n], e.g. from
 * plssvm_mi_learn, alpha[m] included). Linear kernel model vector. */
PLSSVM_MI_API int plssvm_mi_update_w(plssvm_mi_ctx *ctx, const void *alpha, void *w_out);

/* gpu_csvm::predict (src/plssvm/backends/gpu_csvm.cpp:52-120; OpenMP csvm.cpp:193-240):
 * out[p] = bias + sum_i alpha_i k(x_i, z_p) for np points with d features (linear: w . z_p + bias),
 * the context's data being the model's support vectors. Dense points: Z row-major [np][d] of the
 * real type. Sparse points (_csr): int64 rowptr[np+1], int32 col, values in val_fmt. np == 0 is a
 * no-op; a feature-count mismatch fails with the reference's message. bias = -rho. */
PLSSVM_MI_API int plssvm_mi_predict_dense(plssvm_mi_ctx *ctx, const void *alpha, double bias, const void *Z, int64_t np,
                                          int64_t d, void *out);
PLSSVM_MI_API int plssvm_mi_predict_csr(plssvm_mi_ctx *ctx, const void *alpha, double bias, const int64_t *rowptr,
                                        const int32_t *col, const void *val, int val_fmt, int64_t np, int64_t d,
                                        void *out);

/* The same for nclass models on the same support vectors (the one-vs-all classes of plssvm_mi_learn_multi), with
 * the matrix conventions of the _multi block above: ALPHA[nclass][lda] and OUT[nclass][ldo] hold one class per row,
 * lda >= n, ldo >= np, elements past n (np) of a row are never read (written); bias[nclass]. nclass < 1, a NULL
 * buffer or a too small leading dimension: PLSSVM_MI_ERR_ARG (the context stays usable); np == 0 is a no-op.
 * Dense data with the polynomial / rbf kernel runs the fused tile kernel (csrc/predict_tiles.hip): the kernel values
 * of a (support-vector tile, point tile) pair are formed once on MFMA, never written to memory, and multiplied with
 * every class's alpha (up to 8 classes per pass over the tiles). The linear w path and sparse data prepare and
 * upload the points once per call and serve up to 8 classes per pass over the support vectors: the expansion's
 * per-point walk and merge, the brute-force sweep's dot products and kernel values, and the linear path's points are
 * shared, only the products with a class's coefficients run per class, each in the single call's order. The
 * fallback from the expansion to brute force depends on the points and the model's data alone and is taken for all
 * classes together. plssvm_mi_predict_dense / _csr are the nclass = 1 case of these calls.
 * Contract: the decision value of (class c, point z) depends only on the model (the support vectors, alpha_c,
 * bias_c, the kernel parameters) and on z. It does not depend on nclass, on the class's position among the
 * classes, on np, on the point's position in the call, on the chunking of the points, or on the run: row c of OUT is
 * BITWISE what plssvm_mi_predict_dense / _csr return for (alpha_c, bias_c), for any subset or order of the points.
 * Environment, read per call: PLSSVM_MI_PRED_GEMM=1 selects the rocBLAS GEMM + epilogue path for dense poly / rbf
 * (once per class; the A/B baseline; ignored for the Laplacian kernel, which has no GEMM form and always runs the
 * fused tile kernel), PLSSVM_MI_PRED_CHUNK=<points> overrides the number of points per upload,
 * PLSSVM_MI_PRED_SEQ=1 runs the classes of the linear and sparse paths one after another, each with its own point
 * preparation (the A/B baseline of the shared pass; the same bits). */
PLSSVM_MI_API int plssvm_mi_predict_multi_dense(plssvm_mi_ctx *ctx, const void *ALPHA, int64_t nclass, int64_t lda,
                                                const double *bias, const void *Z, int64_t np, int64_t d, void *OUT,
                                                int64_t ldo);
PLSSVM_MI_API int plssvm_mi_predict_multi_csr(plssvm_mi_ctx *ctx, const void *ALPHA, int64_t nclass, int64_t lda,
                                              const double *bias, const int64_t *rowptr, const int32_t *col,
                                              const void *val, int val_fmt, int64_t np, int64_t d, void *OUT,
                                              int64_t ldo);
/* How the last predict call ran: out[0] = classes served per pass over the support vectors (1 when the classes ran
 * one after another, 0 before any call), out[1] = number of times the call uploaded the points. */
PLSSVM_MI_API int plssvm_mi_get_predict_stats(const plssvm_mi_ctx *ctx, int64_t out[2]);

/* plssvm_mi_info.predict_algo: the path the last predict call of the context took */
#define PLSSVM_MI_PREDICT_NONE 0      /* no predict call yet */
#define PLSSVM_MI_PREDICT_LINEAR 1    /* w . z + bias */
#define PLSSVM_MI_PREDICT_GEMM 2      /* dense poly / rbf: rocBLAS G = X Z^T + epilogue (PLSSVM_MI_PRED_GEMM) */
#define PLSSVM_MI_PREDICT_TILES 3     /* dense poly / rbf: the fused MFMA tile kernel; dense laplacian: its VALU twin */
#define PLSSVM_MI_PREDICT_EXPANSION 4 /* sparse poly / rbf: the kernel expansion */
#define PLSSVM_MI_PREDICT_BRUTE 5     /* sparse poly / rbf: every support vector entry per 64 points */
/* support-vector tiles (of tile_rows rows) per workgroup segment of the fused predict kernel */
#define PLSSVM_MI_PREDICT_SEG_TILES 16

/* Timing hook (bench.py): runs `reps` K·p launches (+ reduction/collective) on resident device
 * buffers (p = a fixed device vector) and reports the average device time per K·p and per
 * dominant-kernel launch, measured with hipEvents on the context's stream. */
PLSSVM_MI_API int plssvm_mi_time_kp(plssvm_mi_ctx *ctx, int reps, double *ms_per_kp, double *ms_dominant_kernel);

/* Introspection for roofline accounting: number of pairwise tiles / work units per K·p on this
 * rank, tile edge, padded sizes, bytes of device memory held. */
typedef struct {
    int64_t n, d, m, n_pad, d_pad, nnz;
    int64_t tiles_total, tiles_local, tile_rows, tile_cols;
    int64_t device_bytes;
    int64_t pairs; /* sparse pairwise kernels: stored overlapping pairs (j < i) of this rank */
    int kp_mode, rank, world_size, real_bytes, kernel, is_sparse, val_fmt;
    int rbf_factored;   /* sparse rbf: 1 = factored pair form in use (PLSSVM_MI_OPT_RBF_FORM) */
    int64_t pair_slots; /* sparse pairwise kernels: stored pair slots incl. padding (K·p stream) */
    int64_t spmv_bytes; /* sparse factored linear: HBM bytes both SpMV passes move per K·p (padded SELL
                           stream, slot maps, panel partials) */
    int rbf_small_args; /* sparse factored rbf: 1 = every 2 g |s_ij| is below the short Taylor form's bound */
    int sparse_algo;    /* sparse poly/rbf: PLSSVM_MI_SPARSE_PATTERN | _EXPANSION | _DENSE (0 otherwise) */
    int exp_terms;      /* kernel expansion: polynomial degree K of the per-feature pair function */
    int exp_waves;      /* kernel expansion: waves of the remainder stream */
    int64_t exp_chunks; /* kernel expansion: 4-slot chunks of the remainder stream (this rank's rows); 0 = run layout */
    int exp_hbytes;     /* kernel expansion: bytes of a stored remainder value (2 = bfloat16 under the precision
                           bound of expand_setup.hip "H storage", else sizeof(real)) */
    int exp_layout;     /* kernel expansion: remainder stream layout — 1 = 4-slot chunks with a stored row index per
                           chunk, 2 = 4-slot chunks whose rows are numbered by row-start flags (no row index),
                           4 = row-start flags per slot pair (cells padded to 2 slots); 0 = no expansion
                           (3 was round 2's run layout, removed) */
    int exp_dot2;       /* kernel expansion, bfloat16 H: 1 = the remainder's chunk products run on the v_dot2_f32_bf16
                           kernel (built with EXP_DOT2 and selected: PLSSVM_MI_EXP_DOT2 != 0), 0 = the FMA chain */
    int centered;       /* kernel expansion: 1 = the finalize forms Q~'s rank-1 terms in the centered form
                           (engine.hpp ctr_*; PLSSVM_MI_CTR=0 or a caller's own q vector: 0) */
    int exp_lt;         /* kernel expansion: 1 = the remainder's rows came from the lower-triangle join + transpose
                           (one rank holding every row; PLSSVM_MI_EXP_LT=0: the full join) */
    int64_t kp_cache_tiles; /* pairwise tile path: tiles of this rank whose kernel values are kept in HBM
                               (PLSSVM_MI_OPT_KP_CACHE); tiles_local when all fit, 0 = none */
    int64_t kp_cache_bytes; /* device bytes of those records (tile_rows x tile_cols reals each) */
    int multi_width;        /* vectors the next multi-right-hand-side call serves per pass over the tiles
                               (PLSSVM_MI_OPT_MULTI_WIDTH); 1 = not batched: one vector at a time */
    int64_t kp_cache_packed_tiles; /* of kp_cache_tiles: tiles stored at 7 bytes per value (PLSSVM_MI_OPT_KP_PACK);
                                      0 before the first K·p of a setup has filled the cache; read back from the
                                      device on the first request after that */
    int predict_algo;              /* PLSSVM_MI_PREDICT_*: the path of the context's last predict call */
    int rbf_shift;                 /* 1: dense RBF data, the device holds x - c (c = the training data's column means,
                                      rounded to the real type) and shifts every predict point alike; k(x, z) and every
                                      result are those of the caller's features. Read-only */
} plssvm_mi_info;
PLSSVM_MI_API int plssvm_mi_get_info(const plssvm_mi_ctx *ctx, plssvm_mi_info *info);
/* Of plssvm_mi_info.kp_cache_packed_tiles: the tiles stored at 53 bits per value (the narrow form of
 * PLSSVM_MI_OPT_KP_PACK). 0 before the first K·p of a setup has filled the cache; read back from the device together
 * with kp_cache_packed_tiles on the first request after that. An entry point of its own because plssvm_mi_info keeps
 * its size and its last fields (tests/test_predict_multi_abi.py pins them). */
PLSSVM_MI_API int plssvm_mi_get_kp_cache_narrow_tiles(const plssvm_mi_ctx *ctx, int64_t *narrow_tiles);
/* The plans of the factored sparse-linear K·p as the setup built them (csrc/spmv.hpp; read-only, nothing selects a
 * regime): out[0..5] the CSC pass w = X^T p, out[6..11] the CSR pass raw = X w, each {P panels, ldsx (1 = 16-bit
 * indices into LDS panels, 0 = one panel of 32-bit global indices), W panel width in elements, nblocks workgroups,
 * nchunks 64-slot chunks, f22 (1 = packed FP22 value stream)}; out[12..15] the row-block CSR pass of the one-GPU CG
 * with the finalize fused, {P, W, RBK rows per workgroup, nblk workgroups} (nblk = 0: not built, the CG sums the CSR
 * pass's panel slabs in its finalize). All zeros when the context is not a factored sparse one. An entry point of
 * its own because plssvm_mi_info keeps its size. */
PLSSVM_MI_API int plssvm_mi_get_spmv_plan(const plssvm_mi_ctx *ctx, int64_t out[16]);

#ifdef __cplusplus
}
#endif

#endif /* PLSSVM_MI355X_H */
