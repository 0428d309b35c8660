// Launcher declarations for the MI355X PLSSVM hot-path kernels (implemented in *.hip).
#pragma once

#include <vector>

#include "common.hpp"

namespace plssvm_mi {

// kernel parameters of the LS-SVM kernel function (include/plssvm/kernel_types.hpp:63-85)
// exp(-gamma ||x - z||_1): not a function of x . z, so the dense tile kernels accumulate L1 distances on the VALU
// instead of a Gram block on MFMA (kp_tiles.hip, predict_tiles.hip). Dense data only; PLSSVM_MI_KERNEL_LAPLACIAN
constexpr int KF_LAPLACIAN = 4;
template <typename T>
struct kfun {
    int kernel;  // 0 linear, 1 polynomial, 2 rbf, KF_LAPLACIAN
    int degree;
    T gamma;
    T coef0;
};

// device-resident CG scalars (all CG scalars live on the GPU; the host only polls `converged`)
template <typename T>
struct cg_scalars {
    T delta, delta0, alpha, beta, sp, sqp, eps2delta0, dAd;
    T delta_prev;  // delta of the previous iteration (fused CG kernels: read while delta is rewritten)
    T g1[2], a1[2], d1[2];  // one-reduction CG, by iteration parity: r.r (+inf before the first), alpha, d.Q~d (0)
    int converged;
    int force;  // bench mode: never converge (same work per iteration)
    int64_t iters;
};

// The diagonal of Q~ as the finalize kernels take it: the scalar 1/C, or — with point weights s —
// 1/C beside the rows' 1/s_i. Each finalize kernel is a template on this type: the scalar instance is the kernel as it
// always was (same arguments, same code), the row_diag instance reads sinv[i] beside q[i]. (1/C)(1/s_i) is rounded in
// T before it meets p_i; s_i = 1 gives 1/C exactly.
template <typename T>
struct row_diag {
    T cost_inv;
    const T *sinv;  // the kernel's own row range (offset like q)
};
template <typename T>
__host__ __device__ __forceinline__ T diag_at(T cost_inv, int64_t) {
    return cost_inv;
}
template <typename T>
__host__ __device__ __forceinline__ T diag_at(const row_diag<T> &dg, int64_t i) {
    return dg.cost_inv * dg.sinv[i];
}
// Held rows (k-fold cross-validation): a lane that trains on a subset solves the principal submatrix
// of Q~ on its active rows. hold[i] != 0 removes row i: the finalize kernels store T(0) there (also where they add to
// what is stored) and the row adds nothing to the d.Ad partials; with the vectors zero off the active rows the columns
// are gone as well. An active row runs the row_diag arithmetic (sinv null: the scalar's), so its bits are those of the
// other two instances.
template <typename T>
struct row_diag_held {
    T cost_inv;
    const T *sinv;        // nullable
    const uint8_t *hold;  // the kernel's own row range (offset like q)
};
template <typename T>
__host__ __device__ __forceinline__ T diag_at(const row_diag_held<T> &dg, int64_t i) {
    return dg.sinv != nullptr ? dg.cost_inv * dg.sinv[i] : dg.cost_inv;
}
template <typename T>
__host__ __device__ __forceinline__ bool held_at(T, int64_t) {
    return false;
}
template <typename T>
__host__ __device__ __forceinline__ bool held_at(const row_diag<T> &, int64_t) {
    return false;
}
template <typename T>
__host__ __device__ __forceinline__ bool held_at(const row_diag_held<T> &dg, int64_t i) {
    return dg.hold[i] != 0;
}

// ---- dense pairwise tiles -----------------------------------------------------------------------
// tile edge of the implicit Q~ tiles (rows and columns); n_pad is a multiple of this.
constexpr int KP_TILE = 128;
// K-chunk depth of the pairwise tile kernel: 8 (fp64) / 16 (fp32) keeps LDS at <= 49 KB for 3
// workgroups per CU. The Laplacian instances (VALU K loop, 2 fp64 workgroups per CU: 70 KB each) take 16 in both types:
// their next chunk's DMA is issued behind the chunk's last LDS reads and its latency shows at the chunk barrier, so a
// deeper chunk halves how often
template <typename T, int KERNEL>
constexpr int kp_bk() { return (sizeof(T) == 8 && KERNEL != KF_LAPLACIAN) ? 8 : 16; }
// feature padding of the device layout: a multiple of every chunk depth
template <typename T>
constexpr int kp_dpad() { return 16; }

// XT[k][i] = X[i][k] for i < rows, k < d (X row-major [rows][d]); XT is [>=d][n_pad], pre-zeroed
template <typename T>
void launch_transpose(const T *X, int64_t rows, int64_t d, T *XT, int64_t n_pad, hipStream_t s);

// X[i][k] -= c[k] for i < rows, k < d (X row-major [rows][d]): the dense RBF contexts' shift
template <typename T>
void launch_shift_rows(T *X, int64_t rows, int64_t d, const T *c, hipStream_t s);

// row norms ||x_i||^2 (sequential fma chain in feature order) for the RBF norm trick
template <typename T>
void launch_row_norms(const T *XT, int64_t n_pad, int64_t d, T *norms, hipStream_t s);

// q_i = k(x_i, x_last), i < m (device_kernel_q_*, include/plssvm/backends/HIP/q_kernel.hip.hpp:32-83)
template <typename T>
void launch_q_dense(kfun<T> kf, const T *XT, int64_t n_pad, int64_t d, int64_t m, const T *xlast, T *q,
                    hipStream_t s);

// Tiles are scheduled in KP_SUPER x KP_SUPER super-blocks of the lower triangle (super-block
// (SI, SJ), SI >= SJ, linear index tri_index(SI, SJ)); a rank owns a contiguous super-block range.
constexpr int KP_SUPER = 8;

// slab record of one tile: its 128 row sums, then its 128 column sums (the rank's slab: wgs records)
constexpr int KP_REC = 2 * KP_TILE;
// partial[wg][KP_REC]: per tile wg of super-blocks [s0, s0+nsuper), sum_{j in J} k(x_i,x_j) p_j for i in I
// and sum_{i in I} k(x_i,x_j) p_i for j in J
// wg_off[k] (k = 0..nsuper): first workgroup of super-block s0 + k (one workgroup per real tile: 64 for a
// full super-block, 36 for a diagonal one, fewer in the ragged last row); wgs = wg_off[nsuper]
void kp_tile_offsets(int64_t nb, int64_t s0, int64_t nsuper, std::vector<int32_t> &wg_off);
// Modes of the tile kernel. The kernel values depend only on the data and the kernel parameters, so after the
// first K·p of a setup they can come from HBM instead of the MFMAs: KP_COMPUTE_STORE writes tile wg's 128 x 128
// values to kcache[wg][KP_CACHE_REC] (the lanes' register layout, kp_tiles.hip), KP_LOAD reads them back and
// runs the same epilogue, giving bitwise the computed slab record.
enum kp_tile_mode { KP_COMPUTE = 0, KP_COMPUTE_STORE = 1, KP_LOAD = 2 };
constexpr int64_t KP_CACHE_REC = (int64_t) KP_TILE * KP_TILE;
// The rank's tiles: kernel function, data, the super-blocks [s0, s0 + nsuper) and their workgroup table.
template <typename T>
struct kp_geom {
    kfun<T> kf;
    const T *XT, *norms;
    int64_t n_pad, d_pad, nb, s0, nsuper;
    const int32_t *wg_off;
    int64_t wgs;
};
// The tile cache as a launch sees it: tiles [0, cached) have a record in rec. fp64 records come in three forms
// (kp_record.hpp): desc[tile] says raw (0), or holds the largest exponent E of a wide tile (7 bytes per value, the first
// 112 KiB of its record), or E | KP_DESC_NARROW for a narrow one (53 bits per value, the first 106 KiB); the fill writes
// it (pack 0: every tile raw, 1: raw or wide, 2: all three) and adds one to count[0] per packed tile of either form and
// one to count[1] per narrow tile, KP_LOAD reads it. desc and count are needed whenever cached > 0 in fp64 (the batched
// launch: desc only); fp32 ignores them.
template <typename T>
struct kp_cache_view {
    T *rec = nullptr;
    int32_t *desc = nullptr, *count = nullptr;
    int64_t cached = 0;
    int pack = 0;
};
// tiles [0, cached) from / to the cache (fill: computed and stored, else loaded), tiles [cached, wgs) computed.
template <typename T>
void launch_kp_tiles(const kp_geom<T> &g, const T *p, T *partial, const cg_scalars<T> *status, hipStream_t s,
                     const kp_cache_view<T> &kc = {}, bool fill = false);

// The same tiles for nvec vectors at once (2 .. KP_MULTI_W; 1 is legal): vector c is p + c * pstride, its slab
// partial + c * sstride, its stop flag status[c] (status null: none; a vector whose flag says converged is skipped and
// its slab left alone). A tile's kernel values are formed or streamed once per visit and multiplied with every
// vector in the single-vector kernel's order: slab c is bitwise launch_kp_tiles' slab for p_c. Tiles [0, cached) are
// streamed from the cache, whose records must be filled (launch_kp_tiles with fill), the rest are computed.
constexpr int KP_MULTI_W = 8;
template <typename T>
void launch_kp_tiles_multi(const kp_geom<T> &g, const T *p, int64_t pstride, T *partial, int64_t sstride, int nvec,
                           const cg_scalars<T> *status, hipStream_t s, const kp_cache_view<T> &kc = {});

// ---- fused dense predict tiles (predict_tiles.hip) -------------------------------------------------
// One workgroup owns a 128-point tile and one segment of PRED_SEG consecutive 128-row support-vector tiles. The
// segment length is a compile-time constant: it fixes the summation order of a decision value, which therefore
// depends only on the model and the point (not on the number of points or classes, the chunking or the run).
constexpr int PRED_SEG = 16;
inline int64_t predict_segments(int64_t nb) { return (nb + PRED_SEG - 1) / PRED_SEG; }
// part[c][segment][p] = sum over the segment's support vectors j (tile after tile) of A[c][j] k(x_j, z_p) for the
// ncls <= KP_MULTI_W classes A[ncls][n_pad] (zero from row m on) and the points ZT[d_pad][np_pad] (feature-major,
// zero padded; znorms: their squared norms, rbf only). part is [ncls][predict_segments(nb)][np_pad]; polynomial
// and rbf kernels only; the point tiles covering points [0, npoints) are computed. The kernel values are formed once
// per tile on MFMA and never leave the registers.
template <typename T>
void launch_predict_tiles(kfun<T> kf, const T *XT, const T *norms, int64_t n_pad, int64_t nb, int64_t d_pad,
                          const T *ZT, const T *znorms, int64_t np_pad, int64_t npoints, const T *A, int ncls, T *part,
                          hipStream_t s);
// out[c][p] = ((sum_s part[c][s][p], in segment order) + ab[c] k(xlast, z_p)) + ab[nclass + c] for c < ncls, p < np;
// out is [ncls][np_pad]. ab = the classes' alpha[m], then their biases (nclass each; the caller offsets it to the
// first class of part)
template <typename T>
void launch_predict_finish(kfun<T> kf, const T *part, int64_t nseg, const T *ZT, const T *znorms, int64_t np_pad,
                           int64_t d, const T *xlast, T nlast, const T *ab, int ncls, int nclass, int64_t np, T *out,
                           hipStream_t s);

// raw[i] = sum over the column blocks c in order of row i's slab values of the tiles whose super-block lies
// in [s0, s1) (tile (Ib, c) row sums for c <= Ib, tile (c, Ib) column sums for c > Ib); i < m
template <typename T>
void launch_kp_reduce(const T *partial, int64_t nb, int64_t m, int64_t s0, int64_t s1, const int32_t *wg_off, T *raw,
                      const cg_scalars<T> *status, hipStream_t s);

// ret[i] = (overwrite ? 0 : ret[i]) + add * (raw[i] + (QA - q_i) * sum(p) - sum(q p) + p_i / C)
// raw may alias ret only when overwrite is false and ... (never aliased by callers).
// sinv non-null (point weights): the row_diag instance, p_i / C becomes ((1/C) sinv_i) p_i
// hold non-null (held rows): the row_diag_held instance, ret[i] = T(0) where hold[i] != 0 (overwrite or not)
template <typename T>
void launch_kp_finalize(const T *raw, const T *q, const T *p, const cg_scalars<T> *sc, T QA_cost, T cost_inv,
                        const T *sinv, const uint8_t *hold, T add, int overwrite, int64_t m, T *ret,
                        const cg_scalars<T> *status, hipStream_t s);

// ---- linear factored path: Q~p = X_m (X_m^T p) + rank-1 terms --------------------------------------
template <typename T>
void launch_gemv_t(const T *XT, int64_t n_pad, int64_t d, int64_t r0, int64_t r1, const T *p, T *w,
                   const cg_scalars<T> *status, hipStream_t s);  // w[k] = sum_{r0<=i<r1} XT[k][i] p_i
template <typename T>
void launch_gemv_n(const T *XT, int64_t n_pad, int64_t d, int64_t r0, int64_t r1, const T *w, T *raw,
                   const cg_scalars<T> *status, hipStream_t s);  // raw[i] = sum_k XT[k][i] w_k, r0<=i<r1

// ---- BLAS-1 / CG --------------------------------------------------------------------------------
constexpr int RED_BLOCKS = 512;
// partials[b] for b < RED_BLOCKS; out = sum(a*b) (b == nullptr: sum(a)); second pair optional
template <typename T>
void launch_dot2(const T *a, const T *b, const T *c, const T *e, int64_t n, T *partials, const cg_scalars<T> *status,
                 hipStream_t s);
// final reductions with CG scalar updates; `what` selects the update (see blas1.hip)
enum final_op { FIN_SP_SQP = 0, FIN_DELTA0 = 1, FIN_ALPHA = 2, FIN_DELTA = 3, FIN_PLAIN = 4 };
// G > 1: G gathered partial sets of a sharded group (rank-major, summed in rank order per partial)
template <typename T>
void launch_dot_final(const T *partials, cg_scalars<T> *sc, int op, int64_t run, double *trace, int64_t trace_cap,
                      T *plain_out, hipStream_t s, int G = 1);
template <typename T>
void launch_cg_init(const T *b, int64_t m, T *x, T *r, hipStream_t s);
// the same with held rows: x = 1 where hold[i] == 0 and 0 elsewhere; r = b (the caller's b is 0 on held rows)
template <typename T>
void launch_cg_init_held(const T *b, const uint8_t *hold, int64_t m, T *x, T *r, hipStream_t s);
// Decision values of the training points from raw_i = sum_{j < m} k_ij alpha_j (the K·p's raw part):
// out_i = raw_i + q_i alpha_m + bias for i < m, q_i = k(x_i, x_m). The last point's value, sum_j q_j alpha_j +
// k_mm alpha_m + bias, is the caller's: engine::train_values sums it on the host as an fma chain in index order, like
// learn_tail's q . alpha.
template <typename T>
void launch_train_values_fin(const T *raw, const T *q, T alpha_m, T bias, int64_t m, T *out, hipStream_t s);
template <typename T>
void launch_copy(const T *src, int64_t n, T *dst, const cg_scalars<T> *status, hipStream_t s);
// x += alpha d; if !reset: r -= alpha Ad  else r = b
template <typename T>
void launch_cg_update(T *x, T *r, const T *d, const T *Ad, const T *b, int reset, int64_t m, const cg_scalars<T> *sc,
                      hipStream_t s);
// d = beta d + r
template <typename T>
void launch_cg_direction(T *d, const T *r, int64_t m, const cg_scalars<T> *sc, hipStream_t s);
// Fused CG steps. Each block first sums the previous step's RED_BLOCKS partial pairs itself (in
// dot_final_kernel's order: every block gets the same value), so no final-reduction launch sits
// between them; dots keep dot2_kernel's grid and order, so the results are bitwise those of the
// unfused sequence.
// The input partials (psum, pdad, prr) are G gathered sets in a sharded group (G = 1 otherwise); the
// vectors are the caller's element range (pointers offset to it, m = its length).
// Ad = Q~ d from raw (kp_finalize arithmetic, add = 1, overwrite), sum d / sum q d from psum;
// d.Ad partials -> pdad. slabs != null: raw = the P panel slabs [P][sstride] of an unreduced SpMV pass.
template <typename T>
void launch_cg_fin_dad(const T *raw, const T *slabs, int64_t P, int64_t sstride, const T *q, const T *d, const T *psum,
                       int G, T QA_cost, T cost_inv, const T *sinv, const uint8_t *hold, int raw_only, int64_t m, T *Ad,
                       T *pdad, cg_scalars<T> *sc, hipStream_t s);  // sinv non-null: the row_diag instance; hold non-null:
                                                                    // row_diag_held, Ad = 0 and no d.Ad term on held rows
// alpha = delta / d.Ad (pdad); x += alpha d; r -= alpha Ad and r.r partials -> prr (reset: r = b)
template <typename T>
void launch_cg_upd_rr(T *x, T *r, const T *d, const T *Ad, const T *b, int reset, const T *pdad, int G, int64_t m,
                      T *prr, cg_scalars<T> *sc, hipStream_t s);
// delta = r.r (prr), stop test, beta; d = beta d + r (init: d = r, scalars untouched);
// sum d / sum q d partials -> psum. The iteration index is sc->iters (trace[iters + 1] = delta, iters += 1).
// wout non-null (kernel expansion with bfloat16 windows, round 5): the next K·p's first kernel rides along — w = e d
// (e null: w = d, not written), its bfloat16 copy and the S partials (cw non-null: the centered S_c), in
// exp_wown_kernel's grid, element order and block reduction (bitwise its partials)
template <typename T>
struct dir_w_t {
    const T *e;
    T *w;
    uint16_t *w16;
    const T *cw;
    T *spart;
};
// one-reduction CG (Chronopoulos-Gear, blas1.hip): the update of iteration k from the gathered [r.u | r.r] partials
// (pset, G sets), the residual sums of a new r, the r.r of a batch's last r (poll)
template <typename T>
void launch_cg1_update(T *x, T *r, T *d, T *s, const T *u, const T *b, const T *q, int reset, const T *pset, int G,
                       double *trace, int64_t trace_cap, int64_t m, int par, T *pnext, T *psum, cg_scalars<T> *sc,
                       hipStream_t st, const dir_w_t<T> *wout);
template <typename T>
void launch_cg1_rsums(const T *r, const T *s, const T *q, int64_t m, T *pnext, T *psum, cg_scalars<T> *sc, hipStream_t st,
                      const dir_w_t<T> *wout);
template <typename T>
void launch_cg1_delta(const T *pset, int G, double *trace, int64_t trace_cap, cg_scalars<T> *sc, hipStream_t st);
template <typename T>
void launch_cg_dir_sums(T *d, const T *r, const T *q, const T *prr, int G, int init, double *trace, int64_t trace_cap,
                        int64_t m, T *psum, cg_scalars<T> *sc, hipStream_t s, const dir_w_t<T> *wout = nullptr);

// ---- sparse (CSR / FP22) ------------------------------------------------------------------------
// declared in sparse.hpp

}  // namespace plssvm_mi
