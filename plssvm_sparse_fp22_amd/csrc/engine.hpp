// Per-GPU engine behind the C ABI: device memory, one HIP stream, optional RCCL communicator,
// device-resident CG. One engine<T> per context; T = float | double (the reference's real_type).
#pragma once

#include <rccl/rccl.h>
#include <rocblas/rocblas.h>

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "buffer.hpp"
#include "kernels.hpp"
#include "sparse.hpp"

namespace plssvm_mi {

template <typename T>
inline ncclDataType_t nccl_type() {
    return sizeof(T) == 8 ? ncclFloat64 : ncclFloat32;
}

// an RCCL call of an engine member: under comm_mu, refused once plssvm_mi_comm_abort has released the communicator
#define MI_NCCL_CHECK(expr)                                                                                          \
    do {                                                                                                             \
        ncclResult_t r_;                                                                                             \
        {                                                                                                            \
            std::lock_guard<std::mutex> lk_(this->comm_mu);                                                         \
            if (this->comm_aborted) throw ::plssvm_mi::mi_error(-3, "the group was aborted by another rank");      \
            r_ = (expr);                                                                                             \
        }                                                                                                            \
        if (r_ != ncclSuccess) {                                                                                     \
            throw ::plssvm_mi::mi_error(-3, std::string("RCCL error '") + ncclGetErrorString(r_) + "' (" #expr ")"); \
        }                                                                                                            \
    } while (0)

int exp_dot2_built();  // expand.hip: 1 if the bfloat16 remainder's dot-instruction kernel was compiled (EXP_DOT2)
void exp_load_code_object();  // expand.hip and expand_setup.hip: their code objects loaded (a kernel's attributes queried)
void partition_superblocks(int64_t nb, int rank, int world, int64_t &s0, int64_t &s1, int64_t &s_total,
                           int64_t &tiles_total, int64_t &tiles_local);

struct engine_base {
    virtual ~engine_base() = default;
    // plssvm_mi_comm_abort (another thread of a one-process multi-GPU group, after a peer failed): the communicator
    // is aborted (ncclCommAbort releases a rank waiting in a collective) and every later RCCL call of the engine
    // fails (MI_NCCL_CHECK); the C ABI reports any call that ran into the abort as failed
    std::mutex comm_mu;
    std::atomic<bool> comm_aborted{ false };
    virtual void comm_abort() = 0;
};

template <typename T>
struct engine : engine_base {
    // ---- parameters (csvm<T> protected state, include/plssvm/csvm.hpp:242-277) ----
    int kernel = 0, degree = 3;
    T gamma = 1, coef0 = 0, cost = 1;
    int device = 0;
    hipStream_t stream = nullptr;
    int kp_mode = 0;  // PLSSVM_MI_KP_*
    int rbf_form = 0;  // PLSSVM_MI_OPT_RBF_FORM
    int sparse_algo = 0;  // PLSSVM_MI_OPT_SPARSE_ALGO (0 auto, 1 Gram pattern, 2 kernel expansion, 3 dense, 4 on the fly)

    // ---- multi-GPU row-block group ----
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;
    void comm_abort() override;
    // host-staged exchange (plssvm_mi_comm_init_host): the reference's device_reduction transport
    int (*xchg)(void *, int64_t, int, int, void *) = nullptr;
    void *xchg_user = nullptr;
    std::vector<T> xbuf;
    // test hook: compute only rank sim_rank's share of a sim_world group, no collective, rank-1
    // terms only on sim rank 0 (so the shares of all sim ranks sum to the full K·p)
    int sim_rank = 0, sim_world = 0;

    // ---- data ----
    bool have_data = false, sparse = false;
    int64_t n = 0, d = 0, m = 0, n_pad = 0, d_pad = 0, nb = 0;
    std::vector<T> xlast_h;
    dev_buf<T> XT, norms, xlast;  // dense: XT[d_pad][n_pad]
    // dense RBF data: the features go to the device as x - shift (in T), shift = the column means of the first m
    // points, summed in fp64 in row order and rounded to T — the same on every (simulated) rank, rebuilt by every
    // setup. XT, xlast, xlast_h and every uploaded predict point carry it; the caller never sees it
    bool shifted = false;
    std::vector<T> shift_h;
    dev_buf<T> shift;
    csr_data<T> csr;              // sparse

    // work split
    int64_t t_total = 0, t0 = 0, t1 = 0;  // pairwise tile super-blocks owned by this rank: [t0, t1) of t_total
    int64_t tiles_total = 0, tiles_local = 0;
    dev_buf<int32_t> kp_wgoff;  // tile kernel workgroup table (kp_tile_offsets), kp_wgs workgroups
    int64_t kp_wgs = 0;
    void tiles_upload();
    // Stored kernel-matrix tiles of the pairwise tile path (kp_tiles.hip, KP_COMPUTE_STORE / KP_LOAD): the values
    // k(x_i, x_j) depend only on the data and the kernel parameters, so the first K·p of a setup that runs without
    // a stop flag (cg_begin's r0 product, kp_host) stores the first kc.tiles tiles of this rank's table — all
    // of them where mem_budget() allows — and every later K·p streams them instead of recomputing them; the tiles
    // past the prefix stay implicit.
    struct tile_cache {
        // the two options outlive a setup; reset() leaves them alone
        int cache_opt = 0;  // PLSSVM_MI_OPT_KP_CACHE: 0 auto (on where it fits), 1 off; env PLSSVM_MI_KP_CACHE=0: off
        int pack_opt = 0;   // PLSSVM_MI_OPT_KP_PACK: 0 auto (fp64: narrow where eligible, else wide, else raw), 1 off,
                            // 2 wide only; env at setup: PLSSVM_MI_KP_PACK=0 off, PLSSVM_MI_KP_NARROW=0 wide only
        dev_buf<T> rec;
        int64_t tiles = 0;
        bool valid = false;  // the records are written (by launches already on the stream)
        // Packed records (kp_record.hpp): one descriptor per cached tile — raw, or the tile's largest exponent, flagged
        // for the narrow form — written by the fill, read by every KP_LOAD workgroup; desc[tiles] counts the packed tiles
        // of both forms, desc[tiles + 1] the narrow ones. Allocated and dropped with the records. fp32 records are
        // never packed.
        dev_buf<int32_t> desc;
        int pack = 0;              // this setup's fill: 0 every tile raw, 1 raw or wide, 2 all three forms
        int64_t packed_host = -1;  // the counters, read back together on the first request after the fill (-1: not yet)
        int64_t narrow_host = 0;
        void reset();
        void setup(const engine &e);  // after the setup's other allocations
        int64_t packed(const engine &e);
        int64_t narrow(const engine &e) { return packed(e) > 0 ? narrow_host : 0; }
        int64_t bytes() const { return rec.bytes() + desc.bytes(); }
        // what the launchers see: the first `tiles` records once filled (or while `filling`), else none
        kp_cache_view<T> view(bool filling = false) const {
            return { rec.get(), desc.get(), desc.get() + tiles, (valid || filling) ? tiles : 0, pack };
        }
    };
    tile_cache kc;
    kp_geom<T> kp_geometry() const {
        return { kf(), XT.get(), norms.get(), n_pad, d_pad, nb, t0, t1 - t0, kp_wgoff.get(), kp_wgs };
    }
    void kp_tiles_now(const T *p, const cg_scalars<T> *status);  // the tile launches of one K·p
    int64_t r0 = 0, r1 = 0, chunk = 0;    // rows owned by this rank (factored / sparse row paths)

    // sharded CG (a real group on sparse data by default; PLSSVM_MI_SHARD = 0 / 1 overrides, 1 also for dense
    // data and simulated ranks): each rank updates only its rows [v0, v0 + vn) of x, r, d, Ad; every dot is
    // summed from the G ranks' gathered partials in rank order (the same bits everywhere); a K·p input the
    // path needs whole is gathered first, a path's full-length partial result reduce-scattered
    bool shard = false;
    bool gathered = false;  // sharded in a real group (any size, also a one-rank RCCL group): partials and
                            // inputs move through the group's transport
    int64_t v0 = 0, vn = 0;
    int G = 1;
    dev_buf<T> cgp_g;      // gathered partials, slots [5][G][2 RED_BLOCKS]: sum d / sum q d, d.Ad, r.r, kp sums, S
    std::vector<T> xpart;  // host staging of the host exchange's partial gathers
    const T *gather_partials(T *local, int slot, int64_t K = 2 * RED_BLOCKS);  // K values per rank
    // RCCL group: the sum d / sum q d partials of a CG step ride with the next collective of the K·p
    // (one launch, one latency) instead of a collective of their own
    bool psum_pending = false;
    void psum_group_begin(hipStream_t s);
    void psum_group_end();
    void flush_psum();
    // second stream for collectives that overlap kernels of the same K·p (kernel expansion, sharded RCCL group)
    hipStream_t cstream = nullptr;
    hipEvent_t cev[4] = { nullptr, nullptr, nullptr, nullptr };
    void gather_input(const T *p);   // sharded group: p's rows of every rank, in place
    void reduce_scatter_rows(T *buf);  // sharded group: own rows of the sum over ranks

    // ---- vectors (n_pad, zero padded) ----
    dev_buf<T> partial, q, pv, ret, x, r, dv, Ad, b, raw, w, red;
    // kernel expansion with bfloat16 windows (round 5): the S partials of the w pass (exp_wown_kernel, or the direction
    // update that carries it: dir_w_fill); w_pre = the vector whose w, bfloat16 copy and S partials are in place
    // (set after a carrying direction update of dv, cleared by any other w pass), graph_w_end = w_pre after a
    // captured iteration block
    dev_buf<T> wsp;
    const T *w_pre = nullptr, *graph_w_end = nullptr;
    bool dir_w_fill(dir_w_t<T> &o);
    dev_buf<T> cgp;  // fused CG partials: [0, 2R) sum d / sum q d, [2R, 4R) d.Ad, [4R, 6R) r.r
    // one-reduction CG (blas1.hip cg1_*; PLSSVM_MI_OPT_CG_VARIANT): s = Q~d by recurrence (sv), u = Q~r in Ad, and two
    // partial sets [r.u | r.r] by iteration parity (cg1p), gathered by one collective per iteration
    int cg_variant = 2;  // PLSSVM_MI_CG_REFERENCE / _ONE_REDUCTION / _AUTO (default: one-reduction in sharded groups)
    bool cg1 = false;    // the running solve uses it (cg_begin)
    int cg_par = 0;      // parity of the iteration cg_iter forms
    dev_buf<T> sv, cg1p;
    bool cg1_wanted() const;
    void cg1_iter(int reset);
    dev_buf<cg_scalars<T>> sc;
    dev_buf<double> trace;
    int64_t trace_cap = 0;
    T QA_cost = 0;
    bool have_q = false;
    int64_t run = 0;
    bool cg_active = false;
    static constexpr int CG_RESET = 50;  // r = b - Q~x every 50th iteration (csvm.cpp:119-132)
    hipGraphExec_t cg_graph = nullptr;   // one captured block of CG_RESET iterations (graph_block)
    // a CG iteration's finalize (Ad, d.Ad partials) offered to the K·p: a path that can form it in its own last
    // kernel (the kernel expansion's combine) does so and sets kp_fin_done; cg_product launches it otherwise
    struct kp_fin_t {
        const T *q, *d, *psum;
        int G;
        T QA_cost, cost_inv;
        const T *sinv;  // point weights: 1/s_i beside q (whole length), else null
        T *Ad, *pdad;
    };
    const kp_fin_t *kp_fin_req = nullptr;
    bool kp_fin_done = false;
    // Centered rank-1 terms (round 5, kernel expansion): with k_ij = a_i a_j (kappa' + phi_ij) (rbf: a = e, kappa' = 1;
    // poly: a = 1, phi = c, the kappa terms cancel exactly) the finalize's QA_cost - q_i - q_j + the separable part
    // is (a_i - a_m)(a_j - a_m) kappa' - h_i - h_j + h_m with h_i = a_i a_m phi(x_i . x_m): the same Q~, but formed
    // from small quantities instead of O(1) kernel values that cancel to O(gamma |x|^2) — in fp32 the naive sum loses
    // ~log10(1 / (gamma |x|^2)) digits per K·p (tests/long_trace_cases.py). Inside a finalize-bound K·p the combine's
    // base is c_i S_c (c = a - a_m, S_c = sum_j cw_j w_j, cw = c / e) and the finalize runs with q -> h,
    // QA_cost -> h_m + 1/C (+ any difference of a caller's QA_cost from k_mm + 1/C).
    dev_buf<T> ctr_c, ctr_cw, ctr_h;
    double ctr_hm = 0;
    T ctr_kmm = 0;         // k(x_m, x_m) as generate_q's QA_cost has it
    bool ctr_ok = false;   // the vectors are built and finite (PLSSVM_MI_CTR=0: never)
    bool q_gen = false;    // the device q is the engine's own k(x_i, x_m)
    bool ctr_now = false;  // set by kp_device / cg_product around their K·p: the expansion drops its separable base
    std::vector<T> q_gen_h;
    bool ctr_active() const;
    const T *qf() const { return ctr_active() ? ctr_h.get() : q.get(); }
    T QAf() const;
    T k_mm() const;  // k(x_m, x_m) on the host, as generate_q's QA_cost has it
    void ctr_setup();
    cg_scalars<T> polled{};               // the CG scalars read by the last cg_step poll
    // plssvm_mi_set_progress: called by solve_cg after each polled batch of iterations
    void (*progress)(int64_t, int64_t, const double *, double, double, void *) = nullptr;
    void *progress_user = nullptr;

    engine(int kernel_, int degree_, double gamma_, double coef0_, double cost_, int device_);
    ~engine() override;

    kfun<T> kf() const { return kfun<T>{ kernel, degree, gamma, coef0 }; }
    T cost_inv() const { return T(1) / cost; }
    // ---- point weights (plssvm_mi_set_point_weights): cost C s_i for point i ----
    // Only the diagonal of Q~ changes: row i's 1/C becomes (1/C)(1/s_i), QA_cost = k_mm + (1/C)(1/s_m); both
    // reciprocals and their product are rounded in T, so s = 1 gives 1/C exactly. sinv_h: the n reciprocals (empty =
    // no weights), sinv: the first m of them on the device, zero padded like q. Any setup clears them.
    std::vector<T> sinv_h;
    dev_buf<T> sinv;
    bool weighted() const { return !sinv_h.empty(); }
    const T *sinv_dev() const { return weighted() ? sinv.get() : nullptr; }
    T diag_m() const { return weighted() ? cost_inv() * sinv_h[(size_t) m] : cost_inv(); }  // the last point's diagonal
    void set_sinv(const std::vector<T> &sinv_new);          // the reciprocals (n, or empty: none); QA_cost follows
    void set_point_weights(const T *s);                    // s[n], null clears
    bool factored() const;
    void need_data() const;
    void need_dense_kernel_data() const;  // the sparse setups' first check: throws on a kernel that takes dense data only
    void need_q() const;

    void comm_init(int rank_, int world_, const void *uid);
    void comm_init_host(int rank_, int world_, int (*fn)(void *, int64_t, int, int, void *), void *user);
    void kp_part(const T *p_host, T *out_host, int part);  // test hook, PLSSVM_MI_PART_*
    int part_mode = 0;  // kp_part in progress: PLSSVM_MI_PART_* (the expansion's combine writes that part)
    void setup_dense(const T *X, int64_t n_, int64_t d_);
    void setup_csr(const int64_t *rowptr, const int32_t *col, const void *val, int val_fmt, int64_t n_, int64_t d_);
    void finish_setup();
    void generate_q(T *q_out, double *qa_out);
    void set_q(const T *q_host);

    // out = (overwrite ? 0 : out) + add * Q~ p  (device vectors, length >= m)
    void kp_device(const T *p, T *out, T add, bool overwrite, const cg_scalars<T> *status);
    void kp_raw(const T *p, const cg_scalars<T> *status);  // raw = the pairwise / sparse part of Q~ p
    // kp_raw of a host vector (m values) or, p_host null, of the unit vector e_t (t < 0: of zero), through sc and pv
    void kp_raw_of(const T *p_host, int64_t t = -1, int part = 0);
    void kp_host(const T *q_host, const T *p, T *ret_host, T add);

    // ---- one right-hand side's device state, and the steps of K·p and CG on it ----
    // A non-owning view: the engine's own vectors (own_lane: the single solve) or lane c of the pool below
    // (pool_lane). The single solve and a batched group are the same step functions on different views.
    struct cg_lane {
        // the lane's diagonal: 1/C, the QA_cost that goes with it (the centred one where ctr_active()), and the rows'
        // 1/s_i (null: no point weights) — what kp_fin, cg_fin_dad and cg_product hand to the finalize kernels; hold: the
        // lane's held-row flags (null: none; learn_held), read by kp_fin, cg_fin_dad and the lane's init
        T cost_inv, QA;
        const T *sinv;
        const uint8_t *hold;
        T *x, *r, *d, *Ad, *b, *raw;
        T *cgp;   // 6 RED_BLOCKS: sum d / sum q d, then d.Ad, then r.r
        T *red;   // 2 RED_BLOCKS: the K·p sums and delta0
        T *slab;  // tile records of the last K·p (tile path)
        cg_scalars<T> *sc;
        double *trace;
        int64_t trace_cap;
        T *pdad() const { return cgp + 2 * RED_BLOCKS; }
        T *prr() const { return cgp + 4 * RED_BLOCKS; }
    };
    cg_lane own_lane() const {
        return { cost_inv(), QAf(), sinv_dev(), hold_cur, x.get(), r.get(), dv.get(), Ad.get(), b.get(), raw.get(), cgp.get(),
                 red.get(), partial.get(), sc.get(), trace.get(), trace_cap };
    }
    cg_lane pool_lane(int c) const {
        const lane_diag &dg = lanes.diag[(size_t) c];
        return { dg.cost_inv, dg.QA, dg.sinv, dg.hold, lane_v(LV_X, c), lane_v(LV_R, c), lane_v(LV_D, c), lane_v(LV_AD, c),
                 lane_v(LV_B, c), lane_v(LV_RAW, c), lane_cgp(c), lane_red(c),
                 lanes.slab.get() + (int64_t) c * lanes.sstride, lanes.sc.get() + c,
                 lanes.trace.get() + (int64_t) c * lanes.trace_cap, lanes.trace_cap };
    }
    // The steps take the rows [v0, v0 + vn), sum the G ranks' partials (gather_partials) and use qf() / QAf() /
    // dir_w_fill as the single solve needs them in a group, sharded or on the stored sparse paths. For a pool lane
    // all of that is the identity — multi_batched(): the tile path on one rank, no shard, no simulated rank, the
    // reference recurrence, so v0 = 0, vn = m, G = 1, gather_partials returns its argument, ctr_active() and
    // dir_w_fill() are false (need_pool checks it at the batched entry points). status: the stop flag the kernels
    // leave at, nullptr = none.
    void kp_sums(const T *p, const cg_lane &L, const cg_scalars<T> *status);  // sum p, sum q p -> L.sc (through L.red)
    void kp_slab_reduce(const cg_lane &L, const cg_scalars<T> *status);       // L.slab -> L.raw
    // out = (overwrite ? 0 : out) + add * Q~ p from L.raw and L.sc's sums (a group's shared first product: the
    // engine's own raw and sc with a pool lane's p and out)
    void kp_fin(const cg_lane &L, const T *p, T *out, T add, bool overwrite, const cg_scalars<T> *status);
    // Ad = Q~ v from raw (or P panel slabs) with the v.Ad partials in pd: v = d, pd = pdad (one-reduction CG: r, its set)
    void cg_fin_dad(const cg_lane &L, const T *v, T *pd, const T *slabs, int64_t P);
    void cg_product(const T *v, T *pd);  // the engine's own K·p of v on its path, then (or fused with) cg_fin_dad
    void cg_upd_rr(const cg_lane &L, int reset);                   // alpha; x, r update; r.r partials
    void cg_rr(const cg_lane &L, const cg_scalars<T> *status);     // r.r partials of an explicit residual
    void cg_delta0(const cg_lane &L);                              // delta0 = r.r, trace[0]
    void cg_dir(const cg_lane &L, int init);  // stop test, beta, d = beta d + r (init: d = r); sum d / sum q d
    static cg_scalars<T> cg_scalars_init(T eps, bool force);
    // iterations until the next host poll: 4, 8, 16, ... up to the first reset, then blocks of CG_RESET
    static int64_t poll_batch(int64_t done, int64_t imax, int64_t &batch);

    void cg_begin(const T *b_host, const T *q_host, T eps, bool force, double *delta0_out, int64_t trace_len);
    void cg_iter(int reset);
    bool graph_usable() const;
    void graph_capture();
    void graph_block();
    void graph_reset();
    void cg_step(int64_t nsteps, bool &converged, int64_t &iters);
    void cg_result(T *x_out, double *trace_out, int64_t trace_len, int64_t *iters);
    void solve_cg(const T *b, const T *q_host, int64_t imax, T eps, T *x_out, double *trace_out, int64_t *iters);
    void learn(const T *y, int64_t imax, T eps, T *alpha_out, double *bias_out, double *trace_out, int64_t *iters);
    void time_kp(int reps, double *ms_kp, double *ms_dom);

    // ---- several right-hand sides over one pass of the tiles (lanes.hip) ----
    // Systems that share the kernel matrix — one-vs-all classes (they differ in b), a cost grid or weighted classes (in
    // the diagonal), folds (in the rows they leave out) — run their CG solves as lanes: a lane is one right-hand side's
    // device state (x, r, d, Ad, b, raw, its partials, cg_scalars, trace and tile slab) and its lane_diag.
    // Each iteration makes ONE pass over the tiles for the live lanes' direction vectors (launch_kp_tiles_multi) and
    // then runs the step functions above on each lane's view (pool_lane) — the very functions cg_begin and cg_iter
    // run on own_lane() — so every lane's x, trace and iteration count are bitwise solve_cg's on that right-hand
    // side alone by construction. lane_v / lane_cgp / lane_red and LV_* are for pool_lane and the strided base of the
    // batched tile launch only. The single-solve members above are not touched by a batched group except sc, red,
    // raw and partial (the shared first product Q~ x0, x0 = 1).
    // Batched: the pairwise tile path on one rank (multi_batched); everywhere else, and when not even two lanes fit
    // in device memory, the same entry points run the right-hand sides one after another through solve_cg / kp_host.
    struct lane_diag {
        T cost_inv, QA;
        const T *sinv;
        const uint8_t *hold;
    };
    struct lane_pool {
        // every lane's diagonal (cg_lane), set by the batched entry points before they run a group: the engine's own
        // (lanes_own_diag) or the lane's cost, weights and hold rows (learn_held, from its lane_plan)
        std::vector<lane_diag> diag;
        dev_buf<T> sinv;                   // [width][vstride] per-lane 1/s_i: allocated by the first call that passes
                                           // per-lane weights (need_lane_buf), never for lanes that differ in C only
        dev_buf<uint8_t> hold;             // [width][vstride] per-lane held-row flags: allocated by the first learn_held
                                           // call that passes them (need_lane_buf)
        int width = 0;                     // lanes allocated: 0 = not yet, 1 = none fit (one at a time)
        int64_t vstride = 0, sstride = 0;  // elements between two lanes' vectors / slabs
        dev_buf<T> vec;                    // [LV_COUNT][width][vstride], zero padded like the engine's vectors
        dev_buf<T> slab;                   // [width][sstride = kp_wgs * KP_REC]
        dev_buf<T> part;                   // [width][8 RED_BLOCKS]: a lane's cgp (6 R), then its red (2 R)
        dev_buf<cg_scalars<T>> sc;         // [width]
        dev_buf<double> trace;             // [width][trace_cap]
        int64_t trace_cap = 0;
        int64_t bytes() const {
            return vec.bytes() + slab.bytes() + part.bytes() + sc.bytes() + trace.bytes() + sinv.bytes() + hold.bytes();
        }
    };
    enum lane_vec { LV_X = 0, LV_R, LV_D, LV_AD, LV_B, LV_RAW, LV_COUNT };
    lane_pool lanes;
    int multi_opt = 0;  // PLSSVM_MI_OPT_MULTI_WIDTH: 0 auto, 1 one at a time, n >= 2 at most n lanes
    T *lane_v(int kind, int c) const { return lanes.vec.get() + ((int64_t) kind * lanes.width + c) * lanes.vstride; }
    T *lane_cgp(int c) const { return lanes.part.get() + (int64_t) c * 8 * RED_BLOCKS; }
    T *lane_red(int c) const { return lane_cgp(c) + 6 * RED_BLOCKS; }
    // where the lanes' steps are the single solve's (the tile path on one rank with the reference CG): held-out lanes
    // are offered there; batched there unless multi_opt == 1 (and given memory for two lanes)
    bool held_supported() const;
    bool multi_batched() const;
    // device memory of one lane (with_sinv: and its weight vector; with_hold: and its held-row flags)
    int64_t lane_bytes(bool with_sinv = false, bool with_hold = false) const;
    // the width the next multi call would use (1: one at a time); allocates nothing
    int multi_width_next(bool with_sinv = false, bool with_hold = false) const;
    // the lanes, allocated at the first call (width halved until it fits)
    int multi_lanes(bool with_sinv = false, bool with_hold = false);
    // a per-lane buffer (lanes.sinv, lanes.hold) of an allocated pool, allocated on first need; false: no room for it
    template <typename U>
    bool need_lane_buf(dev_buf<U> &buf);
    T *lane_sinv(int c) const { return lanes.sinv.get() + (int64_t) c * lanes.vstride; }
    uint8_t *lane_hold(int c) const { return lanes.hold.get() + (int64_t) c * lanes.vstride; }
    // The batched launch streams filled records only: if the tile cache is allocated and unfilled, `product` (a K·p of
    // the caller's choice on the single path, after sc is zeroed) fills it; true if it ran
    template <typename F>
    bool fill_tiles(F product) {
        if (kc.tiles <= 0 || kc.valid) return false;
        MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
        product();
        return true;
    }
    void lanes_own_diag();                // every lane: the engine's own cost, QA_cost and weights
    void need_pool();                     // the steps' group / shard / centring handling is the identity here
    void tiles_multi(int kind, int c0, int nvec, bool flags);  // one pass over the tiles for lanes [c0, c0 + nvec)
    // vectors `kout` of lanes [c0, c0 + nvec) = (overwrite ? 0 : kout) + add * Q~ (vectors `kin`): kp_sums per lane, one
    // pass over the tiles, kp_slab_reduce and kp_fin per lane (then_rr: and cg_rr, the reset's r.r of the new
    // residual); flags: the lanes' stop flags apply
    void kp_lanes(int kin, int kout, int c0, int nvec, T add, bool overwrite, bool flags, bool then_rr = false);
    void cg_iter_multi(int nvec, int reset);
    // held: the lanes' diag carries hold rows — x0 is the lane's own (1 on its active rows), so the first residual goes
    // through kp_lanes per lane instead of the shared first product
    void solve_cg_group(const T *B, int nvec, int64_t ld, int64_t imax, T eps, T *X_out, double *trace_out, int64_t *iters,
                        bool held = false);
    void solve_cg_multi(const T *B, int64_t nrhs, int64_t ld, const T *q_host, int64_t imax, T eps, T *X_out,
                        double *trace_out, int64_t *iters);
    void kp_multi(const T *q_host, const T *P, T *RET, int64_t nrhs, int64_t ld, T add);
    // ---- the multi-lane learn (plssvm_mi_learn_multi / _learn_lanes / _learn_held) ----
    // Lane k = learn on the labels Y[k] at cost costs[k] (null: the engine's) with the point weights S[k] (null: the
    // engine's; lds == 0: S is one row for all lanes), leaving out the points with HOLD[k * ldh + i] != 0 (ldh == 0: one
    // row for all lanes; HOLD null: no lane is masked, and every setup serves the call). The host half is a lane_plan
    // (lane_plan.hpp): every argument check, before anything moves; per lane its cost, weight row, hold row and pivot t =
    // its largest training index (m without hold rows), which takes the last point's part: q = column t of the kernel
    // matrix (t < m: one K·e_t over the tiles, shared by the lanes of that pivot), QA = k_tt + diag_t, b = y - y_t; the
    // rows i with hold_i or i >= t are masked (lane_diag::hold / hold_cur). The lanes run grouped by pivot, pivot m first,
    // and are returned in the caller's order; pivots_out (nullable) gets t per lane. Batched where multi_batched() and
    // the per-lane buffers fit, else one after another on own_lane() with the engine's cost, weights and hold_cur set per
    // lane — the same steps, the same bits. Without hold rows the lanes share the first product Q~ x0 and run the
    // unmasked kernel instances; with them each lane's x0 is its own. Held lanes are offered where held_supported()
    // (else ERR_UNSUPPORTED, after the argument checks). One restore rule: the call records what it moved of the
    // engine's cost, QA_cost, weights, q and hold_cur and undoes exactly that on every exit, thrown or not, resetting
    // the captured CG graph only if a value a captured block holds was moved — learn_multi without weights moves nothing.
    const uint8_t *hold_cur = nullptr;  // own_lane()'s held-row flags (set by learn_held around a single solve)
    dev_buf<uint8_t> hold_own;
    void learn_held(const T *Y, int64_t nlane, int64_t ldy, const double *costs, const T *S, int64_t lds,
                    const uint8_t *HOLD, int64_t ldh, int64_t imax, T eps, T *alpha_out, double *bias_out,
                    double *trace_out, int64_t *iters, int64_t *pivots_out);
    void learn_lanes(const T *Y, int64_t nlane, int64_t ldy, const double *costs, const T *S, int64_t lds, int64_t imax,
                     T eps, T *alpha_out, double *bias_out, double *trace_out, int64_t *iters) {
        learn_held(Y, nlane, ldy, costs, S, lds, nullptr, 0, imax, eps, alpha_out, bias_out, trace_out, iters, nullptr);
    }
    // learn() per class of a one-vs-all label matrix Y[nclass][ldy] (+-1): lanes that differ in b only
    void learn_multi(const T *Y, int64_t nclass, int64_t ldy, int64_t imax, T eps, T *alpha_out, double *bias_out,
                     double *trace_out, int64_t *iters) {
        learn_lanes(Y, nclass, ldy, nullptr, nullptr, 0, imax, eps, alpha_out, bias_out, trace_out, iters);
    }
    // OUT[c][i] = sum_j k(x_i, x_j) ALPHA[c][j] + bias[c] for every point i < n of the setup (the model's decision values
    // on its own training points, held-out ones included): one pass over the tiles per group of up to the width
    // vectors where multi_batched(), else one vector after another through kp_part's code; then train_values_fin. The
    // last point's sum is a host fma chain in index order. Row c is bitwise the same whatever nclass, position or width.
    // One GPU: a simulated rank or a group is ERR_UNSUPPORTED. A q that is not the generated one is generated anew (a
    // caller's q is replaced, QA_cost is kept).
    void train_values(const T *ALPHA, int64_t nclass, int64_t lda, const double *bias, T *OUT, int64_t ldo);
    void time_kp_multi(int64_t nrhs, int reps, double *ms_kp);

    // sparse paths (sparse.hip)
    void sparse_q();                                              // q, norms, e on CSR data
    void build_gram_blocks(const int64_t *cpos, int64_t max_inc);  // sparse Gram pattern (pairwise kernels)
    int64_t mem_budget() const;  // device bytes for stored per-pair structures (sparse paths, dense tile cache)
    // row_stats (optional): the sampled rows' partners sharing >= 2 features, mean and max
    int64_t estimate_expansion_bytes(const int64_t *rowptr, const int32_t *col, const std::vector<int64_t> &colptr,
                                     const std::vector<int32_t> &crow, int64_t inc_total, double *row_stats = nullptr) const;
    void release_sparse_structures();
    void csc_device(int64_t nnz, dev_buf<int64_t> &cpos_d);  // csr.colptr / crow / cval and cpos on the device
    void setup_sparse_dense();                                     // densified fallback (PLSSVM_MI_SPARSE_DENSE)
    // on-the-fly path (otf.hip, PLSSVM_MI_SPARSE_ONTHEFLY): estimated seconds per K·p share, setup, K·p
    double otf_estimate_s(const int64_t *rowptr, const int32_t *col, const std::vector<int64_t> &colptr) const;
    void setup_otf(int rbf_fact_ok);
    void otf_dominant(const T *p, const cg_scalars<T> *status);
    void otf_kp_raw(const T *p, const cg_scalars<T> *status, bool with_base);
    bool sparse_stored() const { return sparse && !csr.dense_on; } // K·p through the CSR structures
    bool expansion_eligible();                                    // expand_setup.hip: K, coefficients; true if usable
    // multi-overlap remainder H, diagonal; before_agree (optional): waits for a step the caller runs concurrently
    // (the SELL plans, on a host thread) and returns its failure, which joins the group's agreement and is rethrown
    void build_expansion(const int64_t *cpos, int64_t max_inc,
                         const std::function<std::exception_ptr()> &before_agree = {});
    void expansion_kp_raw(const T *p, const cg_scalars<T> *status, bool with_base);
    void expansion_dominant(const T *p, const cg_scalars<T> *status);  // the remainder stream
    // column moments (SELL CSC pass); spart: the moment reduce also forms S from w's partials (sG sets)
    void expansion_moments(const T *w, const cg_scalars<T> *status, const T *spart = nullptr, int sG = 1);
    void expansion_mscale(const cg_scalars<T> *status);                 // moments -> Horner coefficients
    bool expansion_moment_pass(const T *w, const cg_scalars<T> *status, const T *spart = nullptr,
                               int sG = 1);  // true: reduced straight into M
    bool expansion_moments_fused() const;  // the moment pass has panel slabs (then its reduce can form S)
    coefs expansion_coefs() const;
    // predict nclass models through the expansion (expand.hip), KP_MULTI_W classes per pass over the points; false: not
    // applicable (a decision for all classes together), predict brute force. alpha_dev [nclass][lda], ab_dev: the
    // classes' alpha_m, then their biases; out_dev [nclass][ldo]
    bool expansion_predict(const T *alpha_dev, int64_t lda, int64_t nclass, const T *ab_dev, const int64_t *zr_dev,
                           const int32_t *zc_dev, const T *zv_dev, int64_t np, int64_t max_nnz_z, double zabs_max,
                           double znorm_max, T nlast, T *out_dev, int64_t ldo);
    // raw[i] = sum_j k_ij p_j, i < m (with_base = false: only the overlap terms, PLSSVM_MI_PART_OVERLAP)
    void sparse_kp_raw(const T *p, const cg_scalars<T> *status, bool with_base = true);
    void sparse_dominant(const T *p, const cg_scalars<T> *status);  // the dominant sparse kernel
    void spmv_pass_csc(const T *p, const cg_scalars<T> *status);    // factored linear: w = X^T p
    void spmv_pass_csr(const cg_scalars<T> *status);                // factored linear: raw = X w
    int64_t csr_bytes() const { return csr.bytes(); }

    // model use (predict.hip): gpu_csvm::update_w / predict
    rocblas_handle blas = nullptr;
    void update_w_device(const T *alpha_dev);  // w = sum_i alpha_i x_i (device alpha[n])
    void update_w(const T *alpha_host, T *w_host);
    void predict(const T *alpha_host, T bias, const T *Z, const int64_t *zrowptr, const int32_t *zcol, const void *zval,
                 int zfmt, int64_t np, int64_t dz, T *out);  // predict_multi with nclass = 1
    // nclass models on the context's support vectors: alpha[nclass][lda], bias[nclass], out[nclass][ldo] (host). Dense
    // data with the polynomial / rbf kernel: predict_tiles, every class in one pass over the kernel values. The linear w
    // path and sparse data: predict_shared, the points prepared once and up to KP_MULTI_W classes per pass over the
    // support vectors (PLSSVM_MI_PRED_SEQ=1 or PLSSVM_MI_PRED_GEMM=1, read per call: one predict_shared call per
    // class). Row c is bitwise the single call with (alpha_c, bias_c)
    void predict_multi(const T *alpha_host, int64_t nclass, int64_t lda, const T *bias, const T *Z, const int64_t *zrowptr,
                       const int32_t *zcol, const void *zval, int zfmt, int64_t np, int64_t dz, T *out, int64_t ldo);
    void predict_tiles(const T *alpha_host, int64_t nclass, int64_t lda, const T *bias, const T *Z, const int64_t *zrowptr,
                       const int32_t *zcol, const void *zval, int zfmt, int64_t np, T *out, int64_t ldo);
    void predict_shared(const T *alpha_host, int64_t nclass, int64_t lda, const T *bias, const T *Z, const int64_t *zrowptr,
                        const int32_t *zcol, const void *zval, int zfmt, int64_t np, T *out, int64_t ldo);
    // plssvm_mi_get_predict_stats: classes per pass over the support vectors and point uploads of the last predict call
    int64_t predict_classes_per_pass = 0, predict_uploads = 0;
    int predict_algo = 0;  // PLSSVM_MI_PREDICT_*: the path of the last predict call

    void allreduce(T *buf, int64_t count);
    // setup decisions of a real group: every rank's K values, rank-major (world == 1: the local ones)
    std::vector<double> group_gather(const std::vector<double> &v);
    // one step of a group setup: every rank reports its failure (0 = none, else a PLSSVM_MI_ERR_* code) with
    // K values; a failure anywhere throws the same error on every rank (no rank is left waiting in a later
    // exchange), else every rank gets the world x K values, rank-major
    std::vector<double> group_step(int code, const std::string &why, const std::vector<double> &v);
    bool in_group() const { return world > 1 && sim_world == 0 && (comm != nullptr || xchg != nullptr); }
    void allgather_rows(T *buf);
    int64_t device_bytes() const;
};

}  // namespace plssvm_mi
