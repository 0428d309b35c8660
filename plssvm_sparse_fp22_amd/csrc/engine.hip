// engine<T>: setup, q, K·p and the device-resident CG (host orchestration on one HIP stream).
//
// Reference call stack replaced: csvm::learn -> gpu_csvm::setup_data_on_device
// (src/plssvm/backends/gpu_csvm.cpp:130-157) -> generate_q (:160-183) -> solver_CG (:186-324) ->
// run_device_kernel (:353-363) -> device_reduction (:366-386).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include <limits>

#include "engine.hpp"

namespace plssvm_mi {

namespace {


// host kernel_function<k> (include/plssvm/kernel_types.hpp:63-85) for QA_cost = k(x_m, x_m) + 1/C
template <typename T>
T host_kernel(int kernel, int degree, T gamma, T coef0, const T *a, const T *b, int64_t d) {
    T v = 0;
    if (kernel == 2) {
        for (int64_t k = 0; k < d; ++k) {
            const T diff = a[k] - b[k];
            v = std::fma(diff, diff, v);
        }
        return std::exp(-gamma * v);
    }
    if (kernel == KF_LAPLACIAN) {
        for (int64_t k = 0; k < d; ++k) v += std::fabs(a[k] - b[k]);
        return std::exp(-gamma * v);
    }
    for (int64_t k = 0; k < d; ++k) v = std::fma(a[k], b[k], v);
    if (kernel == 0) return v;
    return std::pow(std::fma(gamma, v, coef0), (T) degree);
}

}  // namespace

// The tile kernel's workgroup table: wg_off[k] = the first workgroup of super-block s0 + k (one
// workgroup per real tile: 64 in a full super-block, 36 in a diagonal one, fewer in the ragged last
// row), wg_off[nsuper] = the grid size. Workgroup ids are 32-bit: a share of more than 2^31 - 1 tiles
// (m beyond ~8.4M rows on one rank) is rejected.
void kp_tile_offsets(int64_t nb, int64_t s0, int64_t nsuper, std::vector<int32_t> &wg_off) {
    wg_off.assign((size_t) nsuper + 1, 0);
    int64_t acc = 0;
    for (int64_t k = 0; k < nsuper; ++k) {
        int64_t SI, SJ;
        tri_tile(s0 + k, SI, SJ);
        const int64_t rows = std::min<int64_t>(KP_SUPER, nb - SI * KP_SUPER), cols = std::min<int64_t>(KP_SUPER, nb - SJ * KP_SUPER);
        acc += SI == SJ ? rows * (rows + 1) / 2 : rows * cols;
        if (acc > (int64_t) INT32_MAX)
            throw mi_error(-5, "the dense pairwise share of this rank exceeds 2^31 tiles: use more GPUs");
        wg_off[(size_t) k + 1] = (int32_t) acc;
    }
}

// Balanced contiguous ranges of 8x8-tile super-blocks of the lower triangle (each holds 64 tiles,
// diagonal ones 36, edge ones fewer): rank r gets the super-blocks whose cumulative tile count
// crosses [r, r+1) * total / world. Host-only (plssvm_mi_partition exposes it for CPU tests).
void partition_superblocks(int64_t nb, int rank, int world, int64_t &s0, int64_t &s1, int64_t &s_total,
                           int64_t &tiles_total, int64_t &tiles_local) {
    const int64_t ns = ceil_div(nb, KP_SUPER);
    s_total = ns * (ns + 1) / 2;
    tiles_total = nb * (nb + 1) / 2;
    std::vector<int64_t> cum(s_total + 1, 0);  // tiles before super-block s
    for (int64_t s = 0; s < s_total; ++s) {
        int64_t SI, SJ;
        tri_tile(s, SI, SJ);
        const int64_t rows = std::min<int64_t>(KP_SUPER, nb - SI * KP_SUPER);
        int64_t cnt = 0;
        for (int64_t a = 0; a < rows; ++a) {
            const int64_t I = SI * KP_SUPER + a;
            cnt += std::max<int64_t>(0, std::min<int64_t>(KP_SUPER, I - SJ * KP_SUPER + 1));
        }
        cum[s + 1] = cum[s] + cnt;
    }
    auto split = [&](int r) {
        return (int64_t) (std::lower_bound(cum.begin(), cum.end(), (tiles_total * r) / world) - cum.begin());
    };
    s0 = rank == 0 ? 0 : split(rank);
    s1 = rank == world - 1 ? s_total : split(rank + 1);
    if (s1 < s0) s1 = s0;
    tiles_local = cum[s1] - cum[s0];
}

template <typename T>
void engine<T>::need_dense_kernel_data() const {
    if (kernel == KF_LAPLACIAN)
        throw mi_error(-5, "The Laplacian kernel takes dense data: use plssvm_mi_setup_dense (no sparse L1-distance K.p)");
}

template <typename T>
engine<T>::engine(int kernel_, int degree_, double gamma_, double coef0_, double cost_, int device_) :
    kernel(kernel_), degree(degree_), gamma((T) gamma_), coef0((T) coef0_), cost((T) cost_), device(device_) {
    MI_HIP_CHECK(hipSetDevice(device));
    MI_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    sc.alloc(1, stream);
    red.alloc(2 * RED_BLOCKS, stream);
    wsp.alloc(2 * RED_BLOCKS, stream);
    cgp.alloc(6 * RED_BLOCKS, stream);
}

template <typename T>
engine<T>::~engine() {
    (void) hipSetDevice(device);
    if (stream) (void) hipStreamSynchronize(stream);
    graph_reset();
    if (comm) (void) ncclCommDestroy(comm);
    for (auto &e : cev)
        if (e) (void) hipEventDestroy(e);
    if (cstream) (void) hipStreamDestroy(cstream);
    if (blas) (void) rocblas_destroy_handle(blas);
    XT.reset();
    partial.reset();
    kc.reset();
    if (stream) (void) hipStreamDestroy(stream);
}

template <typename T>
bool engine<T>::factored() const {
    if (kernel != 0) return false;
    if (kp_mode == 2) return true;
    if (kp_mode == 1) return false;
    return sparse;  // AUTO: dense linear runs the MFMA pairwise tiles, sparse linear the factored SpMVs
}

template <typename T>
void engine<T>::need_data() const {
    if (!have_data) throw mi_error(-6, "No data on the device! Maybe a call to setup_data_on_device() is missing?");
}

template <typename T>
void engine<T>::need_q() const {
    if (!have_q) throw mi_error(-6, "No q vector! Maybe a call to generate_q() is missing?");
}

template <typename T>
void engine<T>::comm_init(int rank_, int world_, const void *uid) {
    if (world_ < 1 || rank_ < 0 || rank_ >= world_) throw mi_error(-1, "invalid rank/world_size");
    if (have_data) throw mi_error(-6, "plssvm_mi_comm_init must be called before setup");
    MI_HIP_CHECK(hipSetDevice(device));
    if (comm) {
        (void) ncclCommDestroy(comm);
        comm = nullptr;
    }
    rank = rank_;
    world = world_;
    // a single-rank group still gets a communicator (every collective then runs through RCCL on
    // one GPU: the test path for the collective code on a one-GPU box)
    if (uid == nullptr) {
        if (world > 1) throw mi_error(-1, "a multi-rank group needs a unique id");
        return;
    }
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    // an aborted context stays aborted: a peer that failed before this rank got here will never join the rendezvous
    // below, and resetting the flag would leave this thread blocked in ncclCommInitRank (device_group's failure protocol)
    if (comm_aborted) throw mi_error(-3, "the group was aborted by another rank");
    {
        ncclComm_t c = nullptr;
        const ncclResult_t rc = ncclCommInitRank(&c, world, id, rank);  // blocks until every rank joined
        if (rc != ncclSuccess)
            throw mi_error(-3, std::string("RCCL error '") + ncclGetErrorString(rc) + "' (ncclCommInitRank)");
        std::lock_guard<std::mutex> lk(comm_mu);
        comm = c;
    }
    if (cstream == nullptr) {
        MI_HIP_CHECK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
        for (auto &e : cev) MI_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
}

// called from another host thread while this engine's own thread may be inside a collective: ncclCommAbort makes the
// pending RCCL kernels return; the engine's later RCCL calls throw (MI_NCCL_CHECK), its destructor skips the destroy
template <typename T>
void engine<T>::comm_abort() {
    std::lock_guard<std::mutex> lk(comm_mu);
    comm_aborted = true;
    if (comm != nullptr) {
        (void) ncclCommAbort(comm);
        comm = nullptr;
    }
}

template <typename T>
void engine<T>::comm_init_host(int rank_, int world_, int (*fn)(void *, int64_t, int, int, void *), void *user) {
    if (world_ < 1 || rank_ < 0 || rank_ >= world_) throw mi_error(-1, "invalid rank/world_size");
    if (fn == nullptr) throw mi_error(-1, "a host-staged group needs an exchange function");
    if (have_data) throw mi_error(-6, "plssvm_mi_comm_init_host must be called before setup");
    if (sim_world > 0) throw mi_error(-1, "a simulated rank cannot join a group");
    MI_HIP_CHECK(hipSetDevice(device));
    if (comm) {
        (void) ncclCommDestroy(comm);
        comm = nullptr;
    }
    comm_aborted = false;
    rank = rank_;
    world = world_;
    xchg = fn;
    xchg_user = user;
}

// Exchange step of one K·p. RCCL: in-stream collective. Host-staged: the reference's
// device_reduction (gpu_csvm.cpp:366-386) — synchronise, D2H, combine on the host (caller's
// collective), H2D — so the device work before and after is exactly the RCCL path's.
template <typename T>
void engine<T>::allreduce(T *buf, int64_t count) {
    if (count <= 0) return;
    if (comm != nullptr) {
        psum_group_begin(stream);
        MI_NCCL_CHECK(ncclAllReduce(buf, buf, (size_t) count, nccl_type<T>(), ncclSum, comm, stream));
        psum_group_end();
    } else if (xchg != nullptr) {
        xbuf.resize((size_t) count);
        MI_HIP_CHECK(hipMemcpyAsync(xbuf.data(), buf, sizeof(T) * (size_t) count, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        if (xchg(xbuf.data(), count, (int) sizeof(T), 0, xchg_user) != 0) throw mi_error(-3, "host exchange failed");
        MI_HIP_CHECK(hipMemcpyAsync(buf, xbuf.data(), sizeof(T) * (size_t) count, hipMemcpyHostToDevice, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));  // xbuf is reused by the next exchange
    }
}

// sharded CG: the 2 x RED_BLOCKS partials of every rank (rank-major, into slot `slot` of cgp_g); the
// consumers sum them in rank order. Unsharded or a single rank: the local partials.
template <typename T>
const T *engine<T>::gather_partials(T *local, int slot, int64_t K) {
    if (!gathered) return local;
    T *out = cgp_g.get() + (int64_t) slot * G * 2 * RED_BLOCKS;  // K = 4 R: slots slot and slot + 1
    if (comm != nullptr) {
        MI_NCCL_CHECK(ncclAllGather(local, out, (size_t) K, nccl_type<T>(), comm, stream));
    } else {
        xpart.resize((size_t) (G * K));
        MI_HIP_CHECK(hipMemcpyAsync(xpart.data() + rank * K, local, sizeof(T) * (size_t) K, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        if (xchg(xpart.data(), K, (int) sizeof(T), 1, xchg_user) != 0) throw mi_error(-3, "host exchange failed");
        MI_HIP_CHECK(hipMemcpyAsync(out, xpart.data(), sizeof(T) * xpart.size(), hipMemcpyHostToDevice, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
    return out;
}

template <typename T>
void engine<T>::psum_group_begin(hipStream_t s) {
    if (!psum_pending || comm == nullptr) return;
    MI_NCCL_CHECK(ncclGroupStart());
    MI_NCCL_CHECK(ncclAllGather(cgp.get(), cgp_g.get(), (size_t) (2 * RED_BLOCKS), nccl_type<T>(), comm, s));
}

template <typename T>
void engine<T>::psum_group_end() {
    if (!psum_pending || comm == nullptr) return;
    MI_NCCL_CHECK(ncclGroupEnd());
    psum_pending = false;
}

template <typename T>
void engine<T>::flush_psum() {
    if (!psum_pending) return;
    psum_pending = false;
    gather_partials(cgp.get(), 0);
}

template <typename T>
void engine<T>::gather_input(const T *p) {
    if (gathered) allgather_rows(const_cast<T *>(p));
}

template <typename T>
void engine<T>::reduce_scatter_rows(T *buf) {
    if (comm != nullptr) {
        psum_group_begin(stream);
        MI_NCCL_CHECK(ncclReduceScatter(buf, buf + (int64_t) rank * chunk, (size_t) chunk, nccl_type<T>(), ncclSum, comm,
                                        stream));
        psum_group_end();
    } else if (xchg != nullptr) {
        allreduce(buf, chunk * world);  // the host transport sums everything; the own rows are used
    }
}

template <typename T>
void engine<T>::allgather_rows(T *buf) {
    if (comm != nullptr) {
        psum_group_begin(stream);
        MI_NCCL_CHECK(ncclAllGather(buf + (int64_t) rank * chunk, buf, (size_t) chunk, nccl_type<T>(), comm, stream));
        psum_group_end();
    } else if (xchg != nullptr) {
        const int64_t total = chunk * world;
        xbuf.resize((size_t) total);
        MI_HIP_CHECK(hipMemcpyAsync(xbuf.data(), buf, sizeof(T) * (size_t) total, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        if (xchg(xbuf.data(), chunk, (int) sizeof(T), 1, xchg_user) != 0) throw mi_error(-3, "host exchange failed");
        MI_HIP_CHECK(hipMemcpyAsync(buf, xbuf.data(), sizeof(T) * (size_t) total, hipMemcpyHostToDevice, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

// Small all-gather for setup decisions that every rank of a group must take identically (the sparse
// algorithm, its fallbacks): each rank contributes K values and gets all world x K, rank-major, through
// RCCL or the host exchange. The values pass through the real type T, so every rank compares the same
// rounded numbers. No group (or a simulated rank): the local values.
template <typename T>
std::vector<double> engine<T>::group_gather(const std::vector<double> &v) {
    const int64_t K = (int64_t) v.size();
    if (!in_group() || K == 0) return v;
    std::vector<T> h((size_t) (K * world), T(0));
    for (int64_t k = 0; k < K; ++k) h[(size_t) (rank * K + k)] = (T) v[(size_t) k];
    if (comm != nullptr) {
        dev_buf<T> buf;
        buf.alloc(K * world, stream);
        MI_HIP_CHECK(hipMemcpyAsync(buf.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, stream));
        MI_NCCL_CHECK(ncclAllGather(buf.get() + rank * K, buf.get(), (size_t) K, nccl_type<T>(), comm, stream));
        MI_HIP_CHECK(hipMemcpyAsync(h.data(), buf.get(), sizeof(T) * h.size(), hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    } else if (xchg(h.data(), K, (int) sizeof(T), 1, xchg_user) != 0) {
        throw mi_error(-3, "host exchange failed");
    }
    return std::vector<double>(h.begin(), h.end());
}

template <typename T>
std::vector<double> engine<T>::group_step(int code, const std::string &why, const std::vector<double> &v) {
    std::vector<double> mine{ (double) code };
    mine.insert(mine.end(), v.begin(), v.end());
    const auto g = group_gather(mine);
    const size_t K1 = mine.size();
    const int nr = (int) (g.size() / K1);
    int worst = 0;  // the first rank's failure, a non-OOM one over ERR_OOM (OOM alone: the caller's fallback)
    for (int r = 0; r < nr; ++r) {
        const int c = (int) g[(size_t) r * K1];
        if (c != 0 && (worst == 0 || worst == -4)) worst = c;
    }
    if (worst != 0)
        throw mi_error(worst, code != 0 ? why : std::string("sparse setup failed on another rank of the group"));
    std::vector<double> out;
    out.reserve((size_t) nr * v.size());
    for (int r = 0; r < nr; ++r)
        out.insert(out.end(), g.begin() + (std::ptrdiff_t) ((size_t) r * K1 + 1), g.begin() + (std::ptrdiff_t) ((size_t) (r + 1) * K1));
    return out;
}

template <typename T>
void engine<T>::setup_dense(const T *X, int64_t n_, int64_t d_) {
    if (X == nullptr || n_ < 1 || d_ < 1) throw mi_error(-1, "Data set is empty!");
    MI_HIP_CHECK(hipSetDevice(device));
    sparse = false;
    n = n_;
    d = d_;
    m = n - 1;
    nb = ceil_div(m, KP_TILE);
    n_pad = std::max<int64_t>(nb, 1) * KP_TILE;
    d_pad = round_up(d, kp_dpad<T>());
    // device layout: feature-major XT[d_pad][n_pad] of the first m points; the last point separately
    // (the reference's data_d_ / data_last_d_, gpu_csvm.cpp:142-155, with 64-bit offsets and tile padding)
    XT.alloc(d_pad * n_pad, stream);
    shifted = kernel == 2 && m > 0;
    shift_h.assign((size_t) d, T(0));
    shift.reset();
    if (shifted) {
        std::vector<double> sum((size_t) d, 0.0);
        for (int64_t i = 0; i < m; ++i)
            for (int64_t k = 0; k < d; ++k) sum[(size_t) k] += (double) X[i * d + k];
        for (int64_t k = 0; k < d; ++k) shift_h[(size_t) k] = (T) (sum[(size_t) k] / (double) m);
        shift.alloc(d, stream, false);
        MI_HIP_CHECK(hipMemcpyAsync(shift.get(), shift_h.data(), sizeof(T) * (size_t) d, hipMemcpyHostToDevice, stream));
    }
    {
        dev_buf<T> tmp;
        tmp.alloc(std::max<int64_t>(m, 1) * d, stream, false);
        if (m > 0) {
            MI_HIP_CHECK(hipMemcpyAsync(tmp.get(), X, sizeof(T) * (size_t) (m * d), hipMemcpyHostToDevice, stream));
            if (shifted) launch_shift_rows<T>(tmp.get(), m, d, shift.get(), stream);
            launch_transpose<T>(tmp.get(), m, d, XT.get(), n_pad, stream);
        }
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
    xlast_h.assign(X + m * d, X + m * d + d);
    for (int64_t k = 0; k < d; ++k) xlast_h[(size_t) k] = xlast_h[(size_t) k] - shift_h[(size_t) k];  // x - 0 = x
    xlast.alloc(d_pad, stream);
    MI_HIP_CHECK(hipMemcpyAsync(xlast.get(), xlast_h.data(), sizeof(T) * (size_t) d, hipMemcpyHostToDevice, stream));
    norms.alloc(n_pad, stream);
    if (kernel == 2) launch_row_norms<T>(XT.get(), n_pad, d, norms.get(), stream);
    finish_setup();
}

template <typename T>
void engine<T>::finish_setup() {
    lanes = lane_pool{};  // an earlier setup's lanes go before the tile cache is sized; the first multi call allocates anew
    sinv_h.clear();       // point weights belong to the data they were set for
    sinv.reset();
    // work split of the implicit matrix over the group (replaces feature_ranges_, gpu_csvm.cpp:136-139)
    partition_superblocks(nb, sim_world > 0 ? sim_rank : rank, sim_world > 0 ? sim_world : world, t0, t1, t_total,
                          tiles_total, tiles_local);
    const int eff_world = sim_world > 0 ? sim_world : world, eff_rank = sim_world > 0 ? sim_rank : rank;
    chunk = ceil_div(std::max<int64_t>(m, 1), eff_world);
    r0 = std::min<int64_t>(m, eff_rank * chunk);
    r1 = std::min<int64_t>(m, r0 + chunk);
    const int64_t vec_len = std::max<int64_t>(n_pad, chunk * eff_world);
    {
        const char *se = std::getenv("PLSSVM_MI_SHARD");
        const int opt = se != nullptr ? std::atoi(se) : -1;
        // a one-rank RCCL group with PLSSVM_MI_SHARD=1 runs every sharded collective through RCCL on one GPU
        // (the test path of the sharded RCCL code on a one-GPU box)
        const bool grp = (comm != nullptr || xchg != nullptr) && sim_world == 0;
        shard = (grp && (opt == 1 || (opt < 0 && sparse && world > 1))) || (sim_world > 0 && opt == 1);
        gathered = shard && grp;
        v0 = shard ? r0 : 0;
        vn = shard ? r1 - r0 : m;
        G = gathered ? world : 1;
        if (gathered) cgp_g.alloc(5 * (int64_t) G * 2 * RED_BLOCKS, stream);
    }
    tiles_upload();
    if (!sparse && !factored()) {
        // the rank's tile slab: one record of row and column sums per own tile (scales with 1 / world)
        partial.alloc(std::max<int64_t>(kp_wgs, 1) * KP_REC, stream, false);
    } else {
        partial.reset();
    }
    q.alloc(vec_len, stream);
    pv.alloc(vec_len, stream);
    ret.alloc(vec_len, stream);
    x.alloc(vec_len, stream);
    r.alloc(vec_len, stream);
    dv.alloc(vec_len, stream);
    Ad.alloc(vec_len, stream);
    b.alloc(vec_len, stream);
    raw.alloc(vec_len, stream);
    w.alloc(std::max<int64_t>(d_pad, 1), stream);
    MI_HIP_CHECK(hipStreamSynchronize(stream));
    kc.setup(*this);
    have_data = true;
    have_q = false;
    q_gen = false;
    ctr_ok = false;
    cg_active = false;
    graph_reset();
}

// the tile kernel's workgroup table for this rank's super-blocks [t0, t1) (also the densified sparse path)
template <typename T>
void engine<T>::tiles_upload() {
    std::vector<int32_t> off;
    kp_tile_offsets(nb, t0, t1 - t0, off);
    kp_wgs = off.back();
    kp_wgoff.alloc((int64_t) off.size(), stream, false);
    MI_HIP_CHECK(hipMemcpyAsync(kp_wgoff.get(), off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice, stream));
    MI_HIP_CHECK(hipStreamSynchronize(stream));
}

template <typename T>
void engine<T>::tile_cache::reset() {
    rec.reset();
    desc.reset();
    tiles = 0;
    valid = false;
    pack = 0;
    packed_host = -1;
    narrow_host = 0;
}

// The tile cache of this setup: as many of the rank's tiles as the memory budget holds, none for a path that does not
// run the tile kernel. The records of an earlier setup are dropped first (their data is gone), nothing is written
// here: the first K·p without a stop flag fills them (kp_tiles_now). No room, or an allocation that fails: no cache.
template <typename T>
void engine<T>::tile_cache::setup(const engine &e) {
    reset();
    const bool tiles_path = !e.factored() && (!e.sparse || e.csr.dense_on);  // kp_raw's launch_kp_tiles branch
    const char *ke = std::getenv("PLSSVM_MI_KP_CACHE");
    if (!tiles_path || cache_opt == 1 || (ke != nullptr && std::atoi(ke) == 0) || e.kp_wgs <= 0 || e.m <= 0) return;
    phase_timer pt;
    const int64_t rec_bytes = KP_CACHE_REC * (int64_t) sizeof(T);
    const int64_t fit = std::min<int64_t>(e.kp_wgs, e.mem_budget() / rec_bytes);
    if (fit <= 0) return;
    try {
        rec.alloc(fit * KP_CACHE_REC, e.stream, false);
        desc.alloc(fit + 2, e.stream);  // every tile raw, no tile packed or narrow; outside the budget: T does not depend on it
    } catch (const mi_error &) {
        (void) hipGetLastError();
        reset();
        return;
    }
    tiles = fit;
    const char *pe = std::getenv("PLSSVM_MI_KP_PACK");
    const char *ne = std::getenv("PLSSVM_MI_KP_NARROW");
    if (sizeof(T) == 8 && pack_opt != 1 && !(pe != nullptr && std::atoi(pe) == 0))
        pack = (pack_opt == 2 || (ne != nullptr && std::atoi(ne) == 0)) ? 1 : 2;
    pt.mark("kp cache alloc");
}

// The tile launches of one K·p. An unfilled cache is filled only by a K·p that no stop flag can cut short and that
// is launched, not captured: a kernel leaving at `converged` must not leave records half written and trusted, and a
// replayed graph must not store. Until then (and past the cached prefix) the tiles are computed.
template <typename T>
void engine<T>::kp_tiles_now(const T *p, const cg_scalars<T> *status) {
    bool fill = false;
    if (kc.tiles > 0 && !kc.valid && status == nullptr) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        MI_HIP_CHECK(hipStreamIsCapturing(stream, &cs));
        fill = cs == hipStreamCaptureStatusNone;
    }
    launch_kp_tiles<T>(kp_geometry(), p, partial.get(), status, stream, kc.view(fill), fill);
    if (fill) kc.valid = true;
}

// Tiles of the cache stored in a packed form (wide or narrow), and those of them in the narrow form: the fill's two
// counters, copied back together, once, on the first request after it
template <typename T>
int64_t engine<T>::tile_cache::packed(const engine &e) {
    if (!valid || tiles <= 0 || pack == 0) return 0;
    if (packed_host < 0) {
        int32_t c[2] = { 0, 0 };
        MI_HIP_CHECK(hipSetDevice(e.device));
        MI_HIP_CHECK(hipMemcpyAsync(c, desc.get() + tiles, sizeof(c), hipMemcpyDeviceToHost, e.stream));
        MI_HIP_CHECK(hipStreamSynchronize(e.stream));
        packed_host = c[0];
        narrow_host = c[1];
    }
    return packed_host;
}

template <typename T>
void engine<T>::generate_q(T *q_out, double *qa_out) {
    need_data();
    MI_HIP_CHECK(hipSetDevice(device));
    if (sparse) {
        sparse_q();
    } else {
        launch_q_dense<T>(kf(), XT.get(), n_pad, d, m, xlast.get(), q.get(), stream);
    }
    ctr_kmm = host_kernel<T>(kernel, degree, gamma, coef0, xlast_h.data(), xlast_h.data(), d);
    QA_cost = ctr_kmm + diag_m();
    q_gen_h.resize((size_t) std::max<int64_t>(m, 0));
    if (m > 0) MI_HIP_CHECK(hipMemcpyAsync(q_gen_h.data(), q.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
    MI_HIP_CHECK(hipStreamSynchronize(stream));
    if (q_out && m > 0) std::memcpy(q_out, q_gen_h.data(), sizeof(T) * (size_t) m);
    if (qa_out) *qa_out = (double) QA_cost;
    have_q = true;
    q_gen = true;
    if (sparse) ctr_setup();
    graph_reset();
}

template <typename T>
void engine<T>::set_q(const T *q_host) {
    need_data();
    if (q_host == nullptr) {
        need_q();
        return;
    }
    if (m > 0) MI_HIP_CHECK(hipMemcpyAsync(q.get(), q_host, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
    // a caller's q equal to the generated one keeps the centered finalize; any other q is used as given
    q_gen = (int64_t) q_gen_h.size() == m && (m == 0 || std::memcmp(q_host, q_gen_h.data(), sizeof(T) * (size_t) m) == 0);
    if (!have_q) {
        QA_cost = host_kernel<T>(kernel, degree, gamma, coef0, xlast_h.data(), xlast_h.data(), d) + diag_m();
        have_q = true;
    }
}

// ---- the steps of K·p and CG on one right-hand side's state (engine.hpp cg_lane) ----------------------------------
// sum(p) and sum(q p): the rank-1 parts of Q~ (QA_cost - q_i - q_j) never enter the tiles (sharded: this
// rank's rows, then the gathered partials of all ranks)
template <typename T>
void engine<T>::kp_sums(const T *p, const cg_lane &L, const cg_scalars<T> *status) {
    launch_dot2<T>(p + v0, nullptr, qf() + v0, p + v0, vn, L.red, status, stream);
    launch_dot_final<T>(gather_partials(L.red, 3), L.sc, FIN_SP_SQP, 0, nullptr, 0, nullptr, stream, G);
}

template <typename T>
void engine<T>::kp_slab_reduce(const cg_lane &L, const cg_scalars<T> *status) {
    launch_kp_reduce<T>(L.slab, nb, m, t0, t1, kp_wgoff.get(), L.raw, status, stream);
}

template <typename T>
void engine<T>::kp_fin(const cg_lane &L, const T *p, T *out, T add, bool overwrite, const cg_scalars<T> *status) {
    const int flags = (overwrite ? 1 : 0) | ((sim_world > 0 && sim_rank != 0 && !shard) ? 2 : 0);
    launch_kp_finalize<T>(L.raw + v0, qf() + v0, p + v0, L.sc, L.QA, L.cost_inv, L.sinv ? L.sinv + v0 : nullptr,
                          L.hold ? L.hold + v0 : nullptr, add, flags, vn, out + v0, status, stream);
}

// out = (overwrite ? 0 : out) + add * Q~ p   — run_device_kernel + device_reduction
template <typename T>
void engine<T>::kp_device(const T *p, T *out, T add, bool overwrite, const cg_scalars<T> *status) {
    if (m <= 0) return;
    const cg_lane L = own_lane();
    kp_sums(p, L, status);
    ctr_now = ctr_active();
    kp_raw(p, status);
    ctr_now = false;
    kp_fin(L, p, out, add, overwrite, status);
}

template <typename T>
void engine<T>::kp_raw(const T *p, const cg_scalars<T> *status) {
    if (m <= 0) return;
    if (sparse_stored()) {
        sparse_kp_raw(p, status);
    } else if (factored()) {
        const bool all_rows = sim_world > 0 && !shard;
        launch_gemv_t<T>(XT.get(), n_pad, d, all_rows ? 0 : r0, all_rows ? m : r1, p, w.get(), status, stream);
        allreduce(w.get(), d);
        launch_gemv_n<T>(XT.get(), n_pad, d, r0, r1, w.get(), raw.get(), status, stream);
        if (!shard) allgather_rows(raw.get());
    } else {
        gather_input(p);
        kp_tiles_now(p, status);
        kp_slab_reduce(own_lane(), status);
        if (shard) reduce_scatter_rows(raw.get());
        else allreduce(raw.get(), m);
    }
}

template <typename T>
void engine<T>::kp_host(const T *q_host, const T *p, T *ret_host, T add) {
    need_data();
    MI_HIP_CHECK(hipSetDevice(device));
    set_q(q_host);
    cg_active = false;
    MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
    if (m > 0) {
        MI_HIP_CHECK(hipMemcpyAsync(pv.get(), p, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
        MI_HIP_CHECK(hipMemcpyAsync(ret.get(), ret_host, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
        kp_device(pv.get(), ret.get(), add, false, nullptr);
        if (gathered) allgather_rows(ret.get());  // device_reduction's result on every rank
        MI_HIP_CHECK(hipMemcpyAsync(ret_host, ret.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
    }
    MI_HIP_CHECK(hipStreamSynchronize(stream));
}

// test hook: one part of Q~p (PLSSVM_MI_PART_KERNEL: sum_j k_ij p_j; PLSSVM_MI_PART_OVERLAP: the
// sparse overlap sum only; PLSSVM_MI_PART_REMAINDER: the kernel expansion's stored remainder stream only), after the
// group exchange
template <typename T>
void engine<T>::kp_part(const T *p_host, T *out_host, int part) {
    need_data();
    if (part < 0 || part > 2) throw mi_error(-1, "unknown K·p part");
    if (part == 1 && !(sparse_stored() && !factored()))
        throw mi_error(-5, "the overlap part exists for the stored sparse poly/rbf paths only");
    if (part == 2 && !(sparse_stored() && !factored() && csr.ex.on && !csr.otf_on))
        throw mi_error(-5, "the remainder part exists for the sparse kernel expansion only");
    MI_HIP_CHECK(hipSetDevice(device));
    cg_active = false;
    MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
    if (m > 0) {
        MI_HIP_CHECK(hipMemcpyAsync(pv.get(), p_host, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
        part_mode = part;
        try {
            if (part != 0) sparse_kp_raw(pv.get(), nullptr, false);
            else kp_raw(pv.get(), nullptr);
        } catch (...) {
            part_mode = 0;
            throw;
        }
        part_mode = 0;
        if (gathered) allgather_rows(raw.get());
        MI_HIP_CHECK(hipMemcpyAsync(out_host, raw.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
    }
    MI_HIP_CHECK(hipStreamSynchronize(stream));
}

// ---- CG: openmp::csvm::solver_CG semantics (src/plssvm/backends/OpenMP/csvm.cpp:82-170) -------------
template <typename T>
cg_scalars<T> engine<T>::cg_scalars_init(T eps, bool force) {
    cg_scalars<T> init{};
    init.eps2delta0 = eps * eps;
    init.force = force ? 1 : 0;
    init.g1[0] = init.g1[1] = init.a1[0] = init.a1[1] = std::numeric_limits<T>::infinity();
    return init;
}

// Ad = Q~ v from the K·p's raw (P > 0: summed from P panel slabs) and the v.Ad partials in pd; sharded: with the
// sum v / sum q v partials the previous step gathered (slot 0)
template <typename T>
void engine<T>::cg_fin_dad(const cg_lane &L, const T *v, T *pd, const T *slabs, int64_t P) {
    const int raw_only = (sim_world > 0 && sim_rank != 0 && !shard) ? 1 : 0;
    launch_cg_fin_dad<T>(L.raw + v0, slabs, P, m, qf() + v0, v + v0, gathered ? cgp_g.get() : L.cgp, G, L.QA, L.cost_inv,
                         L.sinv ? L.sinv + v0 : nullptr, L.hold ? L.hold + v0 : nullptr, raw_only, vn, L.Ad + v0, pd, L.sc,
                         stream);
}

// alpha = delta / (d . Ad) (:116); x += alpha d; r = b every 50th iteration, else r -= alpha Ad   (:119-132)
template <typename T>
void engine<T>::cg_upd_rr(const cg_lane &L, int reset) {
    launch_cg_upd_rr<T>(L.x + v0, L.r + v0, L.d + v0, L.Ad + v0, L.b + v0, reset, gather_partials(L.pdad(), 1), G, vn,
                        L.prr(), L.sc, stream);
}

template <typename T>
void engine<T>::cg_rr(const cg_lane &L, const cg_scalars<T> *status) {
    launch_dot2<T>(L.r + v0, L.r + v0, nullptr, nullptr, vn, L.prr(), status, stream);
}

// delta = r.r ; delta0   (:92-97)   (sharded: this rank's rows, the ranks' partials gathered)
template <typename T>
void engine<T>::cg_delta0(const cg_lane &L) {
    launch_dot2<T>(L.r + v0, L.r + v0, nullptr, nullptr, vn, L.red, nullptr, stream);
    launch_dot_final<T>(gather_partials(L.red, 3), L.sc, FIN_DELTA0, 0, L.trace, L.trace_cap, nullptr, stream, G);
}

// delta = r.r ; stop test ; beta (:135-146); d = beta d + r (:149-151), init: d = r (:97); with sum d / sum q d for
// the next Q~d (kernel expansion, bfloat16 windows: with the next K·p's w pass, dir_w_fill)
template <typename T>
void engine<T>::cg_dir(const cg_lane &L, int init) {
    dir_w_t<T> wo{};
    const bool fw = dir_w_fill(wo);
    launch_cg_dir_sums<T>(L.d + v0, L.r + v0, qf() + v0, init ? nullptr : gather_partials(L.prr(), 2), init ? 1 : G, init,
                          init ? nullptr : L.trace, init ? 0 : L.trace_cap, vn, L.cgp, L.sc, stream, fw ? &wo : nullptr);
    w_pre = fw ? L.d : nullptr;
}

template <typename T>
void engine<T>::cg_begin(const T *b_host, const T *q_host, T eps, bool force, double *delta0_out, int64_t trace_len) {
    need_data();
    MI_HIP_CHECK(hipSetDevice(device));
    set_q(q_host);
    const cg_scalars<T> init = cg_scalars_init(eps, force);
    cg1 = cg1_wanted();
    MI_HIP_CHECK(hipMemcpyAsync(sc.get(), &init, sizeof(init), hipMemcpyHostToDevice, stream));
    trace_cap = std::max<int64_t>(trace_len, 1);
    if (trace.size() < trace_cap) trace.alloc(trace_cap, stream);
    graph_reset();  // QA_cost, trace and the vectors' contents may differ from the captured solve
    if (m > 0) MI_HIP_CHECK(hipMemcpyAsync(b.get(), b_host, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
    // x = 1; r = b; r -= Q~x   (csvm.cpp:85-90)
    if (hold_cur != nullptr) launch_cg_init_held<T>(b.get(), hold_cur, m, x.get(), r.get(), stream);  // learn_held's lane
    else launch_cg_init<T>(b.get(), m, x.get(), r.get(), stream);
    kp_device(x.get(), r.get(), T(-1), false, nullptr);
    cg_delta0(own_lane());
    if (cg1) {
        // one-reduction CG: d = s = 0, the r.r / sum r / sum q r partials of r0 (set 0) for the first product Q~r
        dir_w_t<T> wo{};
        const bool fw = dir_w_fill(wo);
        if (sv.size() < q.size()) sv.alloc(q.size(), stream);
        if (cg1p.size() < 8 * RED_BLOCKS) cg1p.alloc(8 * RED_BLOCKS, stream);  // two [r.u | r.r | r.s | 0] sets
        MI_HIP_CHECK(hipMemsetAsync(dv.get(), 0, sizeof(T) * (size_t) q.size(), stream));
        MI_HIP_CHECK(hipMemsetAsync(sv.get(), 0, sizeof(T) * (size_t) q.size(), stream));
        launch_cg1_rsums<T>(r.get() + v0, sv.get() + v0, qf() + v0, vn, cg1p.get(), cgp.get(), sc.get(), stream, fw ? &wo : nullptr);
        w_pre = fw ? r.get() : nullptr;
    } else {
        cg_dir(own_lane(), 1);
    }
    if (gathered && comm != nullptr) psum_pending = true;  // gathered with the first K·p's collective
    else gather_partials(cgp.get(), 0);
    run = 0;
    cg_active = true;
    // a solve that can reach a whole block captures it now (capture launches nothing; the
    // instantiation stays out of the iterations' time)
    if (trace_len > CG_RESET && graph_usable()) graph_capture();
    if (delta0_out) {
        cg_scalars<T> h{};
        MI_HIP_CHECK(hipMemcpyAsync(&h, sc.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        *delta0_out = (double) h.delta0;
    }
}

// one CG iteration (reset: the every-50th recomputation r = b - Q~x), all launches on the engine stream
// the one-reduction recurrence: forced (PLSSVM_MI_CG_ONE_REDUCTION), or auto for a sharded group of several ranks
template <typename T>
bool engine<T>::cg1_wanted() const {
    return cg_variant == 1 || (cg_variant == 2 && gathered && G > 1);
}

// The engine's own Ad = Q~ v with the v.Ad partials in pd (:111-113): v = d, or r for the one-reduction CG (u in Ad)
template <typename T>
void engine<T>::cg_product(const T *v, T *pd) {
    const cg_lane L = own_lane();
    const cg_scalars<T> *st = L.sc;
    const bool one_gpu_factored = sparse && factored() && world == 1 && sim_world == 0;
    const T *slabs = nullptr;
    int64_t P = 0;
    bool fin = false;
    if (sparse_stored() && one_gpu_factored && csr.rb_csr.nblk > 0) {
        // one GPU, factored sparse linear: CSC pass, then the row-block CSR pass with the finalize and
        // the v.Ad partials fused (spmv.hpp)
        spmv_pass_csc(v, st);
        launch_rowblock_fin<T>(csr.rb_csr, w.get(), d, q.get(), v, L.cgp, L.QA, L.cost_inv, L.sinv, L.Ad, pd, st, stream);
        fin = true;
    } else if (one_gpu_factored && csr.spmv_csr.P > 1) {
        // one GPU, factored sparse linear: the CSR pass's panel slabs are summed by cg_fin_dad
        spmv_pass_csc(v, st);
        launch_panel_spmv<T>(csr.spmv_csr, w.get(), d, L.raw, st, stream, 1, 0, false);
        slabs = csr.spmv_csr.partial.get();
        P = csr.spmv_csr.P;
    } else {
        // offered to the K·p: a path that forms Ad and the partials in its own last kernel sets kp_fin_done
        const kp_fin_t f{ qf(), v, gathered ? cgp_g.get() : L.cgp, G, L.QA, L.cost_inv, L.sinv, L.Ad, pd };
        kp_fin_req = (sim_world > 0 && sim_rank != 0 && !shard) ? nullptr : &f;
        kp_fin_done = false;
        ctr_now = ctr_active();
        kp_raw(v, st);
        ctr_now = false;
        kp_fin_req = nullptr;
        fin = kp_fin_done;
        kp_fin_done = false;
    }
    flush_psum();  // no collective of the K·p carried it
    if (!fin) cg_fin_dad(L, v, pd, slabs, P);
}

// one iteration of the one-reduction CG (blas1.hip cg1_update_kernel): u = Q~r with the finalize forming the r.u
// partials beside the r.r ones of set `par`, ONE gather of that set, then d, s, x, r and the next partials in one kernel
template <typename T>
void engine<T>::cg1_iter(int reset) {
    const cg_scalars<T> *st = sc.get();
    T *psum = cgp.get();
    T *cur = cg1p.get() + (int64_t) cg_par * 4 * RED_BLOCKS, *nxt = cg1p.get() + (int64_t) (cg_par ^ 1) * 4 * RED_BLOCKS;
    cg_product(r.get(), cur);
    // the one collective of the iteration: [r.u | r.r] partials of every rank
    const T *pset = gather_partials(cur, 1, 4 * RED_BLOCKS);
    dir_w_t<T> wo{};
    const bool fw = !reset && dir_w_fill(wo);
    launch_cg1_update<T>(x.get() + v0, r.get() + v0, dv.get() + v0, sv.get() + v0, Ad.get() + v0, b.get() + v0, qf() + v0,
                         reset, pset, G, trace.get(), trace_cap, vn, cg_par, nxt, psum, sc.get(), stream, fw ? &wo : nullptr);
    w_pre = fw ? r.get() : nullptr;
    if (reset) {  // r = b - Q~x, then its partials (csvm.cpp:119-132)
        kp_device(x.get(), r.get(), T(-1), false, st);
        dir_w_t<T> wr{};
        const bool fr = dir_w_fill(wr);
        launch_cg1_rsums<T>(r.get() + v0, sv.get() + v0, qf() + v0, vn, nxt, psum, sc.get(), stream, fr ? &wr : nullptr);
        w_pre = fr ? r.get() : nullptr;
    }
    if (gathered && comm != nullptr) psum_pending = true;  // gathered with the next product's first collective
    else gather_partials(psum, 0);
}

template <typename T>
void engine<T>::cg_iter(int reset) {
    if (cg1) {
        cg1_iter(reset);
        return;
    }
    const cg_lane L = own_lane();
    cg_product(L.d, L.pdad());
    cg_upd_rr(L, reset);
    if (reset) {  // r = b - Q~x (:119-132)
        kp_device(L.x, L.r, T(-1), false, L.sc);
        cg_rr(L, L.sc);
    }
    cg_dir(L, 0);
    if (gathered && comm != nullptr) psum_pending = true;  // gathered with the next K·p's first collective
    else gather_partials(L.cgp, 0);
}

// Iteration blocks of CG_RESET (the reset period) starting at a multiple of it are replayed from one
// captured hipGraph: the launches of a block depend only on the engine's buffers (the iteration
// index lives on the device), so one capture serves every block of a solve. Host-staged groups
// synchronise inside the exchange and are never captured; RCCL groups are captured only with
// PLSSVM_MI_GRAPH=2 (the collectives then run as graph nodes); PLSSVM_MI_GRAPH=0 disables graphs.
template <typename T>
bool engine<T>::graph_usable() const {
    const char *ge = std::getenv("PLSSVM_MI_GRAPH");  // read per call (tests compare graphs off / on in one process)
    const int mode = ge == nullptr ? 1 : std::atoi(ge);
    if (mode == 0 || xchg != nullptr || m <= 0) return false;
    return comm == nullptr || mode == 2;
}

template <typename T>
void engine<T>::graph_reset() {
    if (cg_graph != nullptr) {
        (void) hipGraphExecDestroy(cg_graph);
        cg_graph = nullptr;
    }
}

template <typename T>
void engine<T>::graph_capture() {
    if (cg_graph == nullptr) {
        hipGraph_t g = nullptr;
        // a block forms its first w itself (the replay may follow any other K·p); w_pre stays what the launched
        // work left, graph_w_end is what a replay leaves
        const T *keep = w_pre;
        w_pre = nullptr;
        MI_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        try {
            for (int k = 0; k < CG_RESET; ++k) {
                cg_par = k & 1;  // blocks start at multiples of CG_RESET (even)
                cg_iter(k == CG_RESET - 1 ? 1 : 0);
            }
        } catch (...) {
            (void) hipStreamEndCapture(stream, &g);
            if (g) (void) hipGraphDestroy(g);
            w_pre = keep;
            throw;
        }
        graph_w_end = w_pre;
        w_pre = keep;
        MI_HIP_CHECK(hipStreamEndCapture(stream, &g));
        const hipError_t e = hipGraphInstantiate(&cg_graph, g, nullptr, nullptr, 0);
        (void) hipGraphDestroy(g);
        MI_HIP_CHECK(e);
    }
}

template <typename T>
void engine<T>::graph_block() {
    graph_capture();
    MI_HIP_CHECK(hipGraphLaunch(cg_graph, stream));
    w_pre = graph_w_end;
}

template <typename T>
void engine<T>::cg_step(int64_t nsteps, bool &converged, int64_t &iters) {
    if (!cg_active) throw mi_error(-6, "cg_step without cg_begin");
    MI_HIP_CHECK(hipSetDevice(device));
    // m == 0: the kernels see no elements, converge at once
    for (int64_t s = 0; s < nsteps;) {
        if (run % CG_RESET == 0 && nsteps - s >= CG_RESET && graph_usable()) {
            graph_block();
            s += CG_RESET;
            run += CG_RESET;
        } else {
            cg_par = (int) (run & 1);
            cg_iter(run % CG_RESET == CG_RESET - 1 ? 1 : 0);
            ++s;
            ++run;
        }
    }
    if (cg1 && nsteps > 0) {  // the residual after the batch's last iteration: trace, stop test (cg1_delta_kernel)
        const T *cur = cg1p.get() + (int64_t) (run & 1) * 4 * RED_BLOCKS;
        flush_psum();
        launch_cg1_delta<T>(gather_partials(const_cast<T *>(cur), 1, 4 * RED_BLOCKS), G, trace.get(), trace_cap, sc.get(), stream);
    }
    cg_scalars<T> h{};
    MI_HIP_CHECK(hipMemcpyAsync(&h, sc.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
    MI_HIP_CHECK(hipStreamSynchronize(stream));
    polled = h;
    converged = h.converged != 0;
    iters = h.iters;
}

template <typename T>
void engine<T>::cg_result(T *x_out, double *trace_out, int64_t trace_len, int64_t *iters) {
    if (!cg_active) throw mi_error(-6, "cg_result without cg_begin");
    MI_HIP_CHECK(hipSetDevice(device));
    cg_scalars<T> h{};
    MI_HIP_CHECK(hipMemcpyAsync(&h, sc.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
    if (x_out && m > 0) {
        if (gathered) allgather_rows(x.get());  // every rank's rows of the solution
        MI_HIP_CHECK(hipMemcpyAsync(x_out, x.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
    }
    MI_HIP_CHECK(hipStreamSynchronize(stream));
    const int64_t it = h.iters;
    if (iters) *iters = it;
    if (trace_out && trace_len > 0) {
        const int64_t cnt = std::min<int64_t>(std::min<int64_t>(trace_len, it + 1), trace_cap);
        MI_HIP_CHECK(hipMemcpy(trace_out, trace.get(), sizeof(double) * (size_t) cnt, hipMemcpyDeviceToHost));
    }
}

// batches of iterations between host polls (kernels after convergence exit at entry): 4, 8, 16,
// then up to the first reset, then whole CG_RESET blocks (one captured graph each in the single solve)
template <typename T>
int64_t engine<T>::poll_batch(int64_t done, int64_t imax, int64_t &batch) {
    const int64_t ns = std::min<int64_t>(done < CG_RESET ? std::min<int64_t>(batch, CG_RESET - done) : CG_RESET, imax - done);
    batch *= 2;
    return ns;
}

template <typename T>
void engine<T>::solve_cg(const T *b_host, const T *q_host, int64_t imax, T eps, T *x_out, double *trace_out,
                         int64_t *iters) {
    if (imax < 0) throw mi_error(-1, "imax must be >= 0");
    cg_begin(b_host, q_host, eps, false, nullptr, imax + 1);
    bool conv = false;
    int64_t it = 0, batch = 4;
    std::vector<double> seg;
    while (!conv && run < imax) {
        const int64_t first = it;
        const auto t0 = std::chrono::steady_clock::now();
        cg_step(poll_batch(run, imax, batch), conv, it);
        if (progress != nullptr && it > first) {
            // the batch's residuals delta_first .. delta_it (the iterations' "Start Iteration" lines,
            // OpenMP/csvm.cpp:115-117), the stop target and the batch's wall time
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            seg.resize((size_t) (it - first + 1));
            MI_HIP_CHECK(hipMemcpy(seg.data(), trace.get() + first, sizeof(double) * seg.size(), hipMemcpyDeviceToHost));
            progress(first, it - first, seg.data(), (double) polled.eps2delta0, ms, progress_user);
        }
    }
    cg_result(x_out, trace_out, imax + 1, iters);
}

template <typename T>
void engine<T>::learn_tail(const T *y, const T *q_host, T QA, T *alpha, double *bias_out) const {
    T s = 0, qa = 0;
    for (int64_t i = 0; i < m; ++i) s += alpha[i];
    for (int64_t i = 0; i < m; ++i) qa = std::fma(q_host[i], alpha[i], qa);
    const T bias = y[m] + QA * s - qa;  // (:257); QA = k_mm + (1/C)(1/s_m) with point weights
    alpha[m] = -s;                           // (:258)
    if (bias_out) *bias_out = (double) bias;
}

// csvm<T>::learn (src/plssvm/csvm.cpp:207-267)
template <typename T>
void engine<T>::learn(const T *y, int64_t imax, T eps, T *alpha_out, double *bias_out, double *trace_out,
                      int64_t *iters) {
    need_data();
    if (y == nullptr) throw mi_error(-1, "No labels given for training! Maybe the data is only usable for prediction?");
    std::vector<T> qh(std::max<int64_t>(m, 1)), bh(std::max<int64_t>(m, 1));
    generate_q(qh.data(), nullptr);
    for (int64_t i = 0; i < m; ++i) bh[i] = y[i] - y[m];  // b = y[0..m) - y[m]   (:238-239)
    if (imax < 0) imax = d;                                // solver_CG(b, num_features_, ...)  (:256)
    solve_cg(bh.data(), nullptr, imax, eps, alpha_out, trace_out, iters);
    learn_tail(y, qh.data(), QA_cost, alpha_out, bias_out);
}

// time_kp's cache eviction: reads n 16-byte words (their contents are never used; the sink is written only
// for a value no sweep produces in practice, which keeps the loads)
__global__ __launch_bounds__(256) void flush_read_kernel(const uint4 *__restrict__ a, int64_t n, unsigned *__restrict__ sink) {
    unsigned s = 0;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const uint4 v = a[i];
        s ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (s == 0x9E3779B9u) sink[0] = s;
}

template <typename T>
void engine<T>::time_kp(int reps, double *ms_kp, double *ms_dom) {
    need_data();
    need_q();
    MI_HIP_CHECK(hipSetDevice(device));
    if (reps < 1) reps = 1;
    std::vector<T> ph(std::max<int64_t>(m, 1));
    for (int64_t i = 0; i < m; ++i) ph[i] = T(1) + T((i * 2654435761ull) % 1000) / T(1000);
    if (m > 0) MI_HIP_CHECK(hipMemcpyAsync(pv.get(), ph.data(), sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
    MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
    hipEvent_t e0, e1, d0, d1;
    MI_HIP_CHECK(hipEventCreate(&e0));
    MI_HIP_CHECK(hipEventCreate(&e1));
    MI_HIP_CHECK(hipEventCreate(&d0));
    MI_HIP_CHECK(hipEventCreate(&d1));
    kp_device(pv.get(), ret.get(), T(1), true, nullptr);  // warm-up
    double dom = 0;
    MI_HIP_CHECK(hipEventRecord(e0, stream));
    for (int it = 0; it < reps; ++it) kp_device(pv.get(), ret.get(), T(1), true, nullptr);
    MI_HIP_CHECK(hipEventRecord(e1, stream));
    MI_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    MI_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    // dominant kernel alone (the pairwise tiles: always the implicit kernel over all tiles, never the stored ones — the
    // roofline built on this time is a statement about the MFMA kernel; ms_kp above is K·p as it runs, cache
    // included), same stream, same launches; before each launch a 512 MiB read sweep evicts what
    // the previous launch left in the L2s and the Infinity Cache (256 MiB), as the other kernels of a CG
    // iteration do between two launches — back-to-back launches would otherwise re-read part of their stream
    // from there (a read, not a memset: dirty lines would be written back during the timed launch)
    dev_buf<uint4> flush;
    try {
        flush.alloc(((int64_t) 512 << 20) / 16 + 1, stream, false);
    } catch (const mi_error &) {
        flush.reset();  // no room: time without the eviction
        (void) hipGetLastError();
    }
    for (int it = 0; it < reps; ++it) {
        if (flush.get() != nullptr) {
            hipLaunchKernelGGL(flush_read_kernel, dim3(4096), dim3(256), 0, stream, flush.get(), flush.size() - 1,
                               reinterpret_cast<unsigned *>(flush.get() + flush.size() - 1));
            MI_LAUNCH_CHECK();
        }
        MI_HIP_CHECK(hipEventRecord(d0, stream));
        if (sparse_stored()) {
            sparse_dominant(pv.get(), nullptr);
        } else if (factored()) {
            launch_gemv_n<T>(XT.get(), n_pad, d, r0, r1, w.get(), raw.get(), nullptr, stream);
        } else {
            launch_kp_tiles<T>(kp_geometry(), pv.get(), partial.get(), nullptr, stream);
        }
        MI_HIP_CHECK(hipEventRecord(d1, stream));
        MI_HIP_CHECK(hipEventSynchronize(d1));
        float t = 0;
        MI_HIP_CHECK(hipEventElapsedTime(&t, d0, d1));
        dom += t;
    }
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    (void) hipEventDestroy(d0);
    (void) hipEventDestroy(d1);
    if (ms_kp) *ms_kp = ms / reps;
    if (ms_dom) *ms_dom = dom / reps;
}

// ---- several right-hand sides over one pass of the tiles (engine.hpp "lanes") -------------------

// The batched path: the pairwise tile path on one rank with the reference recurrence. There G = 1, v0 = 0, vn = m,
// no collective, no centered finalize and no w pass riding with the direction update, so the steps (kp_sums ..
// cg_dir) launch on a pool lane exactly what they launch for the single solve there (need_pool). Everything else
// runs the right-hand sides one after another through the single-vector code.
template <typename T>
bool engine<T>::multi_batched() const {
    const bool tiles_path = !factored() && (!sparse || csr.dense_on);
    return have_data && tiles_path && m > 0 && kp_wgs > 0 && world == 1 && comm == nullptr && xchg == nullptr &&
           sim_world == 0 && !shard && !cg1_wanted() && multi_opt != 1;
}

template <typename T>
void engine<T>::need_pool() {
    dir_w_t<T> wo{};
    if (lanes.width < 2 || !multi_batched() || v0 != 0 || vn != m || G != 1 || gathered || ctr_active() || dir_w_fill(wo))
        throw mi_error(-6, "the batched path was entered on a setup it does not cover");
}

template <typename T>
int64_t engine<T>::lane_bytes(bool with_sinv, bool with_hold) const {
    return ((int64_t) (LV_COUNT + (with_sinv ? 1 : 0)) * q.size() + kp_wgs * KP_REC + 8 * RED_BLOCKS) * (int64_t) sizeof(T) +
           (int64_t) sizeof(cg_scalars<T>) + (with_hold ? q.size() : 0);
}

// Lanes are taken from what the setup (tile cache included) left free, keeping 256 MiB for the single path's own
// later needs (traces, a captured block): the widest of W, W / 2, ... that fits; 1 = not even two lanes fit.
template <typename T>
int engine<T>::multi_width_next(bool with_sinv, bool with_hold) const {
    if (!multi_batched()) return 1;
    if (lanes.width > 0) return lanes.width;
    size_t free_b = 0, total_b = 0;
    MI_HIP_CHECK(hipSetDevice(device));
    MI_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const int64_t room = (int64_t) free_b - ((int64_t) 256 << 20);
    int w = multi_opt >= 2 ? std::min(multi_opt, KP_MULTI_W) : KP_MULTI_W;
    while (w >= 2 && (int64_t) w * lane_bytes(with_sinv, with_hold) > room) w /= 2;
    return std::max(w, 1);
}

template <typename T>
int engine<T>::multi_lanes(bool with_sinv, bool with_hold) {
    if (!multi_batched()) return 1;
    if (lanes.width > 0) return lanes.width;
    for (int w = multi_width_next(with_sinv, with_hold); w >= 2; w /= 2) {
        try {
            lanes.vstride = q.size();
            lanes.sstride = kp_wgs * KP_REC;
            lanes.vec.alloc((int64_t) LV_COUNT * w * lanes.vstride, stream);
            lanes.slab.alloc((int64_t) w * lanes.sstride, stream, false);
            lanes.part.alloc((int64_t) w * 8 * RED_BLOCKS, stream);
            lanes.sc.alloc(w, stream);
            if (with_sinv) lanes.sinv.alloc((int64_t) w * lanes.vstride, stream);
            if (with_hold) lanes.hold.alloc((int64_t) w * lanes.vstride, stream);
            lanes.width = w;
            lanes_own_diag();
            return w;
        } catch (const mi_error &e) {
            if (e.code != -4) throw;
            (void) hipGetLastError();
            lanes = lane_pool{};
        }
    }
    lanes.width = 1;
    return 1;
}

// The weight vectors of a pool that was allocated without them (an earlier call had no per-lane weights). No room: the
// caller runs its lanes one after another.
template <typename T>
bool engine<T>::need_lane_sinv() {
    if (lanes.width < 2) return false;
    if (lanes.sinv.size() >= (int64_t) lanes.width * lanes.vstride) return true;
    try {
        lanes.sinv.alloc((int64_t) lanes.width * lanes.vstride, stream);
    } catch (const mi_error &e) {
        if (e.code != -4) throw;
        (void) hipGetLastError();
        lanes.sinv.reset();
        return false;
    }
    return true;
}

template <typename T>
bool engine<T>::need_lane_hold() {
    if (lanes.width < 2) return false;
    if (lanes.hold.size() >= (int64_t) lanes.width * lanes.vstride) return true;
    try {
        lanes.hold.alloc((int64_t) lanes.width * lanes.vstride, stream);
    } catch (const mi_error &e) {
        if (e.code != -4) throw;
        (void) hipGetLastError();
        lanes.hold.reset();
        return false;
    }
    return true;
}

template <typename T>
void engine<T>::lanes_own_diag() {
    lanes.diag.assign((size_t) std::max(lanes.width, 0), lane_diag{ cost_inv(), QAf(), sinv_dev(), nullptr });
}

// One pass over the tiles for the vectors `kind` of lanes [c0, c0 + nvec); flags: the lanes' stop flags apply.
// The stored records are streamed once they are filled; filling them is the single-vector path's job.
template <typename T>
void engine<T>::tiles_multi(int kind, int c0, int nvec, bool flags) {
    launch_kp_tiles_multi<T>(kp_geometry(), lane_v(kind, c0), lanes.vstride, lanes.slab.get() + (int64_t) c0 * lanes.sstride,
                             lanes.sstride, nvec, flags ? lanes.sc.get() + c0 : nullptr, stream, kc.view());
}

// kp_device for lanes [c0, c0 + nvec) with one pass over the tiles (engine.hpp)
template <typename T>
void engine<T>::kp_lanes(int kin, int kout, int c0, int nvec, T add, bool overwrite, bool flags, bool then_rr) {
    for (int c = c0; c < c0 + nvec; ++c) {
        const cg_lane L = pool_lane(c);
        kp_sums(lane_v(kin, c), L, flags ? L.sc : nullptr);
    }
    tiles_multi(kin, c0, nvec, flags);
    for (int c = c0; c < c0 + nvec; ++c) {
        const cg_lane L = pool_lane(c);
        const cg_scalars<T> *st = flags ? L.sc : nullptr;
        kp_slab_reduce(L, st);
        kp_fin(L, lane_v(kin, c), lane_v(kout, c), add, overwrite, st);
        if (then_rr) cg_rr(L, st);
    }
}

// cg_iter for nvec lanes: one batched tile launch on the direction vectors, then cg_iter's steps per lane
template <typename T>
void engine<T>::cg_iter_multi(int nvec, int reset) {
    tiles_multi(LV_D, 0, nvec, true);
    for (int c = 0; c < nvec; ++c) {
        const cg_lane L = pool_lane(c);
        kp_slab_reduce(L, L.sc);
        cg_fin_dad(L, L.d, L.pdad(), nullptr, 0);
        cg_upd_rr(L, reset);
    }
    if (reset) kp_lanes(LV_X, LV_R, 0, nvec, T(-1), false, true, true);  // r = b - Q~x, then its r.r
    for (int c = 0; c < nvec; ++c) cg_dir(pool_lane(c), 0);
}

// solve_cg for nvec <= width right-hand sides (B[c * ld + i]) as lanes 0 .. nvec - 1; q is set
template <typename T>
void engine<T>::solve_cg_group(const T *B, int nvec, int64_t ld, int64_t imax, T eps, T *X_out, double *trace_out,
                               int64_t *iters, bool held) {
    need_pool();
    // cg_begin per lane
    const cg_scalars<T> init = cg_scalars_init(eps, false);
    const std::vector<cg_scalars<T>> inits((size_t) nvec, init);
    MI_HIP_CHECK(hipMemcpyAsync(lanes.sc.get(), inits.data(), sizeof(init) * (size_t) nvec, hipMemcpyHostToDevice, stream));
    const int64_t cap = imax + 1;
    if (lanes.trace_cap != cap) {  // a lane's trace has the single solve's length (the kernels' bound)
        lanes.trace.alloc((int64_t) lanes.width * cap, stream);
        lanes.trace_cap = cap;
    } else {
        MI_HIP_CHECK(hipMemsetAsync(lanes.trace.get(), 0, sizeof(double) * (size_t) lanes.trace.size(), stream));
    }
    for (int c = 0; c < nvec; ++c) {
        MI_HIP_CHECK(hipMemcpyAsync(lane_v(LV_B, c), B + c * ld, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
        if (held) launch_cg_init_held<T>(lane_v(LV_B, c), lanes.diag[(size_t) c].hold, m, lane_v(LV_X, c), lane_v(LV_R, c), stream);
        else launch_cg_init<T>(lane_v(LV_B, c), m, lane_v(LV_X, c), lane_v(LV_R, c), stream);  // x = 1; r = b
    }
    if (held) {
        // x0 = 1 on the lane's own active rows: r -= Q~x per lane, one pass over the (filled) tiles for the group
        kp_lanes(LV_X, LV_R, 0, nvec, T(-1), false, false);
    } else {
        // r -= Q~x: x0 = 1 is the same for every lane, so kp_device's first half runs once, on the engine's own buffers
        // (sum p, sum q p in sc, the pairwise part in raw; with no stop flag it also fills an unfilled tile cache)
        MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
        kp_sums(lane_v(LV_X, 0), own_lane(), nullptr);
        kp_raw(lane_v(LV_X, 0), nullptr);
    }
    for (int c = 0; c < nvec; ++c) {
        const cg_lane L = pool_lane(c);
        if (!held) {
            cg_lane S = own_lane();  // the shared raw and sums, the lane's diagonal
            S.cost_inv = L.cost_inv, S.QA = L.QA, S.sinv = L.sinv;
            kp_fin(S, L.x, L.r, T(-1), false, nullptr);
        }
        cg_delta0(L);
        cg_dir(L, 1);
    }
    // solve_cg's polled batches; a converged lane's kernels leave at entry, the group stops when every lane has
    // converged
    std::vector<cg_scalars<T>> h((size_t) nvec);
    int64_t done = 0, batch = 4;
    bool conv = false;
    while (!conv && done < imax) {
        const int64_t ns = poll_batch(done, imax, batch);
        for (int64_t s = 0; s < ns; ++s, ++done) cg_iter_multi(nvec, done % CG_RESET == CG_RESET - 1 ? 1 : 0);
        MI_HIP_CHECK(hipMemcpyAsync(h.data(), lanes.sc.get(), sizeof(init) * (size_t) nvec, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        conv = true;
        for (int c = 0; c < nvec; ++c) conv = conv && h[(size_t) c].converged != 0;
    }
    if (imax == 0 || done == 0) {
        MI_HIP_CHECK(hipMemcpyAsync(h.data(), lanes.sc.get(), sizeof(init) * (size_t) nvec, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
    for (int c = 0; c < nvec; ++c) {
        const int64_t it = h[(size_t) c].iters;
        if (iters) iters[c] = it;
        MI_HIP_CHECK(hipMemcpyAsync(X_out + c * ld, lane_v(LV_X, c), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
        if (trace_out)
            MI_HIP_CHECK(hipMemcpyAsync(trace_out + c * cap, lanes.trace.get() + (int64_t) c * lanes.trace_cap,
                                        sizeof(double) * (size_t) std::min<int64_t>(cap, it + 1), hipMemcpyDeviceToHost, stream));
    }
    MI_HIP_CHECK(hipStreamSynchronize(stream));
}

template <typename T>
void engine<T>::solve_cg_multi(const T *B, int64_t nrhs, int64_t ld, const T *q_host, int64_t imax, T eps, T *X_out,
                               double *trace_out, int64_t *iters) {
    need_data();
    if (imax < 0) throw mi_error(-1, "imax must be >= 0");
    if (nrhs < 1) throw mi_error(-1, "at least one right-hand side is needed");
    if (ld < m) throw mi_error(-1, "the leading dimension is smaller than the number of rows");
    MI_HIP_CHECK(hipSetDevice(device));
    set_q(q_host);
    const int W = multi_lanes();
    if (W < 2 || nrhs == 1) {  // one at a time through the single solve
        for (int64_t c = 0; c < nrhs; ++c)
            solve_cg(B + c * ld, nullptr, imax, eps, X_out + c * ld, trace_out ? trace_out + c * (imax + 1) : nullptr,
                     iters ? iters + c : nullptr);
        return;
    }
    cg_active = false;  // the group borrows sc, red, raw and the slab of the single solve
    lanes_own_diag();
    for (int64_t c0 = 0; c0 < nrhs; c0 += W)
        solve_cg_group(B + c0 * ld, (int) std::min<int64_t>(W, nrhs - c0), ld, imax, eps, X_out + c0 * ld,
                       trace_out ? trace_out + c0 * (imax + 1) : nullptr, iters ? iters + c0 : nullptr);
}

// RET_c += add * Q~ P_c for nrhs columns (row c of P / RET at c * ld)
template <typename T>
void engine<T>::kp_multi(const T *q_host, const T *P, T *RET, int64_t nrhs, int64_t ld, T add) {
    need_data();
    if (nrhs < 1) throw mi_error(-1, "at least one vector is needed");
    if (ld < m) throw mi_error(-1, "the leading dimension is smaller than the number of rows");
    MI_HIP_CHECK(hipSetDevice(device));
    const int W = nrhs == 1 ? 1 : multi_lanes();
    if (W < 2) {
        for (int64_t c = 0; c < nrhs; ++c) kp_host(q_host, P + c * ld, RET + c * ld, add);
        return;
    }
    set_q(q_host);
    need_pool();
    cg_active = false;
    lanes_own_diag();
    for (int64_t c0 = 0; c0 < nrhs; c0 += W) {
        const int nvec = (int) std::min<int64_t>(W, nrhs - c0);
        MI_HIP_CHECK(hipMemsetAsync(lanes.sc.get(), 0, sizeof(cg_scalars<T>) * (size_t) nvec, stream));
        for (int c = 0; c < nvec; ++c) {
            MI_HIP_CHECK(hipMemcpyAsync(lane_v(LV_D, c), P + (c0 + c) * ld, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
            MI_HIP_CHECK(hipMemcpyAsync(lane_v(LV_R, c), RET + (c0 + c) * ld, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
        }
        int first = 0;
        if (kc.tiles > 0 && !kc.valid) {  // an unfilled tile cache: the first vector fills it, on the single path
            MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
            kp_device(lane_v(LV_D, 0), lane_v(LV_R, 0), add, false, nullptr);
            first = 1;
        }
        if (nvec > first) kp_lanes(LV_D, LV_R, first, nvec - first, add, false, false);
        for (int c = 0; c < nvec; ++c)
            MI_HIP_CHECK(hipMemcpyAsync(RET + (c0 + c) * ld, lane_v(LV_R, c), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

// learn() per class of a one-vs-all label matrix Y[nclass][ldy] (+-1), the solves as one multi-right-hand-side CG
template <typename T>
void engine<T>::learn_multi(const T *Y, int64_t nclass, int64_t ldy, int64_t imax, T eps, T *alpha_out, double *bias_out,
                            double *trace_out, int64_t *iters) {
    learn_lanes(Y, nclass, ldy, nullptr, nullptr, 0, imax, eps, alpha_out, bias_out, trace_out, iters);
}

// ---- point weights and lanes that differ in their diagonal ---------------------------------------
template <typename T>
void engine<T>::check_weights(const T *s, int64_t count) {
    for (int64_t i = 0; i < count; ++i) {
        const T r = T(1) / s[i];
        if (!(s[i] > T(0)) || !std::isfinite(s[i]) || !(r > T(0)) || !std::isfinite(r))
            throw mi_error(-1, "point weight " + std::to_string(i) + " is not a finite number > 0 (with a finite reciprocal)");
    }
}

template <typename T>
void engine<T>::set_sinv(const std::vector<T> &sinv_new) {
    MI_HIP_CHECK(hipSetDevice(device));
    if (!sinv_new.empty()) {
        if (sinv.size() < q.size()) sinv.alloc(q.size(), stream);
        if (m > 0) MI_HIP_CHECK(hipMemcpyAsync(sinv.get(), sinv_new.data(), sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (&sinv_new != &sinv_h) sinv_h = sinv_new;
    // a q in place keeps a QA_cost that matches the diagonal, as generate_q would form it now
    if (have_q) QA_cost = host_kernel<T>(kernel, degree, gamma, coef0, xlast_h.data(), xlast_h.data(), d) + diag_m();
    graph_reset();  // a captured CG block holds the pointer and QA_cost
}

template <typename T>
void engine<T>::set_point_weights(const T *s) {
    if (!have_data) throw mi_error(-1, "point weights are set after a setup (they belong to its points)");
    std::vector<T> inv;
    if (s != nullptr) {
        check_weights(s, n);
        inv.resize((size_t) n);
        for (int64_t i = 0; i < n; ++i) inv[(size_t) i] = T(1) / s[i];
    }
    set_sinv(inv);
}

// What learn_lanes and learn_held check of their common arguments, and the lanes' costs in T (costs null: the engine's)
template <typename T>
std::vector<T> engine<T>::check_lane_args(const T *Y, int64_t nlane, int64_t ldy, const double *costs, const T *S,
                                          int64_t lds) const {
    if (Y == nullptr) throw mi_error(-1, "No labels given for training! Maybe the data is only usable for prediction?");
    if (nlane < 1) throw mi_error(-1, "at least one class is needed");
    if (ldy < n) throw mi_error(-1, "the leading dimension is smaller than the number of points");
    if (S != nullptr && lds != 0 && lds < n) throw mi_error(-1, "the weights' leading dimension is smaller than the number of points");
    std::vector<T> cost_k((size_t) nlane, cost);
    if (costs != nullptr)
        for (int64_t k = 0; k < nlane; ++k) {
            const T c = (T) costs[k], r = T(1) / c;
            if (!(costs[k] > 0) || !std::isfinite(c) || !(c > T(0)) || !std::isfinite(r) || !(r > T(0)))
                throw mi_error(-1, "cost " + std::to_string(k) + " is not a finite number > 0");
            cost_k[(size_t) k] = c;
        }
    if (S != nullptr)
        for (int64_t k = 0; k < (lds != 0 ? nlane : 1); ++k) check_weights(S + k * lds, n);
    return cost_k;
}

// the n reciprocals of a weight row
template <typename T>
std::vector<T> engine<T>::recip_weights(const T *s) const {
    std::vector<T> inv((size_t) n);
    for (int64_t i = 0; i < n; ++i) inv[(size_t) i] = T(1) / s[i];
    return inv;
}

template <typename T>
void engine<T>::learn_lanes(const T *Y, int64_t nlane, int64_t ldy, const double *costs, const T *S, int64_t lds,
                            int64_t imax, T eps, T *alpha_out, double *bias_out, double *trace_out, int64_t *iters) {
    need_data();
    const std::vector<T> cost_k = check_lane_args(Y, nlane, ldy, costs, S, lds);
    const bool per_lane = S != nullptr && lds != 0;
    auto recip = [&](const T *s) { return recip_weights(s); };
    MI_HIP_CHECK(hipSetDevice(device));
    const T cost0 = cost;
    const std::vector<T> sinv0 = sinv_h;
    bool cost_touched = false, sinv_touched = false;  // what the call changed on the engine, for restore
    auto run = [&]() {
        if (S != nullptr && !per_lane) {  // one row for all lanes: the context's weights for this call
            sinv_touched = true;
            set_sinv(recip(S));
        }
        std::vector<T> qh(std::max<int64_t>(m, 1)), bh((size_t) (nlane * ldy));  // b rows ldy apart, like alpha_out's
        generate_q(qh.data(), nullptr);
        for (int64_t c = 0; c < nlane; ++c)
            for (int64_t i = 0; i < m; ++i) bh[(size_t) (c * ldy + i)] = Y[c * ldy + i] - Y[c * ldy + m];  // b = y - y_m
        if (imax < 0) imax = d;
        const int64_t cap = imax + 1;
        const int W = nlane == 1 ? 1 : multi_lanes(per_lane);
        if (W < 2 || (per_lane && !need_lane_sinv())) {
            // one after another through the single solve, the engine's cost and weights set per lane
            for (int64_t k = 0; k < nlane; ++k) {
                cost_touched = cost_touched || costs != nullptr;
                cost = cost_k[(size_t) k];
                if (per_lane) {
                    sinv_touched = true;
                    set_sinv(recip(S + k * lds));
                }
                QA_cost = ctr_kmm + diag_m();  // generate_q's, at this lane's cost and weights
                solve_cg(bh.data() + k * ldy, nullptr, imax, eps, alpha_out + k * ldy, trace_out ? trace_out + k * cap : nullptr,
                         iters ? iters + k : nullptr);
                learn_tail(Y + k * ldy, qh.data(), QA_cost, alpha_out + k * ldy, bias_out ? bias_out + k : nullptr);
            }
            return;
        }
        need_pool();
        cg_active = false;  // the group borrows sc, red, raw and the slab of the single solve
        std::vector<T> QA((size_t) nlane);
        for (int64_t c0 = 0; c0 < nlane; c0 += W) {
            const int nvec = (int) std::min<int64_t>(W, nlane - c0);
            std::vector<std::vector<T>> inv((size_t) nvec);  // alive until the group's last synchronisation
            for (int c = 0; c < nvec; ++c) {
                const int64_t k = c0 + c;
                const T cinv = T(1) / cost_k[(size_t) k];
                T dm = cinv;
                const T *sv = sinv_dev();
                if (per_lane) {
                    inv[(size_t) c] = recip(S + k * lds);
                    MI_HIP_CHECK(hipMemcpyAsync(lane_sinv(c), inv[(size_t) c].data(), sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
                    sv = lane_sinv(c);
                    dm = cinv * inv[(size_t) c][(size_t) m];
                } else if (weighted()) {
                    dm = cinv * sinv_h[(size_t) m];
                }
                QA[(size_t) k] = ctr_kmm + dm;
                lanes.diag[(size_t) c] = lane_diag{ cinv, QA[(size_t) k], sv, nullptr };
            }
            solve_cg_group(bh.data() + c0 * ldy, nvec, ldy, imax, eps, alpha_out + c0 * ldy,
                           trace_out ? trace_out + c0 * cap : nullptr, iters ? iters + c0 : nullptr);
        }
        for (int64_t k = 0; k < nlane; ++k)
            learn_tail(Y + k * ldy, qh.data(), QA[(size_t) k], alpha_out + k * ldy, bias_out ? bias_out + k : nullptr);
    };
    // only what was touched: an unweighted learn_multi keeps its captured graph and pays no extra synchronisation
    auto restore = [&]() {
        cost = cost0;
        if (sinv_touched) {
            set_sinv(sinv0);  // with the QA_cost that goes with them
        } else if (cost_touched) {
            QA_cost = ctr_kmm + diag_m();  // generate_q's (it ran before the cost moved)
            graph_reset();
        }
    };
    try {
        run();
    } catch (...) {
        try {
            restore();
        } catch (...) {
        }
        throw;
    }
    restore();
}

// ---- held-out points as masked lanes (engine.hpp) ---------------------------------------------------
// Where the finalize is kp_finalize_kernel / cg_fin_dad_kernel and nothing else: the pairwise tile path on one rank with
// the reference recurrence (multi_batched() without its width option)
template <typename T>
bool engine<T>::held_supported() const {
    const bool tiles_path = !factored() && (!sparse || csr.dense_on);
    return have_data && tiles_path && m > 0 && kp_wgs > 0 && world == 1 && comm == nullptr && xchg == nullptr &&
           sim_world == 0 && !shard && !cg1_wanted();
}

template <typename T>
void engine<T>::learn_held(const T *Y, int64_t nlane, int64_t ldy, const double *costs, const T *S, int64_t lds,
                           const uint8_t *HOLD, int64_t ldh, int64_t imax, T eps, T *alpha_out, double *bias_out,
                           double *trace_out, int64_t *iters, int64_t *pivots_out) {
    need_data();
    if (HOLD == nullptr) {
        learn_lanes(Y, nlane, ldy, costs, S, lds, imax, eps, alpha_out, bias_out, trace_out, iters);
        if (pivots_out) std::fill(pivots_out, pivots_out + nlane, m);
        return;
    }
    const std::vector<T> cost_k = check_lane_args(Y, nlane, ldy, costs, S, lds);
    const bool per_lane = S != nullptr && lds != 0;
    if (ldh != 0 && ldh < n) throw mi_error(-1, "the hold rows' leading dimension is smaller than the number of points");
    if (!held_supported()) {
        const char *why = sparse_stored()              ? "a stored sparse setup"
                          : factored()                 ? "the factored linear path"
                          : (sim_world > 0)            ? "a simulated rank"
                          : (world > 1 || comm != nullptr || xchg != nullptr || shard) ? "a multi-GPU group"
                          : cg1_wanted()               ? "the one-reduction CG"
                                                       : "a setup without kernel-matrix tiles";
        throw mi_error(-5, std::string("held-out lanes run on the pairwise tile path of one GPU with the reference CG; this "
                                       "context is ") + why + " (train on the subset with a fresh setup instead)");
    }
    // the pivots: the largest training index of every lane; lanes by pivot, pivot m first, then by first appearance
    std::vector<int64_t> piv((size_t) nlane);
    std::vector<int64_t> pivot_order;
    for (int64_t k = 0; k < nlane; ++k) {
        const uint8_t *h = HOLD + k * ldh;
        int64_t t = -1, cnt = 0;
        for (int64_t i = 0; i < n; ++i)
            if (h[i] == 0) t = i, ++cnt;
        if (cnt < 2) throw mi_error(-1, "lane " + std::to_string(k) + " has fewer than two training points");
        piv[(size_t) k] = t;
        if (std::find(pivot_order.begin(), pivot_order.end(), t) == pivot_order.end()) pivot_order.push_back(t);
    }
    std::stable_partition(pivot_order.begin(), pivot_order.end(), [&](int64_t t) { return t == m; });
    if (pivots_out) std::copy(piv.begin(), piv.end(), pivots_out);
    auto recip = [&](const T *s) { return recip_weights(s); };
    MI_HIP_CHECK(hipSetDevice(device));
    const T cost0 = cost;
    const std::vector<T> sinv0 = sinv_h;
    bool cost_touched = false, sinv_touched = false, q_touched = false;
    auto run = [&]() {
        if (S != nullptr && !per_lane) {
            sinv_touched = true;
            set_sinv(recip(S));
        }
        std::vector<T> qm(std::max<int64_t>(m, 1)), qt;
        generate_q(qm.data(), nullptr);
        if (imax < 0) imax = d;
        const int64_t cap = imax + 1;
        const int W = nlane == 1 ? 1 : multi_lanes(per_lane, true);
        const bool batched = W >= 2 && need_lane_hold() && (!per_lane || need_lane_sinv());
        if (hold_own.size() < q.size()) hold_own.alloc(q.size(), stream);
        if (batched) {
            need_pool();
            if (kc.tiles > 0 && !kc.valid) {  // the batched launch streams filled records only: one single-path pass fills them
                MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
                MI_HIP_CHECK(hipMemsetAsync(pv.get(), 0, sizeof(T) * (size_t) pv.size(), stream));
                kp_raw(pv.get(), nullptr);
            }
        }
        cg_active = false;
        for (const int64_t t : pivot_order) {
            std::vector<int64_t> ks;
            for (int64_t k = 0; k < nlane; ++k)
                if (piv[(size_t) k] == t) ks.push_back(k);
            const T *qh = qm.data();
            T ktt = ctr_kmm;
            if (t != m) {
                // q = column t of the kernel matrix: K e_t over the tiles, as kp_part forms it
                const T one = T(1);
                MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
                MI_HIP_CHECK(hipMemsetAsync(pv.get(), 0, sizeof(T) * (size_t) pv.size(), stream));
                MI_HIP_CHECK(hipMemcpyAsync(pv.get() + t, &one, sizeof(T), hipMemcpyHostToDevice, stream));
                q_touched = true;
                kp_raw(pv.get(), nullptr);
                MI_HIP_CHECK(hipMemcpyAsync(q.get(), raw.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToDevice, stream));
                qt.resize((size_t) m);
                MI_HIP_CHECK(hipMemcpyAsync(qt.data(), raw.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
                MI_HIP_CHECK(hipStreamSynchronize(stream));
                q_gen = false;
                graph_reset();
                qh = qt.data();
                ktt = qt[(size_t) t];
            }
            // a lane's mask (rows that are no part of its system: held, or from the pivot on), b and QA
            const int64_t nk = (int64_t) ks.size();
            std::vector<uint8_t> mask((size_t) (nk * m));
            // rows n apart (not the caller's ldy): the host memory of a pivot's lanes does not grow with ldy
            std::vector<T> bh((size_t) (nk * n), T(0)), xt((size_t) (nk * n), T(0)), QA((size_t) nk);
            std::vector<double> tr(trace_out ? (size_t) (nk * cap) : 0);
            std::vector<int64_t> it((size_t) nk);
            std::vector<std::vector<T>> inv((size_t) nk);
            for (int64_t j = 0; j < nk; ++j) {
                const int64_t k = ks[(size_t) j];
                const uint8_t *h = HOLD + k * ldh;
                const T *y = Y + k * ldy;
                for (int64_t i = 0; i < m; ++i) {
                    const bool off = h[i] != 0 || i >= t;
                    mask[(size_t) (j * m + i)] = off ? 1 : 0;
                    bh[(size_t) (j * n + i)] = off ? T(0) : y[i] - y[t];
                }
                const T cinv = T(1) / cost_k[(size_t) k];
                T dt = cinv;
                if (per_lane) {
                    inv[(size_t) j] = recip(S + k * lds);
                    dt = cinv * inv[(size_t) j][(size_t) t];
                } else if (weighted()) {
                    dt = cinv * sinv_h[(size_t) t];
                }
                QA[(size_t) j] = ktt + dt;
            }
            if (batched) {
                for (int64_t j0 = 0; j0 < nk; j0 += W) {
                    const int nvec = (int) std::min<int64_t>(W, nk - j0);
                    for (int c = 0; c < nvec; ++c) {
                        const int64_t j = j0 + c;
                        const T *sv = sinv_dev();
                        if (per_lane) {
                            MI_HIP_CHECK(hipMemcpyAsync(lane_sinv(c), inv[(size_t) j].data(), sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
                            sv = lane_sinv(c);
                        }
                        MI_HIP_CHECK(hipMemcpyAsync(lane_hold(c), mask.data() + j * m, (size_t) m, hipMemcpyHostToDevice, stream));
                        lanes.diag[(size_t) c] = lane_diag{ T(1) / cost_k[(size_t) ks[(size_t) j]], QA[(size_t) j], sv, lane_hold(c) };
                    }
                    solve_cg_group(bh.data() + j0 * n, nvec, n, imax, eps, xt.data() + j0 * n,
                                   trace_out ? tr.data() + j0 * cap : nullptr, it.data() + j0, true);
                }
                lanes_own_diag();  // no later group meets this call's hold rows
            } else {
                for (int64_t j = 0; j < nk; ++j) {
                    const int64_t k = ks[(size_t) j];
                    cost_touched = cost_touched || costs != nullptr;
                    cost = cost_k[(size_t) k];
                    if (per_lane) {
                        sinv_touched = true;
                        set_sinv(inv[(size_t) j]);
                    }
                    QA_cost = QA[(size_t) j];
                    cost_touched = true;  // QA_cost is this lane's pivot's
                    MI_HIP_CHECK(hipMemcpyAsync(hold_own.get(), mask.data() + j * m, (size_t) m, hipMemcpyHostToDevice, stream));
                    hold_cur = hold_own.get();
                    solve_cg(bh.data() + j * n, nullptr, imax, eps, xt.data() + j * n, trace_out ? tr.data() + j * cap : nullptr,
                             it.data() + j);
                    hold_cur = nullptr;
                    graph_reset();
                }
            }
            // learn()'s end with t in the last point's part, in the caller's lane order
            for (int64_t j = 0; j < nk; ++j) {
                const int64_t k = ks[(size_t) j];
                T *a = alpha_out + k * ldy;
                std::copy(xt.begin() + j * n, xt.begin() + j * n + m, a);
                a[m] = T(0);
                if (t == m) {
                    learn_tail(Y + k * ldy, qh, QA[(size_t) j], a, bias_out ? bias_out + k : nullptr);
                } else {
                    T s = 0, qa = 0;
                    for (int64_t i = 0; i < m; ++i) s += a[i];
                    for (int64_t i = 0; i < m; ++i) qa = std::fma(qh[i], a[i], qa);
                    const T bias = Y[k * ldy + t] + QA[(size_t) j] * s - qa;
                    a[t] = -s;
                    if (bias_out) bias_out[k] = (double) bias;
                }
                if (iters) iters[k] = it[(size_t) j];
                if (trace_out) std::copy(tr.begin() + j * cap, tr.begin() + (j + 1) * cap, trace_out + k * cap);
            }
        }
    };
    auto restore = [&]() {
        hold_cur = nullptr;
        cost = cost0;
        if (lanes.width >= 2) lanes_own_diag();
        if (sinv_touched) set_sinv(sinv0);
        if (q_touched) generate_q(nullptr, nullptr);  // the last point's q and the QA_cost of the restored diagonal
        else if (cost_touched && !sinv_touched) QA_cost = ctr_kmm + diag_m();  // generate_q's (it ran before the cost moved)
        graph_reset();
    };
    try {
        run();
    } catch (...) {
        try {
            restore();
        } catch (...) {
        }
        throw;
    }
    restore();
}

template <typename T>
void engine<T>::train_values(const T *ALPHA, int64_t nclass, int64_t lda, const double *bias, T *OUT, int64_t ldo) {
    need_data();
    if (ALPHA == nullptr || OUT == nullptr || bias == nullptr) throw mi_error(-1, "train_values needs alpha, bias and an output");
    if (nclass < 1) throw mi_error(-1, "at least one model is needed");
    if (lda < n || ldo < n) throw mi_error(-1, "a leading dimension is smaller than the number of points");
    // a simulated rank's K·p is its share only, and a group's ranks would each need the others' rows of q and alpha
    if (sim_world > 0 || world > 1 || comm != nullptr || xchg != nullptr || shard)
        throw mi_error(-5, std::string("train_values runs on one GPU; this context is ") +
                               (sim_world > 0 ? "a simulated rank" : "part of a multi-GPU group") + " (predict on the points instead)");
    MI_HIP_CHECK(hipSetDevice(device));
    if (!(have_q && q_gen) || (int64_t) q_gen_h.size() != m) {
        // a caller's q is replaced by the generated one; a QA_cost in place (plssvm_mi_set_qa_cost) stays
        const bool had = have_q;
        const T qa0 = QA_cost;
        generate_q(nullptr, nullptr);
        if (had) QA_cost = qa0;
    }
    cg_active = false;
    // the last point: sum_j q_j alpha_j as an fma chain in index order (learn_tail's), then k_mm alpha_m, then the bias
    for (int64_t c = 0; c < nclass; ++c) {
        const T *a = ALPHA + c * lda;
        T acc = 0;
        for (int64_t j = 0; j < m; ++j) acc = std::fma(q_gen_h[(size_t) j], a[j], acc);
        const T last = ctr_kmm * a[m];
        OUT[c * ldo + m] = (acc + last) + (T) bias[c];
    }
    if (m <= 0) return;
    const int W = nclass == 1 ? 1 : multi_lanes();
    if (W < 2) {  // one vector after another: kp_part's K·p, then the finalize
        for (int64_t c = 0; c < nclass; ++c) {
            const T *a = ALPHA + c * lda;
            MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
            MI_HIP_CHECK(hipMemcpyAsync(pv.get(), a, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
            kp_raw(pv.get(), nullptr);
            launch_train_values_fin<T>(raw.get(), q.get(), a[m], (T) bias[c], m, ret.get(), stream);
            MI_HIP_CHECK(hipMemcpyAsync(OUT + c * ldo, ret.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
            MI_HIP_CHECK(hipStreamSynchronize(stream));
        }
        return;
    }
    need_pool();
    for (int64_t c0 = 0; c0 < nclass; c0 += W) {
        const int nvec = (int) std::min<int64_t>(W, nclass - c0);
        for (int c = 0; c < nvec; ++c)
            MI_HIP_CHECK(hipMemcpyAsync(lane_v(LV_D, c), ALPHA + (c0 + c) * lda, sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
        int first = 0;
        if (kc.tiles > 0 && !kc.valid) {  // an unfilled tile cache: the first vector fills it, on the single path
            MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
            kp_raw(lane_v(LV_D, 0), nullptr);
            launch_train_values_fin<T>(raw.get(), q.get(), ALPHA[c0 * lda + m], (T) bias[c0], m, lane_v(LV_R, 0), stream);
            first = 1;
        }
        if (nvec > first) tiles_multi(LV_D, first, nvec - first, false);
        for (int c = first; c < nvec; ++c) {
            const cg_lane L = pool_lane(c);
            kp_slab_reduce(L, nullptr);
            launch_train_values_fin<T>(L.raw, q.get(), ALPHA[(c0 + c) * lda + m], (T) bias[c0 + c], m, lane_v(LV_R, c), stream);
        }
        for (int c = 0; c < nvec; ++c)
            MI_HIP_CHECK(hipMemcpyAsync(OUT + (c0 + c) * ldo, lane_v(LV_R, c), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

// time_kp's K·p time for the batched product of nrhs resident vectors (groups of at most the width; one at a time
// where nothing is batched): dots, tiles, reduce and finalize of every vector
template <typename T>
void engine<T>::time_kp_multi(int64_t nrhs, int reps, double *ms_kp) {
    need_data();
    need_q();
    if (nrhs < 1) throw mi_error(-1, "at least one vector is needed");
    MI_HIP_CHECK(hipSetDevice(device));
    if (reps < 1) reps = 1;
    const int W = multi_lanes();
    if (W >= 2) need_pool(), lanes_own_diag();
    cg_active = false;
    std::vector<T> ph(std::max<int64_t>(m, 1));
    for (int64_t i = 0; i < m; ++i) ph[i] = T(1) + T((i * 2654435761ull) % 1000) / T(1000);
    T *p0 = W < 2 ? pv.get() : lane_v(LV_D, 0);
    const int nl = W < 2 ? 1 : (int) std::min<int64_t>(W, nrhs);
    for (int c = 0; c < nl; ++c)
        if (m > 0) MI_HIP_CHECK(hipMemcpyAsync(W < 2 ? p0 : lane_v(LV_D, c), ph.data(), sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
    MI_HIP_CHECK(hipMemsetAsync(sc.get(), 0, sizeof(cg_scalars<T>), stream));
    if (W >= 2) MI_HIP_CHECK(hipMemsetAsync(lanes.sc.get(), 0, sizeof(cg_scalars<T>) * (size_t) W, stream));
    kp_device(p0, ret.get(), T(1), true, nullptr);  // warm-up; fills an unfilled tile cache
    auto product = [&]() {
        if (W < 2) {
            for (int64_t c = 0; c < nrhs; ++c) kp_device(p0, ret.get(), T(1), true, nullptr);
            return;
        }
        for (int64_t c0 = 0; c0 < nrhs; c0 += W)
            kp_lanes(LV_D, LV_R, 0, (int) std::min<int64_t>(W, nrhs - c0), T(1), true, false);
    };
    product();  // warm-up
    hipEvent_t e0, e1;
    MI_HIP_CHECK(hipEventCreate(&e0));
    MI_HIP_CHECK(hipEventCreate(&e1));
    MI_HIP_CHECK(hipEventRecord(e0, stream));
    for (int it = 0; it < reps; ++it) product();
    MI_HIP_CHECK(hipEventRecord(e1, stream));
    MI_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    MI_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    if (ms_kp) *ms_kp = ms / reps;
}

template <typename T>
int64_t engine<T>::device_bytes() const {
    return XT.bytes() + norms.bytes() + xlast.bytes() + partial.bytes() + kc.bytes() + q.bytes() * 10 + w.bytes() +
           csr_bytes() + lanes.bytes() + sinv.bytes();
}

template struct engine<float>;
template struct engine<double>;

}  // namespace plssvm_mi
