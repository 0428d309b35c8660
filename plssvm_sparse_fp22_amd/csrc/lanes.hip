// engine<T>: several right-hand sides over one pass of the tiles (engine.hpp "lanes"): the lane pool,
// the batched K·p and CG, point weights, the multi-lane learn (its host half: lane_plan.hpp) and train_values.
#include <algorithm>
#include <cmath>

#include "engine.hpp"
#include "lane_plan.hpp"

namespace plssvm_mi {

// Where the finalize is kp_finalize_kernel / cg_fin_dad_kernel and nothing else: the pairwise tile path on one rank with
// the reference recurrence. There G = 1, v0 = 0, vn = m, no collective, no centered finalize and no w pass riding with
// the direction update, so the steps (kp_sums .. cg_dir) launch on a pool lane exactly what they launch for the single
// solve there (need_pool). Held-out lanes are offered here, at any width.
template <typename T>
bool engine<T>::held_supported() const {
    const bool tiles_path = !factored() && (!sparse || csr.dense_on);
    return have_data && tiles_path && m > 0 && kp_wgs > 0 && world == 1 && comm == nullptr && xchg == nullptr &&
           sim_world == 0 && !shard && !cg1_wanted();
}

// The batched path: there, unless the width option says one at a time. Everything else runs the right-hand sides one
// after another through the single-vector code.
template <typename T>
bool engine<T>::multi_batched() const {
    return held_supported() && multi_opt != 1;
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

// A per-lane buffer (lanes.sinv, lanes.hold) of a pool that was allocated without it (no earlier call passed per-lane
// weights / hold rows). No room: the caller runs its lanes one after another.
template <typename T>
template <typename U>
bool engine<T>::need_lane_buf(dev_buf<U> &buf) {
    if (lanes.width < 2) return false;
    if (buf.size() >= (int64_t) lanes.width * lanes.vstride) return true;
    try {
        buf.alloc((int64_t) lanes.width * lanes.vstride, stream);
    } catch (const mi_error &e) {
        if (e.code != -4) throw;
        (void) hipGetLastError();
        buf.reset();
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
        // an unfilled tile cache: the first vector fills it
        const int first = fill_tiles([&] { kp_device(lane_v(LV_D, 0), lane_v(LV_R, 0), add, false, nullptr); }) ? 1 : 0;
        if (nvec > first) kp_lanes(LV_D, LV_R, first, nvec - first, add, false, false);
        for (int c = 0; c < nvec; ++c)
            MI_HIP_CHECK(hipMemcpyAsync(RET + (c0 + c) * ld, lane_v(LV_R, c), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

// ---- point weights -------------------------------------------------------------------------------
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
    if (have_q) QA_cost = k_mm() + diag_m();
    graph_reset();  // a captured CG block holds the pointer and QA_cost
}

template <typename T>
void engine<T>::set_point_weights(const T *s) {
    if (!have_data) throw mi_error(-1, "point weights are set after a setup (they belong to its points)");
    std::vector<T> inv;
    if (s != nullptr) {
        check_weights(s, n);
        inv = recip_weights(s, n);
    }
    set_sinv(inv);
}

// ---- the multi-lane learn: classes, costs, weights and held-out points as lanes (engine.hpp)
template <typename T>
void engine<T>::learn_held(const T *Y, int64_t nlane, int64_t ldy, const double *costs, const T *S, int64_t lds,
                           const uint8_t *HOLD, int64_t ldh, int64_t imax, T eps, T *alpha_out, double *bias_out,
                           double *trace_out, int64_t *iters, int64_t *pivots_out) {
    need_data();
    const lane_plan<T> plan(n, cost, Y, nlane, ldy, costs, S, lds, HOLD, ldh);  // every argument check
    const bool held = HOLD != nullptr, per_lane = S != nullptr && lds != 0;
    if (held && !held_supported()) {
        const char *why = sparse_stored()              ? "a stored sparse setup"
                          : factored()                 ? "the factored linear path"
                          : (sim_world > 0)            ? "a simulated rank"
                          : (world > 1 || comm != nullptr || xchg != nullptr || shard) ? "a multi-GPU group"
                          : cg1_wanted()               ? "the one-reduction CG"
                                                       : "a setup without kernel-matrix tiles";
        throw mi_error(-5, std::string("held-out lanes run on the pairwise tile path of one GPU with the reference CG; this "
                                       "context is ") + why + " (train on the subset with a fresh setup instead)");
    }
    if (pivots_out)
        for (int64_t k = 0; k < nlane; ++k) pivots_out[k] = plan.lanes[(size_t) k].t;
    MI_HIP_CHECK(hipSetDevice(device));
    const T cost0 = cost;
    const std::vector<T> sinv0 = sinv_h;
    // what the call moved on the engine, for restore: the cost (with QA_cost), the weights, q, own_lane()'s hold rows
    struct {
        bool cost = false, sinv = false, q = false, hold = false;
    } moved;
    auto run = [&]() {
        if (plan.shared != nullptr) {  // one row for all lanes: the context's weights for this call
            moved.sinv = true;
            set_sinv(recip_weights(plan.shared, n));
        }
        std::vector<T> qm(std::max<int64_t>(m, 1)), qt;
        generate_q(qm.data(), nullptr);
        if (imax < 0) imax = d;
        const int64_t cap = imax + 1;
        const int W = nlane == 1 ? 1 : multi_lanes(per_lane, held);
        const bool batched = W >= 2 && (!held || need_lane_buf(lanes.hold)) && (!per_lane || need_lane_buf(lanes.sinv));
        if (held && hold_own.size() < q.size()) hold_own.alloc(q.size(), stream);
        if (batched) {
            need_pool();
            // a held lane's first product is its own, batched: one single-path pass of a zero vector fills the records
            // (without hold rows the group's shared first product fills them)
            if (held) fill_tiles([&] { kp_raw_of(nullptr); });
        }
        cg_active = false;  // a group borrows sc, red, raw and the slab of the single solve
        for (const auto &g : plan.groups) {
            const int64_t t = g.t, nk = (int64_t) g.ks.size();
            const T *qh = qm.data();
            T ktt = ctr_kmm;
            if (t != m) {
                // q = column t of the kernel matrix: K e_t over the tiles
                moved.q = true;
                kp_raw_of(nullptr, t);
                MI_HIP_CHECK(hipMemcpyAsync(q.get(), raw.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToDevice, stream));
                qt.resize((size_t) m);
                MI_HIP_CHECK(hipMemcpyAsync(qt.data(), raw.get(), sizeof(T) * (size_t) m, hipMemcpyDeviceToHost, stream));
                MI_HIP_CHECK(hipStreamSynchronize(stream));
                q_gen = false;
                graph_reset();
                qh = qt.data();
                ktt = qt[(size_t) t];
            }
            // the group's lanes on the host, rows n apart (not the caller's ldy): masks, b, QA; x, traces, iterations
            std::vector<uint8_t> mask(held ? (size_t) (nk * m) : 0);
            std::vector<T> bh((size_t) (nk * n), T(0)), xt((size_t) (nk * n), T(0)), QA((size_t) nk);
            std::vector<double> tr(trace_out ? (size_t) (nk * cap) : 0);
            std::vector<int64_t> it((size_t) nk);
            std::vector<std::vector<T>> inv((size_t) nk);  // a lane's own 1/s, alive until the group's last synchronisation
            for (int64_t j = 0; j < nk; ++j) {
                const auto &L = plan.lanes[(size_t) g.ks[(size_t) j]];
                plan.stage(L, Y + g.ks[(size_t) j] * ldy, held ? mask.data() + j * m : nullptr, bh.data() + j * n);
                if (L.s != nullptr) inv[(size_t) j] = recip_weights(L.s, n);
                QA[(size_t) j] = lane_QA(ktt, L.cost, L.s != nullptr ? inv[(size_t) j].data() : (weighted() ? sinv_h.data() : nullptr), t);
            }
            if (batched) {
                // groups of up to W lanes, each lane's diagonal assembled here from its plan
                for (int64_t j0 = 0; j0 < nk; j0 += W) {
                    const int nvec = (int) std::min<int64_t>(W, nk - j0);
                    for (int c = 0; c < nvec; ++c) {
                        const int64_t j = j0 + c;
                        const auto &L = plan.lanes[(size_t) g.ks[(size_t) j]];
                        lane_diag dg{ T(1) / L.cost, QA[(size_t) j], sinv_dev(), nullptr };
                        if (L.s != nullptr) {
                            MI_HIP_CHECK(hipMemcpyAsync(lane_sinv(c), inv[(size_t) j].data(), sizeof(T) * (size_t) m, hipMemcpyHostToDevice, stream));
                            dg.sinv = lane_sinv(c);
                        }
                        if (L.hold != nullptr) {
                            MI_HIP_CHECK(hipMemcpyAsync(lane_hold(c), mask.data() + j * m, (size_t) m, hipMemcpyHostToDevice, stream));
                            dg.hold = lane_hold(c);
                        }
                        lanes.diag[(size_t) c] = dg;
                    }
                    solve_cg_group(bh.data() + j0 * n, nvec, n, imax, eps, xt.data() + j0 * n, trace_out ? tr.data() + j0 * cap : nullptr,
                                   it.data() + j0, held);
                }
            } else {
                // one after another through the single solve, the engine's cost, weights and hold rows set per lane
                for (int64_t j = 0; j < nk; ++j) {
                    const auto &L = plan.lanes[(size_t) g.ks[(size_t) j]];
                    moved.cost = moved.cost || costs != nullptr;
                    cost = L.cost;
                    if (L.s != nullptr) {
                        moved.sinv = true;
                        set_sinv(inv[(size_t) j]);
                    }
                    QA_cost = QA[(size_t) j];  // generate_q's at this lane's cost and weights, or its pivot's
                    if (L.hold != nullptr) {
                        moved.hold = true;
                        MI_HIP_CHECK(hipMemcpyAsync(hold_own.get(), mask.data() + j * m, (size_t) m, hipMemcpyHostToDevice, stream));
                        hold_cur = hold_own.get();
                    }
                    solve_cg(bh.data() + j * n, nullptr, imax, eps, xt.data() + j * n, trace_out ? tr.data() + j * cap : nullptr,
                             it.data() + j);
                    hold_cur = nullptr;
                }
            }
            // learn()'s end with t in the last point's part, in the caller's lane order
            for (int64_t j = 0; j < nk; ++j) {
                const int64_t k = g.ks[(size_t) j];
                T *a = alpha_out + k * ldy;
                std::copy(xt.begin() + j * n, xt.begin() + j * n + m, a);
                a[m] = T(0);
                learn_tail(Y + k * ldy, qh, QA[(size_t) j], m, t, a, bias_out ? bias_out + k : nullptr);
                if (iters) iters[k] = it[(size_t) j];
                if (trace_out) std::copy_n(tr.begin() + j * cap, std::min<int64_t>(cap, it[(size_t) j] + 1), trace_out + k * cap);
            }
        }
    };
    // The one restore rule: exactly what moved is undone, on every exit. A call that moved nothing (learn_multi without
    // weights) keeps the captured graph it finds and pays no synchronisation; the pool's diag is host state that every
    // batched entry point sets before it runs a group, here it goes back to the engine's own so that no later group
    // meets this call's hold rows.
    auto restore = [&]() {
        hold_cur = nullptr;
        cost = cost0;
        if (moved.sinv) set_sinv(sinv0);              // with the QA_cost that goes with them; resets the graph
        if (moved.q) generate_q(nullptr, nullptr);    // the last point's q and the QA_cost of the restored diagonal; resets the graph
        else if (moved.cost && !moved.sinv) QA_cost = ctr_kmm + diag_m();  // generate_q's (it ran before the cost moved)
        if (moved.cost || moved.hold) graph_reset();  // a captured block holds QA_cost and the hold rows
        if (lanes.width >= 2) lanes_own_diag();
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
            kp_raw_of(a);
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
        // an unfilled tile cache: the first vector fills it
        const int first = fill_tiles([&] {
            kp_raw(lane_v(LV_D, 0), nullptr);
            launch_train_values_fin<T>(raw.get(), q.get(), ALPHA[c0 * lda + m], (T) bias[c0], m, lane_v(LV_R, 0), stream);
        }) ? 1 : 0;
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

// every member defined in this file (need_lane_buf, a member template, is instantiated by its uses here)
#define INST(T)                                                                                                      \
    template void engine<T>::need_pool();                                                                            \
    template int64_t engine<T>::lane_bytes(bool, bool) const;                                                        \
    template int engine<T>::multi_lanes(bool, bool);                                                                 \
    template void engine<T>::lanes_own_diag();                                                                       \
    template void engine<T>::tiles_multi(int, int, int, bool);                                                       \
    template void engine<T>::kp_lanes(int, int, int, int, T, bool, bool, bool);                                      \
    template void engine<T>::cg_iter_multi(int, int);                                                                \
    template void engine<T>::solve_cg_group(const T *, int, int64_t, int64_t, T, T *, double *, int64_t *, bool);    \
    template bool engine<T>::held_supported() const;                                                                 \
    template bool engine<T>::multi_batched() const;                                                                  \
    template int engine<T>::multi_width_next(bool, bool) const;                                                      \
    template void engine<T>::solve_cg_multi(const T *, int64_t, int64_t, const T *, int64_t, T, T *, double *, int64_t *); \
    template void engine<T>::kp_multi(const T *, const T *, T *, int64_t, int64_t, T);                               \
    template void engine<T>::set_sinv(const std::vector<T> &);                                                       \
    template void engine<T>::set_point_weights(const T *);                                                           \
    template void engine<T>::learn_held(const T *, int64_t, int64_t, const double *, const T *, int64_t, const uint8_t *, \
                                        int64_t, int64_t, T, T *, double *, double *, int64_t *, int64_t *);         \
    template void engine<T>::train_values(const T *, int64_t, int64_t, const double *, T *, int64_t);                \
    template void engine<T>::time_kp_multi(int64_t, int, double *);
INST(float)
INST(double)
#undef INST

}  // namespace plssvm_mi
