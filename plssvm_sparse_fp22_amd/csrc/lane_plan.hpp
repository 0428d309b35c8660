// The host half of a multi-lane learn (engine::learn_held): argument checks, every lane's
// cost, weight row, hold row and pivot, the pivot groups, and per lane of a group its mask, right-hand side, QA and
// the end of learn(). Plain C++17 on host integers and scalars, no HIP: the engine includes it, and so does the
// stand-alone CPU check tests/lane_plan_check.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mi_error.hpp"

namespace plssvm_mi {

// point weights: finite and > 0 with a finite reciprocal > 0, else ERR_ARG
template <typename T>
void check_weights(const T *s, int64_t count) {
    for (int64_t i = 0; i < count; ++i) {
        const T r = T(1) / s[i];
        if (!(s[i] > T(0)) || !std::isfinite(s[i]) || !(r > T(0)) || !std::isfinite(r))
            throw mi_error(-1, "point weight " + std::to_string(i) + " is not a finite number > 0 (with a finite reciprocal)");
    }
}

// the n reciprocals of a weight row
template <typename T>
std::vector<T> recip_weights(const T *s, int64_t n) {
    std::vector<T> inv((size_t) n);
    for (int64_t i = 0; i < n; ++i) inv[(size_t) i] = T(1) / s[i];
    return inv;
}

// QA = k_tt + diag_t, diag_t = 1/C or, with the reciprocal weights sinv (null: none), (1/C)(1/s_t): both reciprocals
// and their product are rounded in T
template <typename T>
T lane_QA(T ktt, T cost, const T *sinv, int64_t t) {
    const T cinv = T(1) / cost;
    T dt = cinv;
    if (sinv != nullptr) dt = cinv * sinv[t];
    return ktt + dt;
}

// csvm::learn's end (csvm.cpp:257-258) with the pivot t in the last point's part (t = m: the reference's):
// alpha[t] = -sum alpha, bias = y_t + QA sum alpha - q . alpha over the first m entries (alpha is 0 on masked rows)
template <typename T>
void learn_tail(const T *y, const T *q, T QA, int64_t m, int64_t t, T *alpha, double *bias_out) {
    T s = 0, qa = 0;
    for (int64_t i = 0; i < m; ++i) s += alpha[i];
    for (int64_t i = 0; i < m; ++i) qa = std::fma(q[i], alpha[i], qa);
    const T bias = y[t] + QA * s - qa;  // (:257); QA = k_tt + (1/C)(1/s_t) with point weights
    alpha[t] = -s;                      // (:258)
    if (bias_out) *bias_out = (double) bias;
}

template <typename T>
struct lane_plan {
    struct lane {
        T cost;
        const T *s;           // the lane's own weight row; null: the call's shared row if any, else the context's
        const uint8_t *hold;  // the lane's hold row; null: none (a call without hold rows)
        int64_t t;            // the pivot: the largest index not held (m without hold rows)
    };
    struct group {
        int64_t t;
        std::vector<int64_t> ks;  // the lanes of pivot t, in the caller's order
    };
    int64_t n, m;
    const T *shared;            // the call's one weight row for all lanes (null: none)
    std::vector<lane> lanes;    // in the caller's order
    std::vector<group> groups;  // pivot m first, the others by first appearance

    // Checks every argument of every lane (ERR_ARG) before it returns anything. cost: the context's, for costs == null
    lane_plan(int64_t n_, T cost, const T *Y, int64_t nlane, int64_t ldy, const double *costs, const T *S, int64_t lds,
              const uint8_t *HOLD, int64_t ldh) : n(n_), m(n_ - 1), shared(S != nullptr && lds == 0 ? S : nullptr) {
        if (Y == nullptr) throw mi_error(-1, "No labels given for training! Maybe the data is only usable for prediction?");
        if (nlane < 1) throw mi_error(-1, "at least one class is needed");
        if (ldy < n) throw mi_error(-1, "the leading dimension is smaller than the number of points");
        if (S != nullptr && lds != 0 && lds < n) throw mi_error(-1, "the weights' leading dimension is smaller than the number of points");
        lanes.assign((size_t) nlane, lane{ cost, nullptr, nullptr, m });
        if (costs != nullptr)
            for (int64_t k = 0; k < nlane; ++k) {
                const T c = (T) costs[k], r = T(1) / c;
                if (!(costs[k] > 0) || !std::isfinite(c) || !(c > T(0)) || !std::isfinite(r) || !(r > T(0)))
                    throw mi_error(-1, "cost " + std::to_string(k) + " is not a finite number > 0");
                lanes[(size_t) k].cost = c;
            }
        if (S != nullptr)
            for (int64_t k = 0; k < (lds != 0 ? nlane : 1); ++k) {
                check_weights(S + k * lds, n);
                if (lds != 0) lanes[(size_t) k].s = S + k * lds;
            }
        if (HOLD != nullptr && ldh != 0 && ldh < n)
            throw mi_error(-1, "the hold rows' leading dimension is smaller than the number of points");
        for (int64_t k = 0; k < nlane; ++k) {
            lane &L = lanes[(size_t) k];
            if (HOLD != nullptr) {
                L.hold = HOLD + k * ldh;
                int64_t cnt = 0;
                L.t = -1;
                for (int64_t i = 0; i < n; ++i)
                    if (L.hold[i] == 0) L.t = i, ++cnt;
                if (cnt < 2) throw mi_error(-1, "lane " + std::to_string(k) + " has fewer than two training points");
            }
            auto g = std::find_if(groups.begin(), groups.end(), [&](const group &x) { return x.t == L.t; });
            if (g == groups.end()) g = groups.insert(groups.end(), group{ L.t, {} });
            g->ks.push_back(k);
        }
        std::stable_partition(groups.begin(), groups.end(), [&](const group &x) { return x.t == m; });
    }

    // Lane L of the pivot group t: its mask (the rows that are no part of its system: held, or from the pivot on; none
    // is written for a lane without a hold row) and its right-hand side b = y - y_t, 0 on masked rows; m entries each
    void stage(const lane &L, const T *y, uint8_t *mask, T *b) const {
        for (int64_t i = 0; i < m; ++i) {
            const bool off = (L.hold != nullptr && L.hold[i] != 0) || i >= L.t;
            if (L.hold != nullptr) mask[i] = off ? 1 : 0;
            b[i] = off ? T(0) : y[i] - y[L.t];
        }
    }
};

}  // namespace plssvm_mi
