// Stand-alone check of the host half of a multi-lane learn (csrc/lane_plan.hpp), built and run by
// tests/test_lane_plan_cpu.py (a second time under the address and undefined-behaviour sanitizers). n = 9 points
// (m = 8), in float and double; every comparison is ==. Exit status 0 and "ok" on success; every failing check is
// printed and the status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "lane_plan.hpp"

using namespace plssvm_mi;

namespace {

int failures = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);      \
            std::printf("\n");             \
            ++failures;                    \
        }                                  \
    } while (0)

constexpr int64_t N = 9, M = 8, LD = 11;  // rows LD > N apart: a stride taken for n shows

template <typename T>
const char *name() { return sizeof(T) == 8 ? "double" : "float"; }

// labels of lane k: +-1, no two lanes alike, both signs in every lane
template <typename T>
std::vector<T> labels(int64_t nlane) {
    std::vector<T> Y((size_t) (nlane * LD), T(99));
    for (int64_t k = 0; k < nlane; ++k)
        for (int64_t i = 0; i < N; ++i) Y[(size_t) (k * LD + i)] = ((i * (k + 2) + k) % 3 == 0) ? T(1) : T(-1);
    return Y;
}

template <typename T>
std::vector<T> weights(int64_t rows) {
    std::vector<T> S((size_t) (rows * LD), T(1));
    for (int64_t k = 0; k < rows; ++k)
        for (int64_t i = 0; i < N; ++i) S[(size_t) (k * LD + i)] = T(0.3) + T(0.7) * T(i + 1) / T(k + 3);  // inexact reciprocals
    return S;
}

// the five hold rows of the issue: {last point}, {last three}, {i mod 3 == 0}, {none}, {last point}
std::vector<uint8_t> hold_rows() {
    std::vector<uint8_t> H((size_t) (5 * LD), 7);  // 7 between the rows: must not be read
    for (int64_t i = 0; i < N; ++i) {
        H[(size_t) (0 * LD + i)] = i == N - 1;
        H[(size_t) (1 * LD + i)] = i >= N - 3 ? 200 : 0;  // any non-zero value holds
        H[(size_t) (2 * LD + i)] = i % 3 == 0;
        H[(size_t) (3 * LD + i)] = 0;
        H[(size_t) (4 * LD + i)] = i == N - 1;
    }
    return H;
}

template <typename T>
void expect_error(const char *what, const std::string &text, const T *Y, int64_t nlane, int64_t ldy, const double *costs,
                  const T *S, int64_t lds, const uint8_t *HOLD, int64_t ldh) {
    try {
        lane_plan<T> plan(N, T(4), Y, nlane, ldy, costs, S, lds, HOLD, ldh);
        CHECK(false, "%s %s: no error", name<T>(), what);
    } catch (const mi_error &e) {
        CHECK(e.code == -1, "%s %s: code %d", name<T>(), what, e.code);
        CHECK(text == e.what(), "%s %s: text '%s'", name<T>(), what, e.what());
    }
}

template <typename T>
void no_hold_rows() {
    const std::vector<T> Y = labels<T>(3), S = weights<T>(3);
    const double costs[3] = { 0.5, 4.0, 30.0 };
    const T ktt = T(1) / T(3);  // some k_mm
    const lane_plan<T> own(N, T(7), Y.data(), 3, LD, costs, S.data(), LD, nullptr, 0);
    CHECK(own.n == N && own.m == M && own.shared == nullptr, "%s: n, m, shared", name<T>());
    CHECK(own.groups.size() == 1 && own.groups[0].t == M && own.groups[0].ks == (std::vector<int64_t>{ 0, 1, 2 }),
          "%s: one group of pivot m in caller order", name<T>());
    for (int64_t k = 0; k < 3; ++k) {
        const auto &L = own.lanes[(size_t) k];
        CHECK(L.t == M && L.hold == nullptr && L.cost == (T) costs[k] && L.s == S.data() + k * LD, "%s: lane %d", name<T>(), (int) k);
        std::vector<T> b((size_t) M, T(5));
        own.stage(L, Y.data() + k * LD, nullptr, b.data());  // no mask is written: a null pointer must do
        for (int64_t i = 0; i < M; ++i) CHECK(b[(size_t) i] == Y[(size_t) (k * LD + i)] - Y[(size_t) (k * LD + M)], "%s: b", name<T>());
        // QA, restated from learn_lanes as it was — the lane's own weight row:
        const std::vector<T> inv = recip_weights(L.s, N);
        {
            const T cinv = T(1) / L.cost;
            T dm = cinv;
            dm = cinv * inv[(size_t) M];
            CHECK(lane_QA(ktt, L.cost, inv.data(), M) == ktt + dm, "%s: QA, own row", name<T>());
        }
        for (int64_t i = 0; i < N; ++i) CHECK(inv[(size_t) i] == T(1) / L.s[i], "%s: reciprocals", name<T>());
    }
    // one row for all lanes, or the context's: the engine's sinv_h holds its reciprocals
    const lane_plan<T> shared(N, T(7), Y.data(), 3, LD, costs, S.data() + LD, 0, nullptr, 0);
    CHECK(shared.shared == S.data() + LD, "%s: the shared row", name<T>());
    const std::vector<T> sinv_h = recip_weights(shared.shared, N);
    for (const auto &L : shared.lanes) {
        CHECK(L.s == nullptr && L.t == M, "%s: a shared row is no lane's own", name<T>());
        const T cinv = T(1) / L.cost;
        T dm = cinv;
        dm = cinv * sinv_h[(size_t) M];
        CHECK(lane_QA(ktt, L.cost, sinv_h.data(), M) == ktt + dm, "%s: QA, shared or context row", name<T>());
    }
    // no weights, no costs: the context's cost
    const lane_plan<T> plain(N, T(7), Y.data(), 3, LD, nullptr, nullptr, 0, nullptr, 0);
    for (const auto &L : plain.lanes) {
        CHECK(L.cost == T(7) && L.s == nullptr && plain.shared == nullptr, "%s: the context's cost", name<T>());
        const T cinv = T(1) / L.cost;
        CHECK(lane_QA(ktt, L.cost, (const T *) nullptr, M) == ktt + cinv, "%s: QA, no weights", name<T>());
    }
}

template <typename T>
void check_held(const lane_plan<T> &plan, const std::vector<T> &Y, const std::vector<int64_t> &row_of_lane,
                const std::vector<uint8_t> &H) {
    for (size_t k = 0; k < plan.lanes.size(); ++k) {
        const auto &L = plan.lanes[k];
        const uint8_t *h = H.data() + row_of_lane[k] * LD;
        CHECK(L.hold == h, "%s: lane %d's hold row", name<T>(), (int) k);
        std::vector<uint8_t> mask((size_t) M, 9);
        std::vector<T> b((size_t) M, T(5));
        const T *y = Y.data() + (int64_t) k * LD;
        plan.stage(L, y, mask.data(), b.data());
        for (int64_t i = 0; i < M; ++i) {
            const bool off = h[i] != 0 || i >= L.t;
            CHECK(mask[(size_t) i] == (off ? 1 : 0), "%s: lane %d mask %d", name<T>(), (int) k, (int) i);
            CHECK(off ? (b[(size_t) i] == T(0) && !std::signbit(b[(size_t) i])) : b[(size_t) i] == y[i] - y[L.t], "%s: lane %d b %d",
                  name<T>(), (int) k, (int) i);
        }
    }
}

template <typename T>
void hold_rows_and_groups() {
    const std::vector<T> Y = labels<T>(5);
    const std::vector<uint8_t> H = hold_rows();
    const lane_plan<T> plan(N, T(4), Y.data(), 5, LD, nullptr, nullptr, 0, H.data(), LD);
    const int64_t piv[5] = { 7, 5, 8, 8, 7 };
    for (int k = 0; k < 5; ++k) CHECK(plan.lanes[(size_t) k].t == piv[k], "%s: pivot of lane %d is %d", name<T>(), k, (int) plan.lanes[(size_t) k].t);
    CHECK(plan.groups.size() == 3, "%s: %d groups", name<T>(), (int) plan.groups.size());
    if (plan.groups.size() == 3) {
        CHECK(plan.groups[0].t == 8 && plan.groups[0].ks == (std::vector<int64_t>{ 2, 3 }), "%s: group 0", name<T>());
        CHECK(plan.groups[1].t == 7 && plan.groups[1].ks == (std::vector<int64_t>{ 0, 4 }), "%s: group 1", name<T>());
        CHECK(plan.groups[2].t == 5 && plan.groups[2].ks == (std::vector<int64_t>{ 1 }), "%s: group 2", name<T>());
    }
    check_held(plan, Y, { 0, 1, 2, 3, 4 }, H);
    // the same five lanes reversed (the rows a negative stride apart cannot be passed: a reversed copy). Lane k is the
    // old lane 4 - k: pivots 7, 8, 8, 5, 7; pivot m first, then 7 (seen first), then 5; caller order inside a group
    std::vector<uint8_t> R((size_t) (5 * LD), 7);
    for (int64_t k = 0; k < 5; ++k)
        for (int64_t i = 0; i < N; ++i) R[(size_t) (k * LD + i)] = H[(size_t) ((4 - k) * LD + i)];
    const lane_plan<T> rev(N, T(4), Y.data(), 5, LD, nullptr, nullptr, 0, R.data(), LD);
    for (int k = 0; k < 5; ++k) CHECK(rev.lanes[(size_t) k].t == piv[4 - k], "%s: reversed pivot %d", name<T>(), k);
    CHECK(rev.groups.size() == 3 && rev.groups[0].t == 8 && rev.groups[0].ks == (std::vector<int64_t>{ 1, 2 }) &&
              rev.groups[1].t == 7 && rev.groups[1].ks == (std::vector<int64_t>{ 0, 4 }) && rev.groups[2].t == 5 &&
              rev.groups[2].ks == (std::vector<int64_t>{ 3 }),
          "%s: the reversed lanes' groups", name<T>());
    check_held(rev, Y, { 0, 1, 2, 3, 4 }, R);
    // ldh == 0: one hold row serves all lanes
    const lane_plan<T> one(N, T(4), Y.data(), 3, LD, nullptr, nullptr, 0, H.data() + LD, 0);
    CHECK(one.groups.size() == 1 && one.groups[0].t == 5 && one.groups[0].ks == (std::vector<int64_t>{ 0, 1, 2 }), "%s: ldh = 0 groups", name<T>());
    check_held(one, Y, { 1, 1, 1 }, H);
}

// learn_tail as it stood in the engine before the pivot became a parameter (m = M), copied
template <typename T>
void old_learn_tail(const T *y, const T *q_host, T QA, T *alpha, double *bias_out) {
    const int64_t m = M;
    T s = 0, qa = 0;
    for (int64_t i = 0; i < m; ++i) s += alpha[i];
    for (int64_t i = 0; i < m; ++i) qa = std::fma(q_host[i], alpha[i], qa);
    const T bias = y[m] + QA * s - qa;
    alpha[m] = -s;
    if (bias_out) *bias_out = (double) bias;
}

template <typename T>
void tails() {
    // sums that are inexact in T and depend on the order
    const T a0[N] = { T(1), T(1e-8), T(-1), T(3e-9), T(0.1), T(-7e-9), T(0.2), T(1e-8), T(0) };
    T q[M], y[N];
    for (int64_t i = 0; i < M; ++i) q[i] = T(1) / T(i + 3);
    for (int64_t i = 0; i < N; ++i) y[i] = i % 2 ? T(1) : T(-1);
    const T QA = T(1) + T(1) / T(7);
    T a[N], b[N];
    for (int64_t i = 0; i < N; ++i) a[i] = b[i] = a0[i];
    double bias_a = 0, bias_b = 0;
    learn_tail(y, q, QA, M, M, a, &bias_a);
    old_learn_tail(y, q, QA, b, &bias_b);
    CHECK(bias_a == bias_b, "%s: the tail's bias at t = m: %a, was %a", name<T>(), bias_a, bias_b);
    for (int64_t i = 0; i < N; ++i) CHECK(a[i] == b[i], "%s: the tail's alpha %d at t = m", name<T>(), (int) i);
    T plain = 0;
    for (int64_t i = 0; i < M; ++i) plain += a0[i];
    CHECK(a[M] == -plain && a[M] != T(0), "%s: alpha_m = -sum", name<T>());
    // t = 5: rows from 5 on are masked (alpha 0 there), learn_held's inline formula
    T c[N];
    for (int64_t i = 0; i < N; ++i) c[i] = i < 5 ? a0[i] : T(0);
    T s = 0, qa = 0;
    for (int64_t i = 0; i < M; ++i) s += c[i];
    for (int64_t i = 0; i < M; ++i) qa = std::fma(q[i], c[i], qa);
    const T want = y[5] + QA * s - qa;
    double bias_c = 0;
    learn_tail(y, q, QA, M, 5, c, &bias_c);
    CHECK(c[5] == -s && bias_c == (double) want, "%s: the tail at t = 5", name<T>());
    for (int64_t i = 6; i < N; ++i) CHECK(c[i] == T(0), "%s: the tail at t = 5 wrote row %d", name<T>(), (int) i);
    learn_tail(y, q, QA, M, 5, c, nullptr);  // a null bias pointer is allowed
}

template <typename T>
void errors() {
    const std::vector<T> Y = labels<T>(3);
    const std::vector<uint8_t> H = hold_rows();
    const std::string cost2 = "cost 2 is not a finite number > 0";
    auto weight = [](int i) { return "point weight " + std::to_string(i) + " is not a finite number > 0 (with a finite reciprocal)"; };
    expect_error<T>("no labels", "No labels given for training! Maybe the data is only usable for prediction?", nullptr, 3, LD, nullptr, nullptr, 0, nullptr, 0);
    expect_error<T>("nlane = 0", "at least one class is needed", Y.data(), 0, LD, nullptr, nullptr, 0, nullptr, 0);
    expect_error<T>("ldy < n", "the leading dimension is smaller than the number of points", Y.data(), 3, N - 1, nullptr, nullptr, 0, nullptr, 0);
    std::vector<T> S = weights<T>(3);
    expect_error<T>("lds < n", "the weights' leading dimension is smaller than the number of points", Y.data(), 3, LD, nullptr, S.data(), N - 1, nullptr, 0);
    expect_error<T>("ldh < n", "the hold rows' leading dimension is smaller than the number of points", Y.data(), 3, LD, nullptr, nullptr, 0, H.data(), N - 1);
    // the bad value is the last lane's: every lane is checked before anything is returned. No finite T has a reciprocal
    // that rounds to 0, so the underflow cases are a cost that is 0 once in T (float) and one whose reciprocal is not finite
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tiny = sizeof(T) == 4 ? 1e-39 : 1e-310;
    for (const double bad : { 0.0, -1.0, inf, nan, tiny, sizeof(T) == 4 ? 1e-46 : 0.0, sizeof(T) == 4 ? 1e39 : inf }) {
        const double costs[3] = { 0.5, 4.0, bad };
        expect_error<T>("a bad cost", cost2, Y.data(), 3, LD, costs, nullptr, 0, nullptr, 0);
    }
    for (const T bad : { T(0), T(-2), (T) nan, (T) inf, (T) tiny }) {
        S = weights<T>(3);
        S[(size_t) (2 * LD + 6)] = bad;
        expect_error<T>("a bad weight", weight(6), Y.data(), 3, LD, nullptr, S.data(), LD, nullptr, 0);
    }
    S = weights<T>(3);
    S[(size_t) (N - 1)] = T(0);
    expect_error<T>("a bad shared weight", weight((int) N - 1), Y.data(), 3, LD, nullptr, S.data(), 0, nullptr, 0);
    // the last lane has one training point, then none; two are enough
    std::vector<uint8_t> one = H;
    for (int64_t i = 0; i < N; ++i) one[(size_t) (2 * LD + i)] = i != 4;
    expect_error<T>("one training point", "lane 2 has fewer than two training points", Y.data(), 3, LD, nullptr, nullptr, 0, one.data(), LD);
    one[(size_t) (2 * LD + 4)] = 1;
    expect_error<T>("no training point", "lane 2 has fewer than two training points", Y.data(), 3, LD, nullptr, nullptr, 0, one.data(), LD);
    one[(size_t) (2 * LD + 1)] = one[(size_t) (2 * LD + 4)] = 0;
    const lane_plan<T> two(N, T(4), Y.data(), 3, LD, nullptr, nullptr, 0, one.data(), LD);
    CHECK(two.lanes[2].t == 4, "%s: two training points", name<T>());
    // the weights are checked before the hold rows, the costs before the weights (the order of the engine's checks)
    S = weights<T>(3);
    S[(size_t) (2 * LD)] = T(0);
    const double costs[3] = { 0.5, 4.0, 0.0 };
    expect_error<T>("cost before weight", cost2, Y.data(), 3, LD, costs, S.data(), LD, one.data(), N - 1);
    expect_error<T>("weight before ldh", weight(0), Y.data(), 3, LD, nullptr, S.data(), LD, one.data(), N - 1);
}

template <typename T>
void all() {
    no_hold_rows<T>();
    hold_rows_and_groups<T>();
    tails<T>();
    errors<T>();
}

}  // namespace

int main() {
    all<float>();
    all<double>();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
