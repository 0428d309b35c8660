// Stand-alone check of the 7-byte tile record format (csrc/kp_pack.hpp), built and run by tests/test_kp_pack_cpu.py.
// Exit status 0 and "ok" on success; the first failing check is printed and the status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "kp_pack.hpp"

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

uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}
double from_bits(uint64_t u) {
    double v;
    std::memcpy(&v, &u, sizeof(v));
    return v;
}

constexpr int TILE_VALUES = 128 * 128;

// the descriptor of a tile, as the store kernel forms it: the range of all 16 384 high dwords
uint32_t classify(const std::vector<double> &tile) {
    uint32_t mn = KP_PACK_MN0, mx = KP_PACK_MX0;
    for (double v : tile) kp_pack_track((uint32_t) (bits(v) >> 32), mn, mx);
    return kp_pack_desc(mn, mx);
}

// a tile of `fill` with one value replaced, at a position that moves with the case
uint32_t classify_with(double fill, double odd, int pos) {
    std::vector<double> t(TILE_VALUES, fill);
    t[(size_t) pos % TILE_VALUES] = odd;
    return classify(t);
}

// pack one value against base exponent E and unpack it again
uint64_t round_trip(uint64_t u, uint32_t E) {
    const uint32_t base = kp_pack_base(E);
    const uint32_t h24 = kp_pack_h24((uint32_t) (u >> 32), base);
    if (h24 >> 24) return ~uint64_t(0);  // does not fit 24 bits
    return kp_pack_join(kp_unpack_hi(h24, base), (uint32_t) u);
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double denorm = std::numeric_limits<double>::denorm_min();
    const double min_normal = std::numeric_limits<double>::min();

    // ---- classification ----
    CHECK(classify(std::vector<double>(TILE_VALUES, 1.0)) == 1023, "all ones must pack with E = 1023");
    CHECK(classify_with(1.0, std::ldexp(1.0, -16), 5) == KP_PACK_RAW, "16 binades down must be raw");
    CHECK(classify_with(1.0, std::ldexp(1.0, -15), 5) == 1023, "15 binades down must pack");
    CHECK(classify_with(1.9999, std::ldexp(1.0, -15), 16383) == 1023, "15 binades down (mantissas differ) must pack");
    CHECK(classify_with(1.0, std::ldexp(1.9999, -16), 0) == KP_PACK_RAW, "just under 15 binades down must be raw");
    CHECK(classify_with(1.0, 0.0, 77) == KP_PACK_RAW, "0.0 must be raw");
    CHECK(classify_with(1.0, -0.0, 78) == KP_PACK_RAW, "-0.0 must be raw");
    CHECK(classify_with(1.0, denorm, 79) == KP_PACK_RAW, "a denormal must be raw");
    CHECK(classify_with(std::ldexp(1.0, -1015), denorm, 80) == KP_PACK_RAW, "a denormal beside tiny values must be raw");
    // E - 15 < 1: E = 8 here, the smallest normal lies inside [E - 15, E] but the base would not be a normal exponent
    CHECK(classify_with(std::ldexp(1.0, -1015), min_normal, 81) == KP_PACK_RAW, "smallest normal with E - 15 < 1 must be raw");
    CHECK(classify(std::vector<double>(TILE_VALUES, min_normal)) == KP_PACK_RAW, "E = 1 must be raw");
    CHECK(classify(std::vector<double>(TILE_VALUES, std::ldexp(1.0, -1008))) == KP_PACK_RAW, "E = 15 must be raw");
    CHECK(classify_with(std::ldexp(1.0, -1007), min_normal, 82) == 16, "E = 16 with the smallest normal must pack");
    CHECK(classify_with(1.0, -1.0, 83) == KP_PACK_RAW, "a negative value must be raw");
    CHECK(classify_with(1.0, -std::ldexp(1.0, -3), 84) == KP_PACK_RAW, "a small negative value must be raw");
    CHECK(classify_with(1.0, inf, 85) == KP_PACK_RAW, "inf must be raw");
    CHECK(classify_with(1.0, -inf, 86) == KP_PACK_RAW, "-inf must be raw");
    CHECK(classify_with(1.0, nan, 87) == KP_PACK_RAW, "NaN must be raw");
    CHECK(classify_with(1.0, -nan, 88) == KP_PACK_RAW, "-NaN must be raw");
    CHECK(classify(std::vector<double>(TILE_VALUES, std::numeric_limits<double>::max())) == 2046, "E = 2046 must pack");
    CHECK(classify_with(1.0, 1.0000000000000004, 89) == 1023, "1 + 2 ulp must pack");

    // ---- round trip, bit-exact ----
    const uint64_t ones_mant = 0x000FFFFFFFFFFFFFull;
    struct {
        uint64_t u;
        uint32_t E;
    } fixed[] = {
        { bits(1.0), 1023 },
        { bits(1.0000000000000004), 1023 },
        { bits(1.0), 1038 },                                  // 1.0 at E - 15
        { (uint64_t(1023) << 52) | ones_mant, 1023 },         // mantissa all ones at E
        { (uint64_t(1008) << 52) | ones_mant, 1023 },         // mantissa all ones at E - 15
        { uint64_t(1008) << 52, 1023 },                       // mantissa all zeros at E - 15
        { uint64_t(1) << 52, 16 },                            // the smallest normal at E - 15, E = 16
        { (uint64_t(2046) << 52) | ones_mant, 2046 },         // the largest double
    };
    for (const auto &c : fixed) {
        const uint64_t back = round_trip(c.u, c.E);
        CHECK(back == c.u, "round trip of %016llx at E = %u gave %016llx", (unsigned long long) c.u, c.E,
              (unsigned long long) back);
        CHECK(from_bits(back) == from_bits(c.u), "round trip value");
    }
    std::mt19937_64 rng(20240611);
    int bad = 0;
    for (int i = 0; i < 100000; ++i) {
        const uint32_t E = 16 + (uint32_t) (rng() % (2046 - 16 + 1));
        const uint32_t e = E - (uint32_t) (rng() % 16);
        const uint64_t u = ((uint64_t) e << 52) | (rng() & ones_mant);
        if (round_trip(u, E) != u) ++bad;
    }
    CHECK(bad == 0, "%d of 100000 random values did not round-trip", bad);

    // ---- the kernels' grouping: 4 values -> 4 low dwords + 3 dwords of 24-bit words, every position ----
    bad = 0;
    for (int i = 0; i < 20000; ++i) {
        const uint32_t E = 16 + (uint32_t) (rng() % (2046 - 16 + 1));
        const uint32_t base = kp_pack_base(E);
        uint64_t v[4];
        uint32_t hi[4], lo[4], w[3];
        for (int k = 0; k < 4; ++k) {
            // the extremes in turn at every position: offset 0 / 15, mantissa zeros / ones
            uint32_t off = (uint32_t) (rng() % 16);
            uint64_t mant = rng() & ones_mant;
            if (i % 8 == k) off = 0, mant = 0;
            if (i % 8 == k + 4) off = 15, mant = ones_mant;
            v[k] = ((uint64_t) (E - 15 + off) << 52) | mant;
            hi[k] = (uint32_t) (v[k] >> 32);
            lo[k] = (uint32_t) v[k];
        }
        kp_pack4(hi, base, w);
        for (int k = 0; k < 4; ++k)
            if (kp_pack_join(kp_unpack4(k, w[0], w[1], w[2], base), lo[k]) != v[k]) ++bad;
    }
    CHECK(bad == 0, "%d grouped values did not round-trip", bad);

    // ---- the record layout: the 28 groups of a lane are a permutation, and rows complete in consumption order ----
    {
        int seen[KP_PACK_GROUPS] = {};
        for (int mt = 0; mt < 4; ++mt) {
            for (int r = 0; r < 4; ++r) ++seen[kp_pack_lo_group(mt, r)];
            for (int d = 0; d < 12; d += 4) ++seen[kp_pack_hi_group(mt, d)];
            for (int d = 0; d < 12; ++d) CHECK(kp_pack_hi_group(mt, d) == kp_pack_hi_group(mt, d & ~3), "hi group of a dword");
        }
        for (int g = 0; g < KP_PACK_GROUPS; ++g) CHECK(seen[g] == 1, "group %d used %d times", g, seen[g]);
        int last = -1;
        for (int mt = 0; mt < 4; ++mt)
            for (int r = 0; r < 4; ++r) {
                int need = kp_pack_lo_group(mt, r);
                for (int d = 3 * r; d < 3 * r + 3; ++d) need = need > kp_pack_hi_group(mt, d) ? need : kp_pack_hi_group(mt, d);
                CHECK(need > last, "row (%d, %d) completes at group %d, not after %d", mt, r, need, last);
                last = need;
            }
        CHECK(last == KP_PACK_GROUPS - 1, "the last row completes at group %d", last);
    }

    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
