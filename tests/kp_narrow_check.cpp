// Stand-alone check of the 53-bit tile record format (csrc/kp_narrow.hpp), built and run by tests/test_kp_narrow_cpu.py
// (a second time under the address and undefined-behaviour sanitizers).
// Exit status 0 and "ok" on success; every failing check is printed and the status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "kp_narrow.hpp"

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

constexpr int TILE_VALUES = 128 * 128;
constexpr uint64_t ONES_MANT = 0x000FFFFFFFFFFFFFull;
constexpr uint64_t ALT_MANT = 0x000AAAAAAAAAAAAAull;

// the descriptor of a tile, as the store kernel forms it: the range of all 16 384 high dwords
uint32_t classify(const std::vector<double> &tile) {
    uint32_t mn = KP_PACK_MN0, mx = KP_PACK_MX0;
    for (double v : tile) kp_pack_track((uint32_t) (bits(v) >> 32), mn, mx);
    const uint32_t d = kp_narrow_desc(mn, mx);
    // the three forms agree with kp_pack_desc: raw stays raw, the others carry its E
    const uint32_t wide = kp_pack_desc(mn, mx);
    CHECK((d == KP_PACK_RAW) == (wide == KP_PACK_RAW), "raw in one classification only");
    CHECK(d == KP_PACK_RAW || kp_desc_exp(d) == wide, "E of %x is not %u", d, wide);
    return d;
}

enum form { RAW, WIDE, NARROW };
form form_of(uint32_t d) { return d == KP_PACK_RAW ? RAW : (kp_desc_is_narrow(d) ? NARROW : WIDE); }

// a tile of `fill` with one value replaced, at every one of a set of positions that moves through the tile
bool all_positions(double fill, double odd, form want, uint32_t E) {
    static const int pos[] = { 0, 1, 63, 64, 127, 128, 255, 256, 4095, 8191, 8192, 12345, 16382, 16383 };
    for (int p : pos) {
        std::vector<double> t(TILE_VALUES, fill);
        t[(size_t) p] = odd;
        const uint32_t d = classify(t);
        if (form_of(d) != want) return false;
        if (want != RAW && kp_desc_exp(d) != E) return false;
    }
    return true;
}

// A lane's record of a whole tile record buffer (256 threads, record order), written the way the store kernel does it
// (kp_narrow_put into the stream, groups at kp_narrow_lo_group / kp_narrow_hi_group) and read back the way the load
// kernel does it, row by row. `touched` counts the reads of each of the lane's 106 dwords: [group][dword].
struct lane_io {
    std::vector<uint32_t> rec = std::vector<uint32_t>(KP_NARROW_BYTES / 4, 0xDEADBEEFu);
    int t = 0;
    int reads_lo[16] = {};
    int reads_hi[KP_NARROW_HDW] = {};
    int max_group_of_row[16] = {};

    uint32_t &lo(int k, int nt) { return rec.at((size_t) kp_narrow_group_dword(kp_narrow_lo_group(k), t) + (size_t) nt); }
    uint32_t &hi(int j) {  // dword j of the stream
        CHECK(j >= 0 && j < KP_NARROW_HDW, "stream dword %d", j);
        return rec.at((size_t) kp_narrow_group_dword(kp_narrow_hi_group(j >> 2), t) + (size_t) (j & 3));
    }

    void store(const uint64_t v[64], uint32_t base) {
        uint32_t w[KP_NARROW_HDW];
        for (int j = 0; j < KP_NARROW_HDW; ++j) w[j] = 0xFFFFFFFFu;  // garbage: put must not rely on a zero fill
        int stored = 0;
        for (int k = 0; k < 16; ++k) {
            for (int nt = 0; nt < 4; ++nt) {
                lo(k, nt) = (uint32_t) v[4 * k + nt];
                kp_narrow_put(4 * k + nt, kp_narrow_h21((uint32_t) (v[4 * k + nt] >> 32), base), w);
            }
            for (; stored < kp_narrow_hi_done(k); ++stored)  // a group leaves as soon as it is complete
                for (int e = 0; e < (stored == KP_NARROW_HGROUPS - 1 ? 2 : 4); ++e) hi(4 * stored + e) = w[4 * stored + e];
        }
        CHECK(stored == KP_NARROW_HGROUPS, "%d H groups stored", stored);
    }

    uint64_t load(int k, int nt, uint32_t base) {
        const int v = 4 * k + nt, j = kp_narrow_word(v);
        ++reads_hi[j];
        uint32_t w1 = 0x5A5A5A5Au;
        if (kp_narrow_straddles(v)) {
            ++reads_hi[j + 1];
            w1 = hi(j + 1);
        }
        const int g = kp_narrow_hi_group((kp_narrow_straddles(v) ? j + 1 : j) >> 2);
        if (g > max_group_of_row[k]) max_group_of_row[k] = g;
        if (kp_narrow_lo_group(k) > max_group_of_row[k]) max_group_of_row[k] = kp_narrow_lo_group(k);
        ++reads_lo[k];
        return kp_pack_join(kp_narrow_unpack(v, hi(j), w1, base), lo(k, nt));
    }
};

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double denorm = std::numeric_limits<double>::denorm_min();
    const double min_normal = std::numeric_limits<double>::min();
    const double below_one = 0.99999999999999989;  // the largest double below 1

    // ---- classification boundaries: one odd value at moving positions ----
    CHECK(all_positions(0.75, 0.5, NARROW, 1022), "one binade must be narrow");
    CHECK(all_positions(0.75, below_one, NARROW, 1022), "one binade (mantissa all ones) must be narrow");
    CHECK(all_positions(0.75, 0.25, NARROW, 1022), "exponents {E - 1, E} must be narrow");
    CHECK(all_positions(0.26, 0.99, NARROW, 1022), "exponents {E - 1, E}, the odd one on top, must be narrow");
    CHECK(all_positions(0.75, 0.2499999, WIDE, 1022), "exponents {E - 2, E} must take the 7-byte form");
    CHECK(all_positions(0.75, 0.125, WIDE, 1022), "exponents {E - 2, E} (a power of two) must take the 7-byte form");
    CHECK(all_positions(0.2, 0.75, WIDE, 1022), "exponents {E - 2, E}, the odd one on top, must take the 7-byte form");
    CHECK(all_positions(1.0, std::ldexp(1.0, -15), WIDE, 1023), "span 15 must take the 7-byte form");
    CHECK(all_positions(1.0, std::ldexp(1.0, -16), RAW, 0), "span 16 must be raw");
    CHECK(all_positions(0.75, 0.99, NARROW, 1022), "values in [0.5, 1) must be narrow");
    CHECK(all_positions(0.75, 1.0, NARROW, 1023), "an exact 1.0 among values in [0.5, 1) must be narrow");
    CHECK(all_positions(0.3, 1.0, WIDE, 1023), "an exact 1.0 among values in [0.25, 0.5) must take the 7-byte form");
    CHECK(all_positions(0.75, -0.75, RAW, 0), "a negative value must be raw");
    CHECK(all_positions(0.75, 0.0, RAW, 0), "a zero must be raw");
    CHECK(all_positions(0.75, -0.0, RAW, 0), "a negative zero must be raw");
    CHECK(all_positions(0.75, denorm, RAW, 0), "a denormal must be raw");
    CHECK(all_positions(0.75, inf, RAW, 0), "inf must be raw");
    CHECK(all_positions(0.75, -inf, RAW, 0), "-inf must be raw");
    CHECK(all_positions(0.75, nan, RAW, 0), "NaN must be raw");
    CHECK(all_positions(0.75, -nan, RAW, 0), "-NaN must be raw");
    // the edges of E
    CHECK(all_positions(std::ldexp(1.0, -1007), std::ldexp(1.5, -1007), NARROW, 16), "E = 16, one binade, must be narrow");
    CHECK(all_positions(std::ldexp(1.0, -1007), std::ldexp(1.5, -1008), NARROW, 16), "E = 16 with E - 1 must be narrow");
    CHECK(all_positions(std::ldexp(1.0, -1007), min_normal, WIDE, 16), "E = 16 with the smallest normal must take the 7-byte form");
    CHECK(all_positions(std::ldexp(1.0, -1008), std::ldexp(1.5, -1008), RAW, 0), "E = 15 must be raw, as in kp_pack.hpp");
    CHECK(all_positions(min_normal, denorm, RAW, 0), "a denormal beside the smallest normals must be raw");
    CHECK(all_positions(std::numeric_limits<double>::max(), std::ldexp(1.0, 1023), NARROW, 2046), "E = 2046 must be narrow");
    CHECK(all_positions(std::numeric_limits<double>::max(), std::ldexp(1.0, 1022), NARROW, 2046), "E = 2046 with 2045 must be narrow");
    CHECK(all_positions(std::ldexp(1.0, 1023), inf, RAW, 0), "inf beside E = 2046 must be raw");
    // descriptors: one uniform compare tells the forms apart, and the flag lies above bit 11
    CHECK(KP_NARROW_FLAG > 0x800u && (KP_NARROW_FLAG & 2047u) == 0, "the flag bit lies above bit 11");
    CHECK(!kp_desc_is_narrow(KP_PACK_RAW) && !kp_desc_is_narrow(2046u) && kp_desc_is_narrow(16u | KP_NARROW_FLAG), "the compare");
    CHECK(kp_narrow_base(16) == (15u << 20) && kp_narrow_base(1023) == (1022u << 20), "the base");

    // ---- positions: no shift of 32 or more, nothing past dword 41, fields tile the stream ----
    {
        int covered[KP_NARROW_HDW * 32] = {};
        for (int v = 0; v < 64; ++v) {
            const int j = kp_narrow_word(v), sh = kp_narrow_shift(v);
            CHECK(sh >= 0 && sh < 32, "shift %d of value %d", sh, v);
            CHECK(32 * j + sh == KP_NARROW_BITS * v, "value %d sits at bit %d", v, 32 * j + sh);
            CHECK(kp_narrow_straddles(v) == (sh + KP_NARROW_BITS > 32), "straddle of value %d", v);
            CHECK(!kp_narrow_straddles(v) || (sh >= 1 && 32 - sh >= 1 && 32 - sh < 32), "the carry shift of value %d", v);
            CHECK(j + (kp_narrow_straddles(v) ? 1 : 0) < KP_NARROW_HDW, "value %d reads dword %d", v, j + 1);
            for (int b = 0; b < KP_NARROW_BITS; ++b) ++covered[KP_NARROW_BITS * v + b];
        }
        for (int b = 0; b < KP_NARROW_HDW * 32; ++b) CHECK(covered[b] == 1, "bit %d covered %d times", b, covered[b]);
        CHECK(!kp_narrow_straddles(63) && kp_narrow_word(63) == 41, "the last value lies inside dword 41");
        CHECK(16 * 4 + KP_NARROW_HDW == KP_NARROW_DWORDS, "dwords per lane");
    }

    // ---- group bookkeeping: the record order, a permutation without holes, inside the 108 544 bytes ----
    {
        static const char *order[KP_NARROW_GROUPS] = { "L0", "H0", "L1", "H1", "L2", "L3", "H2", "L4", "H3", "L5", "L6", "H4", "L7", "H5",
                                                       "L8", "L9", "H6", "L10", "H7", "L11", "L12", "H8", "L13", "H9", "L14", "L15", "H10" };
        char name[8];
        int seen[KP_NARROW_GROUPS] = {};
        for (int k = 0; k < 16; ++k) {
            const int g = kp_narrow_lo_group(k);
            CHECK(g >= 0 && g < KP_NARROW_GROUPS - 1, "L%d at %d", k, g);
            std::snprintf(name, sizeof(name), "L%d", k);
            if (g >= 0 && g < KP_NARROW_GROUPS) {
                CHECK(std::strcmp(name, order[g]) == 0, "group %d is %s, not %s", g, order[g], name);
                ++seen[g];
            }
            CHECK(kp_narrow_hi_need(k) == ((84 * k + 83) / 32) / 4, "row %d needs H%d", k, kp_narrow_hi_need(k));
        }
        for (int h = 0; h < KP_NARROW_HGROUPS; ++h) {
            const int g = kp_narrow_hi_group(h);
            CHECK(g >= 0 && g < KP_NARROW_GROUPS, "H%d at %d", h, g);
            std::snprintf(name, sizeof(name), "H%d", h);
            if (g >= 0 && g < KP_NARROW_GROUPS) {
                CHECK(std::strcmp(name, order[g]) == 0, "group %d is %s, not %s", g, order[g], name);
                ++seen[g];
            }
            const int k0 = kp_narrow_hi_row(h);  // the first row that needs H_h
            CHECK(k0 >= 0 && k0 < 16 && kp_narrow_hi_need(k0) >= h && (k0 == 0 || kp_narrow_hi_need(k0 - 1) < h), "first row of H%d: %d", h, k0);
        }
        for (int g = 0; g < KP_NARROW_GROUPS; ++g) CHECK(seen[g] == 1, "group %d used %d times", g, seen[g]);
        CHECK(kp_narrow_hi_group(KP_NARROW_HGROUPS - 1) == KP_NARROW_GROUPS - 1, "H10 is the last, short group");
        // the 256 lanes' parts of the groups tile the record exactly
        std::vector<int> used(KP_NARROW_BYTES / 4, 0);
        for (int g = 0; g < KP_NARROW_GROUPS; ++g)
            for (int t = 0; t < 256; ++t)
                for (int e = 0; e < (g == KP_NARROW_GROUPS - 1 ? 2 : 4); ++e) {
                    const int at = kp_narrow_group_dword(g, t) + e;
                    CHECK(at >= 0 && at < KP_NARROW_BYTES / 4, "group %d thread %d at dword %d", g, t, at);
                    if (at >= 0 && at < KP_NARROW_BYTES / 4) ++used[(size_t) at];
                }
        int holes = 0;
        for (int u : used) holes += u != 1;
        CHECK(holes == 0, "%d dwords of the record not used exactly once", holes);
        CHECK(KP_NARROW_BYTES == 108544 && KP_NARROW_BYTES <= 128 * 128 * 8, "record bytes");
        // a group is stored once complete, never before a row that still writes into it, and all by the last row
        int done = 0;
        for (int k = 0; k < 16; ++k) {
            const int now = kp_narrow_hi_done(k);
            CHECK(now >= done && now <= KP_NARROW_HGROUPS, "H groups done after row %d: %d", k, now);
            for (int h = 0; h < now; ++h) {
                const int last_dword = h == KP_NARROW_HGROUPS - 1 ? 41 : 4 * h + 3;
                CHECK(32 * (last_dword + 1) <= 84 * (k + 1), "H%d stored after row %d is not complete", h, k);
            }
            done = now;
        }
        CHECK(done == KP_NARROW_HGROUPS, "H groups done after the last row: %d", done);
    }

    // ---- round trip of whole lane records, through the record order ----
    std::mt19937_64 rng(20240917);
    int bad = 0, cases = 0;
    const uint64_t mants[] = { 0, ONES_MANT, ALT_MANT, ALT_MANT >> 1 };
    const uint32_t Es[] = { 16, 17, 1022, 1023, 2046 };
    for (uint32_t E : Es) {
        const uint32_t base = kp_narrow_base(E);
        for (int lane_t : { 0, 1, 63, 64, 255 }) {
            // each position x each exponent x each mantissa pattern (3 = random), neighbours at all ones / all zeros / random
            for (int pos = 0; pos < 64; ++pos)
                for (int eo = 0; eo < 2; ++eo)
                    for (int mp = 0; mp < 5; ++mp)
                        for (int nb = 0; nb < 3; ++nb) {
                            if (lane_t != 0 && lane_t != 255 && (mp + nb + pos) % 3) continue;  // a thinner sweep for the middle lanes
                            uint64_t v[64];
                            for (int i = 0; i < 64; ++i) {
                                if (nb == 0) v[i] = ((uint64_t) E << 52) | ONES_MANT;         // field all ones, low dword all ones
                                else if (nb == 1) v[i] = (uint64_t) (E - 1) << 52;            // field all zeros
                                else v[i] = ((uint64_t) (E - (rng() & 1)) << 52) | (rng() & ONES_MANT);
                            }
                            v[pos] = ((uint64_t) (E - 1 + (uint32_t) eo) << 52) | (mp < 4 ? mants[mp] : (rng() & ONES_MANT));
                            lane_io io;
                            io.t = lane_t;
                            io.store(v, base);
                            for (int k = 0; k < 16; ++k)
                                for (int nt = 0; nt < 4; ++nt) {
                                    const int i = 4 * k + nt, j = kp_narrow_word(i);
                                    const uint32_t w1 = kp_narrow_straddles(i) ? io.hi(j + 1) : 0xA5A5A5A5u;
                                    const uint64_t back = kp_pack_join(kp_narrow_unpack(i, io.hi(j), w1, base), io.lo(k, nt));
                                    if (back != v[i]) {
                                        if (bad < 5)
                                            std::printf("FAIL value %d (pos %d, E %u, eo %d, mp %d, nb %d): %016llx -> %016llx\n", i, pos, E, eo,
                                                        mp, nb, (unsigned long long) v[i], (unsigned long long) back);
                                        ++bad;
                                    }
                                }
                            ++cases;
                        }
        }
    }
    CHECK(bad == 0, "%d values of %d lane records did not round-trip", bad, cases);
    CHECK(cases > 10000, "only %d lane records", cases);

    // ---- what a row reads: L_k and the H groups up to (84 k + 83) / 32 / 4, each stream dword the right number of times ----
    {
        uint64_t v[64];
        for (int i = 0; i < 64; ++i) v[i] = ((uint64_t) (1022 - (rng() & 1)) << 52) | (rng() & ONES_MANT);
        lane_io io;
        io.t = 200;
        io.store(v, kp_narrow_base(1022));
        int last = -1;
        for (int k = 0; k < 16; ++k) {
            for (int nt = 0; nt < 4; ++nt) {
                const uint64_t got = io.load(k, nt, kp_narrow_base(1022));
                CHECK(got == v[4 * k + nt], "value %d read row by row", 4 * k + nt);
            }
            CHECK(io.reads_lo[k] == 4, "row %d read %d low dwords", k, io.reads_lo[k]);
            const int want = kp_narrow_lo_group(k) > kp_narrow_hi_group(kp_narrow_hi_need(k)) ? kp_narrow_lo_group(k) : kp_narrow_hi_group(kp_narrow_hi_need(k));
            CHECK(io.max_group_of_row[k] == want, "row %d reads up to group %d, not %d", k, io.max_group_of_row[k], want);
            CHECK(io.max_group_of_row[k] > last, "row %d completes at group %d, not after %d", k, io.max_group_of_row[k], last);
            last = io.max_group_of_row[k];
        }
        CHECK(last == KP_NARROW_GROUPS - 1, "the last row completes at group %d", last);
        for (int j = 0; j < KP_NARROW_HDW; ++j) CHECK(io.reads_hi[j] >= 1 && io.reads_hi[j] <= 3, "stream dword %d read %d times", j, io.reads_hi[j]);
    }

    if (failures) return 1;
    std::printf("%d lane records\nok\n", cases);
    return 0;
}
