// Stand-alone check of the packed tile record formats (csrc/kp_record.hpp: 24-bit "wide" and 21-bit "narrow" fields),
// built and run by tests/test_kp_record_cpu.py (a second time under the address and undefined-behaviour sanitizers).
// Exit status 0 and "ok" on success; every failing check is printed and the status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "kp_record.hpp"

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
uint64_t join(uint32_t hi, uint32_t lo) { return ((uint64_t) hi << 32) | lo; }

constexpr int TILE_VALUES = 128 * 128;
constexpr uint64_t ONES_MANT = 0x000FFFFFFFFFFFFFull;
constexpr uint64_t ALT_MANT = 0x000AAAAAAAAAAAAAull;

enum form { RAW, WIDE, NARROW };

// The descriptor of a tile at pack level 2, as the store kernel forms it: the range of all 16 384 high dwords. The
// lower levels agree with it: level 1 stores a narrow tile wide and keeps the others, level 0 stores every tile raw.
uint32_t classify(const std::vector<double> &tile) {
    uint32_t mn = KP_PACK_MN0, mx = KP_PACK_MX0;
    for (double v : tile) kp_pack_track((uint32_t) (bits(v) >> 32), mn, mx);
    const uint32_t d = kp_desc(mn, mx, 2);
    CHECK(kp_desc(mn, mx, 1) == kp_desc_exp(d), "level 1 of %x is %x", d, kp_desc(mn, mx, 1));
    CHECK(kp_desc(mn, mx, 0) == KP_DESC_RAW, "level 0 of %x is not raw", d);
    return d;
}
form form_of(uint32_t d) { return d == KP_DESC_RAW ? RAW : (kp_desc_is_narrow(d) ? NARROW : WIDE); }

// a tile of `fill` with one value replaced, at every one of a set of positions that moves through the tile
bool all_positions(double fill, double odd, form want, uint32_t E) {
    static const int pos[] = { 0, 1, 63, 64, 127, 128, 255, 256, 4095, 8191, 8192, 12345, 16382, 16383 };
    for (int p : pos) {
        std::vector<double> t(TILE_VALUES, fill);
        t[(size_t) p] = odd;
        const uint32_t d = classify(t);
        if (form_of(d) != want || kp_desc_exp(d) != E) return false;  // raw: E = 0
    }
    return true;
}

// the two layouts as they are stored today, restated: a refactor of the header must not move a byte
std::vector<std::string> order_of(int bits) {
    if (bits == KP_BITS_NARROW)
        return { "L0", "H0", "L1", "H1", "L2", "L3", "H2", "L4", "H3", "L5", "L6", "H4", "L7", "H5",
                 "L8", "L9", "H6", "L10", "H7", "L11", "L12", "H8", "L13", "H9", "L14", "L15", "H10" };
    std::vector<std::string> o(28);
    for (int mt = 0; mt < 4; ++mt) {
        for (int r = 0; r < 4; ++r) o[(size_t) (7 * mt + 2 * r)] = "L" + std::to_string(4 * mt + r);
        for (int d = 0; d < 12; d += 4) o[(size_t) (7 * mt + 1 + 2 * (d >> 2))] = "H" + std::to_string(3 * mt + (d >> 2));
    }
    return o;
}

// A lane's part of a whole tile record buffer (256 threads, record order), written the way the store kernel does it
// (put into the stream, groups at lo_group / hi_group as soon as hi_done says so) and read back the way the load
// kernel does it, row by row, counting the reads.
template <int BITS>
struct lane_io {
    using R = kp_record<BITS>;
    std::vector<uint32_t> rec = std::vector<uint32_t>(R::BYTES / 4, 0xDEADBEEFu);
    int t = 0;
    int reads_lo[16] = {};
    int reads_hi[R::HDW] = {};
    int max_group_of_row[16] = {};

    uint32_t &lo(int k, int nt) { return rec.at((size_t) R::group_dword(R::lo_group(k), t) + (size_t) nt); }
    uint32_t &hi(int j) {  // dword j of the stream
        CHECK(j >= 0 && j < R::HDW, "stream dword %d", j);
        return rec.at((size_t) R::group_dword(R::hi_group(j >> 2), t) + (size_t) (j & 3));
    }

    void store(const uint64_t v[64], uint32_t base) {
        uint32_t w[R::HDW];
        for (int j = 0; j < R::HDW; ++j) w[j] = 0xFFFFFFFFu;  // garbage: put must not rely on a zero fill
        int stored = 0;
        for (int k = 0; k < 16; ++k) {
            for (int nt = 0; nt < 4; ++nt) {
                lo(k, nt) = (uint32_t) v[4 * k + nt];
                R::put(4 * k + nt, (uint32_t) (v[4 * k + nt] >> 32) - base, w);
            }
            if (BITS == 24) {  // the 7-byte form's packing of a row's four fields into three dwords, written out
                const uint32_t h0 = (uint32_t) (v[4 * k] >> 32) - base, h1 = (uint32_t) (v[4 * k + 1] >> 32) - base,
                               h2 = (uint32_t) (v[4 * k + 2] >> 32) - base, h3 = (uint32_t) (v[4 * k + 3] >> 32) - base;
                CHECK(w[3 * k] == (h0 | (h1 << 24)) && w[3 * k + 1] == ((h1 >> 8) | (h2 << 16)) && w[3 * k + 2] == ((h2 >> 16) | (h3 << 8)),
                      "row %d is not packed as w0 = h0 | h1 << 24, w1 = h1 >> 8 | h2 << 16, w2 = h2 >> 16 | h3 << 8", k);
            }
            for (; stored < R::hi_done(k); ++stored)  // a group leaves as soon as it is complete
                for (int e = 0; e < (stored == R::HGROUPS - 1 ? R::TAIL : 4); ++e) hi(4 * stored + e) = w[4 * stored + e];
        }
        CHECK(stored == R::HGROUPS, "%d H groups stored", stored);
    }

    uint64_t load(int k, int nt, uint32_t base) {
        const int v = 4 * k + nt, j = R::word(v);
        ++reads_hi[j];
        uint32_t w1 = 0x5A5A5A5Au;
        if (R::straddles(v)) {
            ++reads_hi[j + 1];
            w1 = hi(j + 1);
        }
        const int g = R::hi_group((R::straddles(v) ? j + 1 : j) >> 2);
        if (g > max_group_of_row[k]) max_group_of_row[k] = g;
        if (R::lo_group(k) > max_group_of_row[k]) max_group_of_row[k] = R::lo_group(k);
        ++reads_lo[k];
        return join(R::unpack(v, hi(j), w1, base), lo(k, nt));
    }
};

// every check of one field width; returns the lane records it sent through the record order
template <int BITS>
int check_width(std::mt19937_64 &rng) {
    using R = kp_record<BITS>;
    constexpr uint32_t SPAN = (1u << (BITS - 20)) - 1u;  // binades below E that the field's exponent offset reaches
    CHECK(R::base(16) == ((16u - SPAN) << 20) && R::base(1023) == ((1023u - SPAN) << 20), "the base");
    CHECK(R::HDW == 2 * BITS && R::GROUPS == 16 + R::HGROUPS && R::BYTES <= 128 * 128 * 8, "sizes");

    // ---- positions: no shift of 32 or more, nothing past the last dword, fields tile the stream ----
    {
        int covered[R::HDW * 32] = {};
        for (int v = 0; v < 64; ++v) {
            const int j = R::word(v), sh = R::shift(v);
            CHECK(sh >= 0 && sh < 32, "shift %d of value %d", sh, v);
            CHECK(32 * j + sh == BITS * v, "value %d sits at bit %d", v, 32 * j + sh);
            CHECK(R::straddles(v) == (sh + BITS > 32), "straddle of value %d", v);
            CHECK(!R::straddles(v) || (sh >= 1 && 32 - sh >= 1 && 32 - sh < 32), "the carry shift of value %d", v);
            CHECK(j + (R::straddles(v) ? 1 : 0) < R::HDW, "value %d reads dword %d", v, j + 1);
            for (int b = 0; b < BITS; ++b) ++covered[BITS * v + b];
        }
        for (int b = 0; b < R::HDW * 32; ++b) CHECK(covered[b] == 1, "bit %d covered %d times", b, covered[b]);
        CHECK(!R::straddles(63) && R::word(63) == R::HDW - 1, "the last value lies inside the last dword");
    }

    // ---- group bookkeeping: the record order, a permutation without holes, inside the record's bytes ----
    {
        const std::vector<std::string> order = order_of(BITS);
        CHECK((int) order.size() == R::GROUPS, "%d groups", R::GROUPS);
        std::vector<int> seen((size_t) R::GROUPS, 0);
        for (int k = 0; k < 16; ++k) {
            const int g = R::lo_group(k);
            CHECK(g >= 0 && g < R::GROUPS - (R::TAIL < 4 ? 1 : 0), "L%d at %d", k, g);
            if (g >= 0 && g < R::GROUPS) {
                CHECK(order[(size_t) g] == "L" + std::to_string(k), "group %d is %s, not L%d", g, order[(size_t) g].c_str(), k);
                ++seen[(size_t) g];
            }
            CHECK(R::hi_need(k) == ((4 * BITS * k + 4 * BITS - 1) / 32) / 4, "row %d needs H%d", k, R::hi_need(k));
        }
        for (int h = 0; h < R::HGROUPS; ++h) {
            const int g = R::hi_group(h);
            CHECK(g >= 0 && g < R::GROUPS, "H%d at %d", h, g);
            if (g >= 0 && g < R::GROUPS) {
                CHECK(order[(size_t) g] == "H" + std::to_string(h), "group %d is %s, not H%d", g, order[(size_t) g].c_str(), h);
                ++seen[(size_t) g];
            }
            const int k0 = R::hi_row(h);  // the first row that needs H_h
            CHECK(k0 >= 0 && k0 < 16 && R::hi_need(k0) >= h && (k0 == 0 || R::hi_need(k0 - 1) < h), "first row of H%d: %d", h, k0);
        }
        for (int g = 0; g < R::GROUPS; ++g) CHECK(seen[(size_t) g] == 1, "group %d used %d times", g, seen[(size_t) g]);
        CHECK(R::TAIL == 4 || R::hi_group(R::HGROUPS - 1) == R::GROUPS - 1, "a short H group is the last group");
        // the 256 lanes' parts of the groups tile the record exactly
        std::vector<int> used(R::BYTES / 4, 0);
        for (int g = 0; g < R::GROUPS; ++g)
            for (int t = 0; t < 256; ++t)
                for (int e = 0; e < (g == R::GROUPS - 1 ? R::TAIL : 4); ++e) {
                    const int at = R::group_dword(g, t) + e;
                    CHECK(at >= 0 && at < R::BYTES / 4, "group %d thread %d at dword %d", g, t, at);
                    if (at >= 0 && at < R::BYTES / 4) ++used[(size_t) at];
                }
        int holes = 0;
        for (int u : used) holes += u != 1;
        CHECK(holes == 0, "%d dwords of the record not used exactly once", holes);
        // a group is stored once complete, never before a row that still writes into it, and all by the last row
        int done = 0;
        for (int k = 0; k < 16; ++k) {
            const int now = R::hi_done(k);
            CHECK(now >= done && now <= R::HGROUPS, "H groups done after row %d: %d", k, now);
            for (int h = 0; h < now; ++h) {
                const int last_dword = h == R::HGROUPS - 1 ? R::HDW - 1 : 4 * h + 3;
                CHECK(32 * (last_dword + 1) <= 4 * BITS * (k + 1), "H%d stored after row %d is not complete", h, k);
            }
            done = now;
        }
        CHECK(done == R::HGROUPS, "H groups done after the last row: %d", done);
    }

    // ---- round trip of whole lane records, through the record order ----
    int bad = 0, cases = 0;
    const uint64_t mants[] = { 0, ONES_MANT, ALT_MANT, ALT_MANT >> 1 };
    const uint32_t Es[] = { 16, 17, 1022, 1023, 2046 };
    for (uint32_t E : Es) {
        const uint32_t base = R::base(E);
        for (int lane_t : { 0, 1, 63, 64, 255 }) {
            // each position x the lowest / highest exponent x each mantissa pattern (4 = random), neighbours at all ones /
            // all zeros / random
            for (int pos = 0; pos < 64; ++pos)
                for (int eo = 0; eo < 2; ++eo)
                    for (int mp = 0; mp < 5; ++mp)
                        for (int nb = 0; nb < 3; ++nb) {
                            if (lane_t != 0 && lane_t != 255 && (mp + nb + pos) % 3) continue;  // a thinner sweep for the middle lanes
                            uint64_t v[64];
                            for (int i = 0; i < 64; ++i) {
                                if (nb == 0) v[i] = ((uint64_t) E << 52) | ONES_MANT;         // field all ones, low dword all ones
                                else if (nb == 1) v[i] = (uint64_t) (E - SPAN) << 52;         // field all zeros
                                else v[i] = ((uint64_t) (E - (rng() % (SPAN + 1))) << 52) | (rng() & ONES_MANT);
                            }
                            v[pos] = ((uint64_t) (E - SPAN + (uint32_t) eo * SPAN) << 52) | (mp < 4 ? mants[mp] : (rng() & ONES_MANT));
                            lane_io<BITS> io;
                            io.t = lane_t;
                            io.store(v, base);
                            for (int k = 0; k < 16; ++k)
                                for (int nt = 0; nt < 4; ++nt) {
                                    const int i = 4 * k + nt, j = R::word(i);
                                    const uint32_t w1 = R::straddles(i) ? io.hi(j + 1) : 0xA5A5A5A5u;
                                    const uint64_t back = join(R::unpack(i, io.hi(j), w1, base), io.lo(k, nt));
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

    // ---- what a row reads: L_k and the H groups up to hi_need(k), each stream dword the right number of times ----
    {
        uint64_t v[64];
        for (int i = 0; i < 64; ++i) v[i] = ((uint64_t) (1022 - (rng() % (SPAN + 1))) << 52) | (rng() & ONES_MANT);
        lane_io<BITS> io;
        io.t = 200;
        io.store(v, R::base(1022));
        int last = -1;
        for (int k = 0; k < 16; ++k) {
            for (int nt = 0; nt < 4; ++nt) CHECK(io.load(k, nt, R::base(1022)) == v[4 * k + nt], "value %d read row by row", 4 * k + nt);
            CHECK(io.reads_lo[k] == 4, "row %d read %d low dwords", k, io.reads_lo[k]);
            const int want = R::lo_group(k) > R::hi_group(R::hi_need(k)) ? R::lo_group(k) : R::hi_group(R::hi_need(k));
            CHECK(io.max_group_of_row[k] == want, "row %d reads up to group %d, not %d", k, io.max_group_of_row[k], want);
            CHECK(io.max_group_of_row[k] > last, "row %d completes at group %d, not after %d", k, io.max_group_of_row[k], last);
            last = io.max_group_of_row[k];
        }
        CHECK(last == R::GROUPS - 1, "the last row completes at group %d", last);
        for (int j = 0; j < R::HDW; ++j) CHECK(io.reads_hi[j] >= 1 && io.reads_hi[j] <= 3, "stream dword %d read %d times", j, io.reads_hi[j]);
    }
    return cases;
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double denorm = std::numeric_limits<double>::denorm_min();
    const double min_normal = std::numeric_limits<double>::min();
    const double max = std::numeric_limits<double>::max();
    const double below_one = 0.99999999999999989;  // the largest double below 1

    // ---- classification boundaries: one odd value at moving positions ----
    CHECK(all_positions(1.0, 1.0, NARROW, 1023), "all ones must be narrow with E = 1023");
    CHECK(all_positions(1.0, 1.0000000000000004, NARROW, 1023), "1 + 2 ulp among ones must be narrow");
    CHECK(all_positions(0.75, 0.5, NARROW, 1022), "one binade must be narrow");
    CHECK(all_positions(0.75, below_one, NARROW, 1022), "one binade (mantissa all ones) must be narrow");
    CHECK(all_positions(0.75, 0.25, NARROW, 1022), "exponents {E - 1, E} must be narrow");
    CHECK(all_positions(0.26, 0.99, NARROW, 1022), "exponents {E - 1, E}, the odd one on top, must be narrow");
    CHECK(all_positions(0.75, 0.2499999, WIDE, 1022), "exponents {E - 2, E} must be wide");
    CHECK(all_positions(0.75, 0.125, WIDE, 1022), "exponents {E - 2, E} (a power of two) must be wide");
    CHECK(all_positions(0.2, 0.75, WIDE, 1022), "exponents {E - 2, E}, the odd one on top, must be wide");
    CHECK(all_positions(1.0, std::ldexp(1.0, -15), WIDE, 1023), "span 15 must be wide");
    CHECK(all_positions(1.9999, std::ldexp(1.0, -15), WIDE, 1023), "span 15 (mantissas differ) must be wide");
    CHECK(all_positions(1.0, std::ldexp(1.0, -16), RAW, 0), "span 16 must be raw");
    CHECK(all_positions(1.0, std::ldexp(1.9999, -16), RAW, 0), "just under 15 binades down must be raw");
    CHECK(all_positions(0.75, 0.99, NARROW, 1022), "values in [0.5, 1) must be narrow");
    CHECK(all_positions(0.75, 1.0, NARROW, 1023), "an exact 1.0 among values in [0.5, 1) must be narrow");
    CHECK(all_positions(0.3, 1.0, WIDE, 1023), "an exact 1.0 among values in [0.25, 0.5) must be wide");
    for (double fill : { 0.75, 1.0 }) {
        CHECK(all_positions(fill, -fill, RAW, 0), "a negative value must be raw");
        CHECK(all_positions(fill, -std::ldexp(1.0, -3), RAW, 0), "a small negative value must be raw");
        CHECK(all_positions(fill, 0.0, RAW, 0), "a zero must be raw");
        CHECK(all_positions(fill, -0.0, RAW, 0), "a negative zero must be raw");
        CHECK(all_positions(fill, denorm, RAW, 0), "a denormal must be raw");
        CHECK(all_positions(fill, inf, RAW, 0), "inf must be raw");
        CHECK(all_positions(fill, -inf, RAW, 0), "-inf must be raw");
        CHECK(all_positions(fill, nan, RAW, 0), "NaN must be raw");
        CHECK(all_positions(fill, -nan, RAW, 0), "-NaN must be raw");
    }
    // the edges of E
    CHECK(all_positions(std::ldexp(1.0, -1007), std::ldexp(1.5, -1007), NARROW, 16), "E = 16, one binade, must be narrow");
    CHECK(all_positions(std::ldexp(1.0, -1007), std::ldexp(1.5, -1008), NARROW, 16), "E = 16 with E - 1 must be narrow");
    CHECK(all_positions(std::ldexp(1.0, -1007), min_normal, WIDE, 16), "E = 16 with the smallest normal must be wide");
    CHECK(all_positions(std::ldexp(1.0, -1008), std::ldexp(1.5, -1008), RAW, 0), "E = 15 must be raw");
    CHECK(all_positions(std::ldexp(1.0, -1008), std::ldexp(1.0, -1008), RAW, 0), "E = 15, one value, must be raw");
    // E - 15 < 1: E = 8 here, the smallest normal lies inside [E - 15, E] but the base would not be a normal exponent
    CHECK(all_positions(std::ldexp(1.0, -1015), min_normal, RAW, 0), "the smallest normal with E - 15 < 1 must be raw");
    CHECK(all_positions(std::ldexp(1.0, -1015), denorm, RAW, 0), "a denormal beside tiny values must be raw");
    CHECK(all_positions(min_normal, min_normal, RAW, 0), "E = 1 must be raw");
    CHECK(all_positions(min_normal, denorm, RAW, 0), "a denormal beside the smallest normals must be raw");
    CHECK(all_positions(max, max, NARROW, 2046), "E = 2046, one value, must be narrow");
    CHECK(all_positions(max, std::ldexp(1.0, 1023), NARROW, 2046), "E = 2046 must be narrow");
    CHECK(all_positions(max, std::ldexp(1.0, 1022), NARROW, 2046), "E = 2046 with 2045 must be narrow");
    CHECK(all_positions(std::ldexp(1.0, 1023), inf, RAW, 0), "inf beside E = 2046 must be raw");
    // descriptors: one uniform compare tells the forms apart, and the flag lies above bit 11
    CHECK(KP_DESC_NARROW > 0x800u && (KP_DESC_NARROW & 2047u) == 0, "the flag bit lies above bit 11");
    CHECK(!kp_desc_is_narrow(KP_DESC_RAW) && !kp_desc_is_narrow(2046u) && kp_desc_is_narrow(16u | KP_DESC_NARROW), "the compare");
    CHECK(kp_record<24>::base(16) == (1u << 20) && kp_record<21>::base(16) == (15u << 20), "the smallest bases");

    // ---- a single value at every exponent offset of either width: the field fits and comes back bit-exact ----
    std::mt19937_64 rng(20240917);
    int bad = 0;
    for (int i = 0; i < 100000; ++i) {
        const uint32_t E = 16 + (uint32_t) (rng() % (2046 - 16 + 1)), off = (uint32_t) (rng() % 16);
        const uint64_t mant = i % 3 == 0 ? 0 : (i % 3 == 1 ? ONES_MANT : (rng() & ONES_MANT));
        const uint64_t u = ((uint64_t) (E - off) << 52) | mant;
        const uint32_t f24 = (uint32_t) (u >> 32) - kp_record<24>::base(E), f21 = (uint32_t) (u >> 32) - kp_record<21>::base(E);
        bad += (f24 >> 24) != 0 || join(kp_record<24>::unpack(0, f24, 0, kp_record<24>::base(E)), (uint32_t) u) != u;
        if (off <= 1) bad += (f21 >> 21) != 0 || join(kp_record<21>::unpack(0, f21, 0, kp_record<21>::base(E)), (uint32_t) u) != u;
    }
    CHECK(bad == 0, "%d of 100000 random values did not round-trip", bad);

    // ---- both widths: stream positions, record order, stores, whole-lane round trips, the groups a row reads ----
    CHECK(kp_record<24>::HDW == 48 && kp_record<24>::HGROUPS == 12 && kp_record<24>::TAIL == 4 && kp_record<24>::GROUPS == 28 &&
              kp_record<24>::BYTES == 114688, "the wide record's sizes");
    CHECK(kp_record<21>::HDW == 42 && kp_record<21>::HGROUPS == 11 && kp_record<21>::TAIL == 2 && kp_record<21>::GROUPS == 27 &&
              kp_record<21>::BYTES == 108544, "the narrow record's sizes");
    const int wide = check_width<KP_BITS_WIDE>(rng), narrow = check_width<KP_BITS_NARROW>(rng);

    if (failures) return 1;
    std::printf("%d wide and %d narrow lane records\nok\n", wide, narrow);
    return 0;
}
