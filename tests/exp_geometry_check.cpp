// Stand-alone check of the kernel expansion's host decisions (csrc/exp_geometry.hpp: the remainder stream's geometry,
// the slot cap of the one-pass joins, the two layout rules), built and run by tests/test_exp_geometry_cpu.py (a second
// time under the address and undefined-behaviour sanitizers). The expected values are literals worked out by hand from
// the formulas of DESIGN.md §5. Exit status 0 and "ok" on success; every failing check is printed and the status is 1.
#include <cstdint>
#include <cstdio>

#include "exp_geometry.hpp"

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

constexpr int CUS = 256;

void geometry(int64_t R, int es, int rbb, int rb, int g, int64_t blocks, int frbb = 0, int fg = 0) {
    const exp_geometry x = exp_choose_geometry(R, CUS, es, frbb, fg);
    const int64_t nb = (R + x.RB - 1) / x.RB;
    CHECK(x.RBB == rbb && x.RB == rb && x.G == g && nb == blocks,
          "R %lld es %d forced (%d, %d): RBB %d RB %d G %d blocks %lld, want %d %d %d %lld", (long long) R, es, frbb, fg, x.RBB,
          x.RB, x.G, (long long) nb, rbb, rb, g, (long long) blocks);
    CHECK(x.RB >= EXP_NWV && x.RB % EXP_NWV == 0 && x.RB * es <= x.RBB, "R %lld es %d: RB %d does not fit class %d",
          (long long) R, es, x.RB, x.RBB);
}

void windows(int es, bool hbf16, int64_t m, int g_in, int cw, int64_t nw, int g_out) {
    exp_geometry x;
    x.RBB = 32768;
    x.G = g_in;
    exp_set_windows(x, es, hbf16, m);
    CHECK(x.CW == cw && x.nW == nw && x.G == g_out, "es %d hbf16 %d m %lld G %d: CW %d nW %lld G %d, want %d %lld %d", es,
          (int) hbf16, (long long) m, g_in, x.CW, (long long) x.nW, x.G, cw, (long long) nw, g_out);
}

}  // namespace

int main() {
    // ---- the two timed geometries, fp32, 256 CUs (3-RBF 128 row blocks x 2 = 256 workgroups; config 5's
    // row blocks of 7 824 rows) ----
    geometry(999999, 4, 32768, 7824, 2, 128);
    geometry(1999999, 4, 32768, 7824, 1, 256);
    windows(4, true, 1000000, 2, 65536, 16, 2);    // bfloat16 windows
    windows(4, false, 1000000, 2, 32768, 31, 2);   // float windows
    windows(4, true, 2000000, 1, 65536, 31, 1);
    windows(8, false, 1000000, 1, 16384, 62, 1);   // double windows
    CHECK(exp_cw16_host(32768) == 65536 && exp_cw_host(32768, 4) == 32768 && exp_cw_host(32768, 8) == 16384, "CW of 32 KiB");
    CHECK(exp_cw16_host(4096) == 65536 && exp_cw_host(4096, 4) == 39936 && exp_cw_host(16384, 8) == 18432, "CW of small classes");

    // ---- the accumulator class boundaries: with want = ceil(R / 256) rounded up to 16 rows per block, the values of R
    // where want x es crosses 4 096 / 8 192 / 16 384 / 32 768 bytes; want x 2 crosses cap_max = 32 768 / es at the
    // 16 384-byte boundary. Up to there the largest class is split into G window groups; beyond, one group, and past
    // 32 768 bytes the block is clamped to the class (then there are more blocks than CUs). ----
    // fp32
    geometry(262144, 4, 32768, 8192, 8, 32);    // want 1024: 4 096 B
    geometry(262145, 4, 32768, 7296, 7, 36);    // want 1040
    geometry(524288, 4, 32768, 8192, 4, 64);    // want 2048: 8 192 B
    geometry(524289, 4, 32768, 6176, 3, 85);    // want 2064
    geometry(1048576, 4, 32768, 8192, 2, 128);  // want 4096: 16 384 B, want x 2 == cap_max
    geometry(1048577, 4, 32768, 4112, 1, 256);  // want 4112: want x 2 > cap_max
    geometry(2097152, 4, 32768, 8192, 1, 256);  // want 8192: 32 768 B
    geometry(2097153, 4, 32768, 8192, 1, 257);  // want 8208: clamped
    // fp64
    geometry(131072, 8, 32768, 4096, 8, 32);    // want 512: 4 096 B
    geometry(131073, 8, 32768, 3648, 7, 36);    // want 528
    geometry(262144, 8, 32768, 4096, 4, 64);    // want 1024: 8 192 B
    geometry(262145, 8, 32768, 3088, 3, 85);    // want 1040
    geometry(524288, 8, 32768, 4096, 2, 128);   // want 2048: 16 384 B, want x 2 == cap_max
    geometry(524289, 8, 32768, 2064, 1, 255);   // want 2064: want x 2 > cap_max
    geometry(1048576, 8, 32768, 4096, 1, 256);  // want 4096: 32 768 B
    geometry(1048577, 8, 32768, 4096, 1, 257);  // want 4112: clamped

    // ---- edge values of R ----
    geometry(1, 4, 32768, 16, 256, 1);
    geometry(1, 8, 32768, 16, 256, 1);
    geometry(0, 4, 32768, 16, 256, 0);  // no division by zero; no blocks
    geometry(0, 8, 32768, 16, 256, 0);
    CHECK(exp_choose_geometry(1000, 0, 4, 0, 0).RB >= EXP_NWV, "no CU count: still a geometry");

    // ---- the knobs: a forced class sets RB = RBB / es and G = 1; a forced G is taken, and clamped to the windows ----
    geometry(999999, 4, 4096, 1024, 1, 977, 4096);
    geometry(999999, 4, 8192, 2048, 1, 489, 8192);
    geometry(999999, 4, 16384, 4096, 1, 245, 16384);
    geometry(999999, 4, 32768, 8192, 1, 123, 32768);
    geometry(999999, 8, 16384, 2048, 1, 489, 16384);
    geometry(999999, 4, 32768, 7824, 2, 128, 5000);      // not a class: ignored
    geometry(999999, 4, 32768, 7824, 5, 128, 0, 5);      // forced G
    geometry(999999, 4, 4096, 1024, 3, 977, 4096, 3);    // both
    geometry(999999, 4, 32768, 7824, 2, 128, 0, -1);     // not a count: ignored
    windows(4, true, 1000000, 100, 65536, 16, 16);       // G above nW: clamped
    windows(4, true, 1000000, 16, 65536, 16, 16);
    windows(4, true, 65536, 2, 65536, 1, 1);
    windows(4, true, 65537, 2, 65536, 2, 2);
    windows(4, false, 0, 3, 32768, 1, 1);                // no partners: one window
    windows(4, false, 5, 0, 32768, 1, 1);                // G is at least 1

    // ---- the slot cap: max(2 mean, 1.5 max, 64) rounded up to 8; a positive forced value as it is ----
    CHECK(exp_slot_cap(0.0, 0.0, 0) == 64, "floor");
    CHECK(exp_slot_cap(10.0, 20.0, 0) == 64, "floor over small samples");
    CHECK(exp_slot_cap(32.0, 10.0, 0) == 64 && exp_slot_cap(32.5, 10.0, 0) == 72, "2 x mean: 64 stays, 65 rounds up to 72");
    CHECK(exp_slot_cap(1.0, 48.0, 0) == 72 && exp_slot_cap(1.0, 49.0, 0) == 80, "1.5 x max: 72 stays, 73 rounds up to 80");
    CHECK(exp_slot_cap(100.0, 100.0, 0) == 200, "the larger of the two");
    CHECK(exp_slot_cap(100.0, 100.0, 8) == 8 && exp_slot_cap(100.0, 100.0, 13) == 13, "forced: taken as it is");
    CHECK(exp_slot_cap(100.0, 100.0, -5) == 200, "a negative forced value is ignored");

    // ---- chunk flags: every |H| < 2, and 16 B x dummies <= half of 2 B x chunks (chunks = indexed slots / 4), that is
    // 64 x dummies <= slots ----
    CHECK(exp_take_chunk_flags(100, false, 6400, EXP_ROWS_AUTO), "at equality: flags");
    CHECK(exp_take_chunk_flags(99, false, 6400, EXP_ROWS_AUTO), "fewer dummies: flags");
    CHECK(!exp_take_chunk_flags(101, false, 6400, EXP_ROWS_AUTO), "more dummies: index");
    CHECK(!exp_take_chunk_flags(100, false, 6396, EXP_ROWS_AUTO), "fewer slots: index");
    CHECK(!exp_take_chunk_flags(0, false, 6400, EXP_ROWS_INDEX), "=index keeps the row index");
    CHECK(exp_take_chunk_flags(1000000, false, 4, EXP_ROWS_FLAGS), "=flags forces the flags");
    CHECK(exp_take_chunk_flags(1000000, false, 4, EXP_ROWS_PAIRS), "=pairs needs the flags too");
    CHECK(!exp_take_chunk_flags(0, true, 6400, EXP_ROWS_AUTO), "an |H| >= 2: the bit is not free");
    CHECK(!exp_take_chunk_flags(0, true, 6400, EXP_ROWS_FLAGS) && !exp_take_chunk_flags(0, true, 6400, EXP_ROWS_PAIRS),
          "an |H| >= 2 vetoes the flags even when forced");

    // ---- pair flags: slots2 <= 0.97 slots4 ----
    CHECK(exp_take_pair_flags(9700, 10000, EXP_ROWS_AUTO), "at equality: pairs");
    CHECK(exp_take_pair_flags(9699, 10000, EXP_ROWS_AUTO), "saves more: pairs");
    CHECK(!exp_take_pair_flags(9701, 10000, EXP_ROWS_AUTO), "saves less: chunk flags");
    CHECK(exp_take_pair_flags(10000, 10000, EXP_ROWS_PAIRS), "=pairs forces them");
    CHECK(!exp_take_pair_flags(1, 10000, EXP_ROWS_FLAGS), "=flags keeps the chunk flags");

    if (failures == 0) std::printf("ok\n");
    return failures == 0 ? 0 : 1;
}
