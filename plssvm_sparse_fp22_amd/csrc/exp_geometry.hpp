// Host decisions of the kernel expansion's setup (expand_setup.hip) as plain integer arithmetic: no
// HIP, so tests/exp_geometry_check.cpp runs them on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>

namespace plssvm_mi {

constexpr int EXP_NWV = 16;  // waves per remainder-stream workgroup (one workgroup per CU)
// Remainder-stream geometry: one 1024-thread workgroup per block of RB rows (RB / EXP_NWV rows per
// wave) holds an LDS row accumulator (RB values) and one LDS window of CW partners (the next window is
// prefetched into registers), together the CU's 160 KiB. RBB = accumulator bytes in {4, 8, 16, 32} KiB;
// setup picks the largest whose block count still fills the CUs (bigger blocks = w restaged fewer
// times; a bigger window = fewer (row, window) groups = less 4-slot padding).
constexpr int EXP_LDS = 163840;
inline int exp_cw_host(int rbb, int es) { return (EXP_LDS - rbb) / es / 1024 * 1024; }
// bfloat16 windows (hbf16, expand_setup.hip "H storage"): twice the partners in the same LDS, at most 65536
// (16-bit window-local j)
inline int exp_cw16_host(int rbb) { return std::min((EXP_LDS - rbb) / 2 / 1024 * 1024, 65536); }

struct exp_geometry {
    int RBB = 32768, RB = EXP_NWV, G = 1;  // accumulator bytes, rows per block, window groups per row block
    int CW = 0;                            // partners per window
    int64_t nW = 0;                        // windows
};

// Rows per block RB = the rank's R rows spread evenly over the CUs (a multiple of EXP_NWV: one round of blocks,
// every CU busy), at most what the largest accumulator class holds (the rest of the LDS is the window). Few rows (an
// 8-GPU rank's share: blocks of less than half the largest class): still the largest class, and G window groups per
// row block to fill the CUs — every row block restages all of w once, so fewer, bigger row blocks restage less.
// forced_rbb (a class, PLSSVM_MI_EXP_RBB) and forced_g (>= 1, PLSSVM_MI_EXP_G) override; 0: not forced.
inline exp_geometry exp_choose_geometry(int64_t R, int cus, int es, int forced_rbb, int forced_g) {
    const auto cdiv = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    const auto rup = [&](int64_t a, int64_t b) { return cdiv(a, b) * b; };
    exp_geometry g;
    cus = std::max(cus, 1);
    const int64_t Rr = std::max<int64_t>(R, 1), cap_max = 32768 / es;
    const int64_t want = rup(cdiv(Rr, (int64_t) cus), (int64_t) EXP_NWV);
    if (want * 2 > cap_max) {
        // more than half of the largest class: want es > 16384, so no smaller class holds the block (the smaller
        // classes are reached only when forced)
        g.RB = (int) std::min<int64_t>(want, cap_max);
    } else {
        int64_t nI = cdiv(Rr, cap_max);
        g.G = (int) std::max<int64_t>(1, cus / nI);
        // as many row blocks as the G window groups leave CUs (3-RBF: 128 x 2 = 256 workgroups, not 123 x 2)
        nI = std::max<int64_t>(nI, cus / g.G);
        g.RB = (int) rup(cdiv(Rr, nI), (int64_t) EXP_NWV);
    }
    if (forced_rbb == 4096 || forced_rbb == 8192 || forced_rbb == 16384 || forced_rbb == 32768)
        g.RBB = forced_rbb, g.RB = forced_rbb / es, g.G = 1;
    if (forced_g >= 1) g.G = forced_g;
    return g;
}

// the windows of m partners: CW from the accumulator class and the window's format (bfloat16 windows hold twice the
// partners), and no more window groups than windows
inline void exp_set_windows(exp_geometry &g, int es, bool hbf16, int64_t m) {
    g.CW = hbf16 ? exp_cw16_host(g.RBB) : exp_cw_host(g.RBB, es);
    g.nW = (std::max<int64_t>(m, 1) + g.CW - 1) / g.CW;
    g.G = (int) std::max<int64_t>(1, std::min<int64_t>(g.G, g.nW));
}

// partners per row of the one-pass joins' slot pool, from the setup's sample of the rank's rows (mean and max
// partners per row); forced > 0 (PLSSVM_MI_EXP_RJ_CAP) is taken as it is
inline int64_t exp_slot_cap(double rj_mean, double rj_max, int64_t forced) {
    if (forced > 0) return forced;
    const int64_t c = std::max<int64_t>({ (int64_t) (2.0 * rj_mean), (int64_t) (1.5 * rj_max), 64 });
    return (c + 7) / 8 * 8;
}

// PLSSVM_MI_EXP_ROWS
constexpr int EXP_ROWS_INDEX = -1, EXP_ROWS_AUTO = 0, EXP_ROWS_FLAGS = 1, EXP_ROWS_PAIRS = 2;

// flagged chunks instead of a row index per chunk: when every |H| < 2 (bit 14 of a stored bfloat16 is free) and the
// dummies of the empty cells (16 B each) cost at most half of the row indices they replace (2 B per chunk of 4
// slots); =flags / =pairs force them when the bit is free, =index keeps the row index
inline bool exp_take_chunk_flags(int64_t dummy_cells, bool big_h, int64_t indexed_slots, int rows_opt) {
    if (rows_opt < 0 || big_h) return false;
    const double chunks = (double) indexed_slots / 4.0;
    return rows_opt >= 1 || 16.0 * (double) dummy_cells <= 0.5 * 2.0 * chunks;
}

// pair flags (cells padded to 2 slots, slots2 in all) instead of chunk flags (4 slots, slots4): when they save
// >= 3 % of the slots; =pairs forces them, =flags keeps the chunk flags
inline bool exp_take_pair_flags(int64_t slots2, int64_t slots4, int rows_opt) {
    if (rows_opt == EXP_ROWS_FLAGS) return false;
    return rows_opt == EXP_ROWS_PAIRS || (double) slots2 <= 0.97 * (double) slots4;
}

}  // namespace plssvm_mi
