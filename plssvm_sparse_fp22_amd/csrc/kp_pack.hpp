// Lossless 7-byte form of the fp64 values of a stored kernel-matrix tile.
//
// Inside one 128 x 128 tile of an RBF matrix every value is positive and the exponents span a few binades, so the
// 12 bits of sign and exponent carry almost nothing. A tile whose 16 384 values are all positive normal numbers with
// biased exponents in [E - 15, E] (E = the largest one, >= 16) is "packable": a value is kept as its low 32 mantissa
// bits plus the 24-bit word  h24 = ((e - (E - 15)) << 20) | mantissa[51:32]  =  high dword - ((E - 15) << 20),
// and comes back as  high dword = h24 + ((E - 15) << 20): one integer add with a tile-wide operand. Every other
// tile (a sign, a zero, a denormal, an inf, a NaN, a wider span) keeps its raw 8-byte record.
//
// Four values (one (mt, r) row of a lane, kp_tiles.hip) make seven dwords: the four low dwords as they are, and the
// four 24-bit words in three dwords (kp_pack4 / kp_unpack4).
//
// Plain functions on uint32_t / uint64_t, for host and device: the store kernel, the load kernel and the CPU test
// (tests/kp_pack_check.cpp) all call these.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KP_PACK_FN __host__ __device__ inline
#else
#define KP_PACK_FN inline
#endif

namespace plssvm_mi {

constexpr uint32_t KP_PACK_SPAN = 15;  // binades below E that the 4-bit exponent offset reaches
constexpr uint32_t KP_PACK_RAW = 0;    // descriptor of a tile that keeps its raw record (else: the tile's E)

// Running range of a tile's high dwords. A value that can never be packed (sign bit set, biased exponent 0 or 2047:
// -x, +-0, denormals, inf, NaN) pulls the minimum to 0, which no packable range contains.
KP_PACK_FN void kp_pack_track(uint32_t hi, uint32_t &mn, uint32_t &mx) {
    const bool bad = (hi - 0x00100000u) >= (0x7FF00000u - 0x00100000u);  // e == 0, e == 2047 or negative
    const uint32_t v = bad ? 0u : hi;
    mn = v < mn ? v : mn;
    mx = hi > mx ? hi : mx;
}
constexpr uint32_t KP_PACK_MN0 = 0xFFFFFFFFu, KP_PACK_MX0 = 0u;  // the empty range

// Descriptor of a tile from the range of all its values: E (16 .. 2046) when packable, else KP_PACK_RAW.
KP_PACK_FN uint32_t kp_pack_desc(uint32_t mn, uint32_t mx) {
    const uint32_t E = mx >> 20, e0 = mn >> 20;
    if (E > 2046u || E <= KP_PACK_SPAN) return KP_PACK_RAW;  // E - 15 must be a normal number's exponent (>= 1)
    if (e0 < E - KP_PACK_SPAN) return KP_PACK_RAW;           // also every "bad" value: e0 = 0
    return E;
}

// the tile-wide operand of the decode
KP_PACK_FN uint32_t kp_pack_base(uint32_t E) { return (E - KP_PACK_SPAN) << 20; }

// one value
KP_PACK_FN uint32_t kp_pack_h24(uint32_t hi, uint32_t base) { return hi - base; }
KP_PACK_FN uint32_t kp_unpack_hi(uint32_t h24, uint32_t base) { return h24 + base; }

// four 24-bit words <-> three dwords (little end first: value 0 in the low 24 bits of w[0])
KP_PACK_FN void kp_pack4(const uint32_t hi[4], uint32_t base, uint32_t w[3]) {
    const uint32_t h0 = hi[0] - base, h1 = hi[1] - base, h2 = hi[2] - base, h3 = hi[3] - base;
    w[0] = h0 | (h1 << 24);
    w[1] = (h1 >> 8) | (h2 << 16);
    w[2] = (h2 >> 16) | (h3 << 8);
}
// the high dword of value k (0..3) of the three dwords w0, w1, w2
KP_PACK_FN uint32_t kp_unpack4(int k, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t base) {
    uint32_t h;
    switch (k) {
        case 0: h = w0 & 0x00FFFFFFu; break;
        case 1: h = (uint32_t) (((((uint64_t) w1) << 32) | w0) >> 24) & 0x00FFFFFFu; break;
        case 2: h = (uint32_t) (((((uint64_t) w2) << 32) | w1) >> 16) & 0x00FFFFFFu; break;
        default: h = w2 >> 8; break;
    }
    return h + base;
}

// Record layout of a packed tile, in 16-byte groups per lane ([group][thread][16 B], as the raw record). A lane's 64
// values are 16 rows (mt, r) of four; the four rows of one mt take seven groups:
//   7 mt + 0: low dwords of row r = 0     7 mt + 1: high words, dwords 0..3  of the mt's 12 (row r: dwords 3r .. 3r+2)
//   7 mt + 2: low dwords of row r = 1     7 mt + 3: high words, dwords 4..7
//   7 mt + 4: low dwords of row r = 2     7 mt + 5: high words, dwords 8..11
//   7 mt + 6: low dwords of row r = 3
// so row (mt, r) is complete once group 7 mt + 2 r (+ 1 for r < 3) has arrived: the groups come in the order the
// epilogue consumes the rows. 28 groups = 448 B per lane, 112 KiB per tile, against 32 groups = 128 KiB raw.
constexpr int KP_PACK_GROUPS = 28;
KP_PACK_FN constexpr int kp_pack_lo_group(int mt, int r) { return 7 * mt + 2 * r; }
KP_PACK_FN constexpr int kp_pack_hi_group(int mt, int dword) { return 7 * mt + 1 + 2 * (dword >> 2); }  // dword 0..11

// bit casts kept in plain integer arithmetic for the callers
KP_PACK_FN uint64_t kp_pack_join(uint32_t hi, uint32_t lo) { return ((uint64_t) hi << 32) | lo; }

}  // namespace plssvm_mi
