// Lossless packed forms of the fp64 values of a stored kernel-matrix tile.
//
// Inside one 128 x 128 tile of an RBF matrix every value is positive and the exponents span a few binades, so the
// 12 bits of sign and exponent carry almost nothing. A tile whose 16 384 values are all positive normal numbers with
// biased exponents in [E - S, E] (E = the largest one, >= 16; S = 2^(BITS - 20) - 1) keeps a value as its low 32
// mantissa bits plus the BITS-wide field  f = ((e - (E - S)) << 20) | mantissa[51:32]  =  high dword - ((E - S) << 20),
// and gets it back as  high dword = f + ((E - S) << 20): one integer add with a tile-wide operand. Two widths are
// stored: BITS = 24 ("wide", S = 15, 7 bytes per value) and BITS = 21 ("narrow", S = 1, 53 bits per value: 52 mantissa
// bits cannot be compressed, so that is the floor of a lossless record). Every other tile (a sign, a zero, a denormal,
// an inf, a NaN, a wider span) keeps its raw 8-byte record.
//
// A lane's 64 values (v = 16 mt + 4 r + nt, kp_tiles.hip: row k = 4 mt + r holds v = 4 k .. 4 k + 3) become the 64 low
// dwords, one dwordx4 per row (L0 .. L15), and the 64 fields as one little-endian bit stream of 2 BITS dwords, value v
// at bit BITS v, cut into dwordx4 groups H0 .. (BITS = 21: the last one, H10, is a dwordx2).
//
// Plain functions on uint32_t, for host and device: the store kernel, the load kernel and the CPU test
// (tests/kp_record_check.cpp) all call these.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KP_REC_FN __host__ __device__ inline
#else
#define KP_REC_FN inline
#endif

namespace plssvm_mi {

constexpr int KP_BITS_WIDE = 24, KP_BITS_NARROW = 21;
// A tile's descriptor: KP_DESC_RAW, its E (16 .. 2046) when wide, E | KP_DESC_NARROW when narrow. One uniform compare
// tells the forms apart: desc >= KP_DESC_NARROW, else desc != KP_DESC_RAW.
constexpr uint32_t KP_DESC_RAW = 0, KP_DESC_NARROW = 0x1000u;
KP_REC_FN bool kp_desc_is_narrow(uint32_t desc) { return desc >= KP_DESC_NARROW; }
KP_REC_FN uint32_t kp_desc_exp(uint32_t desc) { return desc & (KP_DESC_NARROW - 1u); }

// Running range of a tile's high dwords. A value that can never be packed (sign bit set, biased exponent 0 or 2047:
// -x, +-0, denormals, inf, NaN) pulls the minimum to 0, which no packable range contains.
KP_REC_FN void kp_pack_track(uint32_t hi, uint32_t &mn, uint32_t &mx) {
    const bool bad = (hi - 0x00100000u) >= (0x7FF00000u - 0x00100000u);  // e == 0, e == 2047 or negative
    const uint32_t v = bad ? 0u : hi;
    mn = v < mn ? v : mn;
    mx = hi > mx ? hi : mx;
}
constexpr uint32_t KP_PACK_MN0 = 0xFFFFFFFFu, KP_PACK_MX0 = 0u;  // the empty range

// Descriptor of a tile from the range of all its values. pack: 0 every tile raw, 1 raw or wide, 2 all three forms.
KP_REC_FN uint32_t kp_desc(uint32_t mn, uint32_t mx, int pack) {
    const uint32_t E = mx >> 20, e0 = mn >> 20;
    if (pack <= 0 || E > 2046u || E <= 15u) return KP_DESC_RAW;  // E - 15 must be a normal number's exponent (>= 1)
    if (e0 < E - 15u) return KP_DESC_RAW;                        // also every "bad" value: e0 = 0
    return (pack >= 2 && E - e0 <= 1u) ? (E | KP_DESC_NARROW) : E;
}

template <int BITS>
struct kp_record {
    static_assert(BITS > 20 && BITS <= 24, "the field holds the 20 high mantissa bits and an exponent offset");
    static constexpr uint32_t MASK = (1u << BITS) - 1u;
    static constexpr int HDW = 2 * BITS;               // dwords of a lane's bit stream: 48, 42
    static constexpr int HGROUPS = (HDW + 3) / 4;      // 12, 11
    static constexpr int TAIL = HDW - 4 * (HGROUPS - 1);  // dwords of the last H group: 4, 2 (then it is [thread][8 B])
    static constexpr int GROUPS = 16 + HGROUPS;        // 28, 27
    static constexpr int BYTES = 256 * 4 * (64 + HDW);  // 114 688, 108 544 per tile, against 131 072 raw

    // the tile-wide operand of the decode: (E - 15) << 20, (E - 1) << 20
    static KP_REC_FN uint32_t base(uint32_t E) { return (E - (MASK >> 20)) << 20; }

    // Where value v (0 .. 63) sits in the bit stream: dword word(v), bit shift(v) of it. A field that does not fit the
    // rest of its dword continues in the next one (never past the last: value 63 ends with the stream).
    static KP_REC_FN constexpr int word(int v) { return (BITS * v) >> 5; }
    static KP_REC_FN constexpr int shift(int v) { return (BITS * v) & 31; }
    static KP_REC_FN constexpr bool straddles(int v) { return shift(v) > 32 - BITS; }

    // Appends value v's field to the stream w[0 .. HDW). Called for v = 0, 1, 2, ... in order, it writes every dword
    // before it ORs into it (the field that reaches a dword first assigns it), so w needs no zero fill and, unrolled,
    // every dword is a value of its own that lives from its first field to its store.
    static KP_REC_FN void put(int v, uint32_t f, uint32_t *w) {
        const int j = word(v), sh = shift(v);
        if (sh == 0) w[j] = f;
        else w[j] |= f << sh;
        if (straddles(v)) w[j + 1] = f >> (32 - sh);
    }

    // The high dword of value v from the stream's dwords w0 = w[word(v)] and w1 = w[word(v) + 1] (w1 is not looked at
    // unless straddles(v): pass anything). Every shift is a constant in 1 .. 31 once v is.
    static KP_REC_FN uint32_t unpack(int v, uint32_t w0, uint32_t w1, uint32_t base) {
        const int sh = shift(v);
        uint32_t f;
        if (!straddles(v)) f = w0 >> sh;
        else f = (uint32_t) (((((uint64_t) w1) << 32) | w0) >> sh);
        return (f & MASK) + base;
    }

    // Record layout: [group][thread][16 B] like the raw record, a dwordx2 tail [thread][8 B]. The groups come in the
    // order the epilogue consumes the rows: row k needs L_k and the stream up to bit 4 BITS (k + 1), that is the H
    // groups up to hi_need(k); each H group follows the L group of the first row that needs it.
    //   24: L0 H0 L1 H1 L2 H2 L3 | L4 H3 L5 H4 L6 H5 L7 | ...  (seven groups per mt: 7 mt + 2 r, 7 mt + 1 + 2 i)
    //   21: L0 H0 L1 H1 L2 L3 H2 L4 H3 L5 L6 H4 L7 H5 L8 L9 H6 L10 H7 L11 L12 H8 L13 H9 L14 L15 H10
    static KP_REC_FN constexpr int hi_need(int k) { return (4 * BITS * (k + 1) - 1) >> 7; }  // last H group of row k
    static KP_REC_FN constexpr int hi_row(int h) { return (128 * h) / (4 * BITS); }          // first row that needs H_h
    static KP_REC_FN constexpr int lo_group(int k) { return k + (k == 0 ? 0 : hi_need(k - 1) + 1); }
    static KP_REC_FN constexpr int hi_group(int h) { return h + hi_row(h) + 1; }
    // H groups whose dwords are all written once rows 0 .. k are appended (the fill stores a group as soon as it is
    // complete)
    static KP_REC_FN constexpr int hi_done(int k) { return k == 15 ? HGROUPS : (4 * BITS * (k + 1)) >> 7; }
    // dword offset of thread t's part of record group g, from the record's start (256 threads)
    static KP_REC_FN constexpr int group_dword(int g, int t) { return g * 1024 + (g == GROUPS - 1 ? TAIL : 4) * t; }
};

}  // namespace plssvm_mi
