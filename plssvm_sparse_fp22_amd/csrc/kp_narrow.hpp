// Lossless 53-bit form of the fp64 values of a stored kernel-matrix tile, beside the raw record and
// the 7-byte form of kp_pack.hpp.
//
// A packable tile (kp_pack.hpp) whose biased exponents are E - 1 and E only (E = the largest one) is "narrow": a value
// is kept as its low 32 mantissa bits plus the 21-bit word  h21 = ((e - (E - 1)) << 20) | mantissa[51:32]  =
// high dword - ((E - 1) << 20),  and comes back as  high dword = h21 + ((E - 1) << 20). 52 mantissa bits cannot be
// compressed, so 53 bits per value is the floor of a lossless record.
//
// A lane's 64 values (v = 16 mt + 4 r + nt, kp_tiles.hip: row k = 4 mt + r holds v = 4 k .. 4 k + 3) make 106 dwords:
// the 64 low dwords (one dwordx4 per row: L0 .. L15) and the 64 21-bit words as one little-endian bit stream of 1 344
// bits = 42 dwords, value v at bit 21 v (H0 .. H9 as dwordx4, H10 = dwords 40 and 41 as a dwordx2).
//
// Plain functions on uint32_t, for host and device: the store kernel, the load kernel and the CPU test
// (tests/kp_narrow_check.cpp) all call these.
#pragma once

#include <cstdint>

#include "kp_pack.hpp"

namespace plssvm_mi {

constexpr uint32_t KP_NARROW_FLAG = 0x1000u;  // descriptor of a narrow tile: E | KP_NARROW_FLAG (E <= 2046 < 0x1000)
constexpr uint32_t KP_NARROW_MASK = 0x001FFFFFu;
constexpr int KP_NARROW_BITS = 21;
constexpr int KP_NARROW_HDW = 42;     // dwords of a lane's bit stream
constexpr int KP_NARROW_HGROUPS = 11; // H0 .. H9 (16 B per lane) and H10 (8 B per lane)
constexpr int KP_NARROW_GROUPS = 27;  // 16 L groups + 11 H groups; the last one (H10) is [thread][8 B]
constexpr int KP_NARROW_DWORDS = 106;

// Descriptor of a tile from the range of all its values (kp_pack_track): E | KP_NARROW_FLAG when narrow, else what
// kp_pack_desc says (E: 7-byte form, KP_PACK_RAW: raw). One uniform compare tells the forms apart:
// desc >= KP_NARROW_FLAG, else desc != KP_PACK_RAW.
KP_PACK_FN uint32_t kp_narrow_desc(uint32_t mn, uint32_t mx) {
    const uint32_t E = kp_pack_desc(mn, mx);
    if (E == KP_PACK_RAW) return KP_PACK_RAW;
    return ((mx >> 20) - (mn >> 20) <= 1u) ? (E | KP_NARROW_FLAG) : E;
}
KP_PACK_FN bool kp_desc_is_narrow(uint32_t desc) { return desc >= KP_NARROW_FLAG; }
KP_PACK_FN uint32_t kp_desc_exp(uint32_t desc) { return desc & (KP_NARROW_FLAG - 1u); }

// the tile-wide operand of the decode (E >= 16 for every packable tile)
KP_PACK_FN uint32_t kp_narrow_base(uint32_t E) { return (E - 1u) << 20; }

// one value
KP_PACK_FN uint32_t kp_narrow_h21(uint32_t hi, uint32_t base) { return hi - base; }

// Where value v (0 .. 63) sits in the bit stream: dword kp_narrow_word(v), bit kp_narrow_shift(v) of it. A word that
// starts at bit <= 11 lies inside its dword; any other continues in the next dword (never past dword 41: value 63
// starts at bit 11 of dword 41).
KP_PACK_FN constexpr int kp_narrow_word(int v) { return (KP_NARROW_BITS * v) >> 5; }
KP_PACK_FN constexpr int kp_narrow_shift(int v) { return (KP_NARROW_BITS * v) & 31; }
KP_PACK_FN constexpr bool kp_narrow_straddles(int v) { return kp_narrow_shift(v) > 32 - KP_NARROW_BITS; }

// Appends value v's word to the stream w[0 .. 41]. Called for v = 0, 1, 2, ... in order, it writes every dword before
// it ORs into it (the word that reaches a dword first assigns it), so w needs no zero fill and, unrolled, every dword
// is a value of its own that lives from its first word to its store.
KP_PACK_FN void kp_narrow_put(int v, uint32_t h21, uint32_t *w) {
    const int j = kp_narrow_word(v), sh = kp_narrow_shift(v);
    if (sh == 0) w[j] = h21;
    else w[j] |= h21 << sh;
    if (kp_narrow_straddles(v)) w[j + 1] = h21 >> (32 - sh);
}

// The high dword of value v from the stream's dwords w0 = w[kp_narrow_word(v)] and w1 = w[kp_narrow_word(v) + 1]
// (w1 is not looked at unless kp_narrow_straddles(v): pass anything). Every shift is a constant in 1 .. 31 once v is.
KP_PACK_FN uint32_t kp_narrow_unpack(int v, uint32_t w0, uint32_t w1, uint32_t base) {
    const int sh = kp_narrow_shift(v);
    uint32_t h;
    if (!kp_narrow_straddles(v)) h = w0 >> sh;  // sh = 0 .. 11
    else h = (uint32_t) (((((uint64_t) w1) << 32) | w0) >> sh);  // sh = 12 .. 31
    return (h & KP_NARROW_MASK) + base;
}

// Record layout of a narrow tile: [group][thread][16 B] like the other forms, the last group [thread][8 B]. The groups
// come in the order the epilogue consumes the rows: row k needs L_k and the stream up to dword (84 k + 83) / 32, that
// is the H groups up to kp_narrow_hi_need(k):
//   L0 H0 L1 H1 L2 L3 H2 L4 H3 L5 L6 H4 L7 H5 L8 L9 H6 L10 H7 L11 L12 H8 L13 H9 L14 L15 H10
// 26 x 4 096 + 2 048 = 108 544 B per tile, against 112 KiB (7-byte form) and 128 KiB (raw).
KP_PACK_FN constexpr int kp_narrow_hi_need(int k) { return (4 * KP_NARROW_BITS * k + 4 * KP_NARROW_BITS - 1) >> 7; }  // last H group of row k
KP_PACK_FN constexpr int kp_narrow_hi_row(int h) { return (128 * h) / (4 * KP_NARROW_BITS); }  // first row that needs H_h
KP_PACK_FN constexpr int kp_narrow_lo_group(int k) { return k + (k == 0 ? 0 : kp_narrow_hi_need(k - 1) + 1); }
KP_PACK_FN constexpr int kp_narrow_hi_group(int h) { return h + kp_narrow_hi_row(h) + 1; }
// H groups whose dwords are all written once rows 0 .. k are appended (the fill stores a group as soon as it is complete)
KP_PACK_FN constexpr int kp_narrow_hi_done(int k) {
    return k == 15 ? KP_NARROW_HGROUPS : (4 * KP_NARROW_BITS * (k + 1)) >> 7;
}
// dword offset of thread t's part of record group g, from the record's start (256 threads)
KP_PACK_FN constexpr int kp_narrow_group_dword(int g, int t) { return g * 1024 + (g == KP_NARROW_GROUPS - 1 ? 2 : 4) * t; }
constexpr int KP_NARROW_BYTES = 26 * 4096 + 2048;

}  // namespace plssvm_mi
