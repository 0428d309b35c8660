// Implicit pairwise K·p tiles on MFMA (gfx950) — the dense hot kernel.
//
// Replaces device_kernel_{linear,poly,radial} (include/plssvm/backends/HIP/svm_kernel.hip.hpp:36-268)
// and its OpenMP twin (src/plssvm/backends/OpenMP/svm_kernel.cpp:21-47). Per 128x128 lower-triangle
// tile (I >= J) of k(x_i, x_j):
//   * X is feature-major in HBM (XT[k][i]); each BK-deep K chunk of the two 128-column panels is
//     streamed global -> LDS with buffer_load_dwordx4 ... lds (1 KiB per wave-instruction, no VGPR
//     staging; scalar descriptor base + constant per-lane offset, so no VALU address math in the K
//     loop), double-buffered so chunk kc+1 lands while chunk kc feeds the MFMAs: one barrier per
//     chunk;
//   * 4 waves as 2x2, each a 64x64 sub-tile = 4x4 accumulators of v_mfma_f64_16x16x4_f64 /
//     v_mfma_f32_16x16x4_f32 (exact fma chains in k order);
//   * epilogue in registers: kernel function (RBF via ||a||^2 + ||b||^2 - 2 a.b, clamped at 0),
//     times p_j -> row sums (16-lane shuffles) and times p_i -> mirrored column sums (cross-half
//     shuffles); results go to the tile's own 256-value record of the rank's slab (row sums, then
//     column sums: the slab holds only this rank's tiles, so it shrinks with the group) — no atomics,
//     so a fixed-order second pass makes K·p bitwise reproducible;
//   * tiles are visited in 8x8 super-blocks (16 panels = 4 MiB in fp64: one XCD's L2) and the
//     workgroup ids are remapped so each XCD walks a contiguous range of super-blocks.
#include <cstdlib>

#include "kernels.hpp"
#include "kp_device.hpp"
#include "kp_record.hpp"

namespace plssvm_mi {

namespace {

// occupancy: 3 workgroups per CU (<= 49 KB LDS, <= 168 VGPRs) hide the chunk barriers / DMA waits
// best; the fp64 RBF variant spills a few epilogue values at that budget (outside the K loop), and
// still runs as fast as with 2 workgroups and 16-deep chunks
// The fp64 Laplacian instances run 2 per CU: the VALU K loop keeps the 128 accumulator registers plus one feature's 16
// row and 4 column values (40 registers) and the next feature's reads in flight, which does not fit 168 VGPRs; the loop
// is VALU-issue-bound, so two waves per SIMD are enough to cover the LDS reads and the chunk barrier. fp32 fits 3.
template <typename T, int KERNEL>
constexpr int kp_waves_per_eu() { return (KERNEL == KF_LAPLACIAN && sizeof(T) == 8) ? 2 : 3; }

// fp64 RBF: chunk kc+1's DMA is issued after chunk kc's LDS reads; every other instance: right after the barrier.
// Same box, round 6 (profiles/r06_kp_dma_order_ab.json): config 2 (fp64 RBF) 39.51 / 39.58 ms against 39.62 / 39.67 ms
// with the DMA first; fp64 linear 37.18 / 37.23 against 36.67 / 36.67 ms, fp64 poly 38.72 / 38.76 against 38.58 /
// 38.58 ms, configs[3] (fp32 linear) 1 913 against 1 782 ms. KP_DMA_AFTER_READS=0 / 1 forces one order (A/B only)
#ifndef KP_DMA_AFTER_READS
#define KP_DMA_AFTER_READS 2
#endif
template <typename T, int KERNEL>
constexpr bool kp_dma_after_reads() {
    if (KERNEL == KF_LAPLACIAN) return true;  // behind the chunk's last LDS reads (its K loop reads feature by feature)
    return KP_DMA_AFTER_READS == 2 ? (sizeof(T) == 8 && KERNEL == 2) : KP_DMA_AFTER_READS == 1;
}

// KP_LOAD streams a tile's stored kernel values instead of forming them: no K loop, LDS = the reduction buffers
// only. Workgroups per CU (= waves per SIMD): KP_LOAD_WAVES, default 3 in fp64 (128 of <= 168 VGPRs hold the
// tile's values: 3 x 128 KiB of loads in flight per CU) and 4 in fp32; A/B in DESIGN.md §3.1.2
#ifndef KP_LOAD_WAVES
#define KP_LOAD_WAVES 0
#endif
// The multi-vector KP_LOAD keeps the whole record live across the loop over vectors: in fp64 that does not fit 168
// VGPRs (22 spilled dwords, three of them record chunks whose spill stores wait for their loads right after issue,
// which serialises the head of the stream), so it runs 2 workgroups per CU with 256 VGPRs; KP_MULTI_LOAD_WAVES=3
// builds the 3-per-CU variant (A/B in DESIGN.md §3.1.3). (kp_load_f64 decodes the record once and needs 166 VGPRs:
// at 3 per CU it no longer spills, and measured faster for 4 and 8 vectors but slower for 1 and 2, §3.1.2.)
#ifndef KP_MULTI_LOAD_WAVES
#define KP_MULTI_LOAD_WAVES 2
#endif
template <typename T, int KERNEL, int MODE, bool MULTI = false>
constexpr int kp_mode_waves() {
    if (MULTI && MODE == KP_LOAD && sizeof(T) == 8) return KP_MULTI_LOAD_WAVES;
    if (MODE != KP_LOAD) return kp_waves_per_eu<T, KERNEL>();
    return KP_LOAD_WAVES > 0 ? KP_LOAD_WAVES : (sizeof(T) == 8 ? 3 : 4);
}

template <typename T>
struct kp_vec;
template <>
struct kp_vec<double> {
    typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct kp_vec<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};

// The fp64 record loads carry the non-temporal hint: a record is read again only after the rest of the cache (tens
// of GB) has gone by, so nothing of it is worth keeping in a cache. -DKP_LOAD_NT=0 builds plain loads (A/B in
// every run with the hint beat every run without)
#ifndef KP_LOAD_NT
#define KP_LOAD_NT 1
#endif
// The slab is written once by the tile kernels and read once by kp_reduce_share_kernel: the tile kernels' slab stores
// and the reduce's slab loads carry the non-temporal hint as well. -DKP_SLAB_NT=0 builds both plain (A/B in DESIGN.md
// §3.1.2: the slab pass takes 107 us with the hint and 155 us without)
#ifndef KP_SLAB_NT
#define KP_SLAB_NT 1
#endif
template <typename T>
__device__ __forceinline__ void kp_slab_store(T *at, T v) {
    if constexpr (KP_SLAB_NT != 0) __builtin_nontemporal_store(v, at);
    else *at = v;
}

// LDS layout of the epilogue's reduction buffers (element counts): p_I, p_J, n_I, n_J, then row partials
// [wc][128 rows][16 (+1 pad)] and column partials [wr][128 cols][4 (+1 pad)]
constexpr int KP_OFF_PAN = 4 * KP_TILE;
constexpr int KP_RSTR = 17, KP_RHALF = KP_TILE * KP_RSTR + 1, KP_CSTR = 5;

// The fp64 KP_LOAD workgroup: the tile's record -> registers -> the "times p" epilogue of kp_tile_kernel (the same
// fma chains, LDS park and fixed-order sums, so the slab record is bitwise the computed one). FORM: KP_FORM_WIDE and
// KP_FORM_NARROW, the record is a packed one of kp_record.hpp with 24-bit or 21-bit fields — 28 dwordx4 per lane, or
// 26 and one dwordx2, instead of 32, each value's high dword rebuilt from its field of the lane's bit stream and the
// tile's base just before its fma. All of the lane's loads are issued before the first use: the whole record (106, 112
// or 128 KiB) is in flight. MULTI: the values are decoded once, then multiplied with every live vector as in
// kp_tile_kernel's MULTI epilogue.
constexpr int KP_FORM_RAW = 0, KP_FORM_WIDE = 1, KP_FORM_NARROW = 2;
template <int FORM, bool MULTI>
__device__ __forceinline__ void kp_load_f64(const double *__restrict__ kcache, int64_t wg, uint32_t base,
                                            const double *__restrict__ p, double *__restrict__ partial, double *smem,
                                            int tid, int lane, int wr, int wc, bool diag, int64_t pidx, unsigned live,
                                            int64_t pstride, int64_t sstride) {
    using M = mfma16<double>;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    // this lane's element of p (MULTI: of the first live vector), ahead of the record: loads return in order, and the
    // staging barrier below must not wait for the record
    int c = MULTI ? __builtin_ctz(live) : 0;
    double pnext = p[MULTI ? c * pstride + pidx : pidx];
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    constexpr bool PACKED = FORM != KP_FORM_RAW;
    using R = kp_record<FORM == KP_FORM_NARROW ? KP_BITS_NARROW : KP_BITS_WIDE>;
    constexpr int HFULL = R::HDW / 4;  // dwordx4 groups of the bit stream; a rest of two dwords is the dwordx2 tail
    f64x2 kld[PACKED ? 1 : 32];
    u32x4 kl[PACKED ? 16 : 1], kh[PACKED ? HFULL : 1];  // L0 .. L15, the full H groups
    u32x2 kht = { 0u, 0u };
    if constexpr (PACKED) {
        // record order: L_k, then the H group that row k is the first to need (at most one: hi_row grows)
        const uint32_t *rec = reinterpret_cast<const uint32_t *>(kcache + wg * KP_CACHE_REC);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const u32x4 *lo = reinterpret_cast<const u32x4 *>(rec + R::group_dword(R::lo_group(k), tid));
            kl[k] = KP_LOAD_NT ? __builtin_nontemporal_load(lo) : *lo;
            if constexpr (!MULTI) __builtin_amdgcn_sched_barrier(0);  // issued in record order: they return in order
#pragma unroll
            for (int h = 0; h < R::HGROUPS; ++h) {
                if (R::hi_row(h) != k) continue;
                const uint32_t *hi = rec + R::group_dword(R::hi_group(h), tid);
                const u32x4 *hi4 = reinterpret_cast<const u32x4 *>(hi);
                const u32x2 *hi2 = reinterpret_cast<const u32x2 *>(hi);
                if (h < HFULL) kh[h] = KP_LOAD_NT ? __builtin_nontemporal_load(hi4) : *hi4;
                else kht = KP_LOAD_NT ? __builtin_nontemporal_load(hi2) : *hi2;
                if constexpr (!MULTI) __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        const f64x2 *rec = reinterpret_cast<const f64x2 *>(kcache + wg * KP_CACHE_REC) + tid;
#pragma unroll
        for (int g = 0; g < 32; ++g) {
            kld[g] = KP_LOAD_NT ? __builtin_nontemporal_load(rec + g * 256) : rec[g * 256];
            if constexpr (!MULTI) __builtin_amdgcn_sched_barrier(0);
        }
    }
    // single vector: nothing of the epilogue moves up between the loads (a use there waits for its load with the rest
    // unissued), and below one row ends before the next begins, so the waits follow the record's groups as they arrive
    // (left to itself the scheduler gathers the integer decode of all rows behind the first LDS read: vmcnt(1) at once)
    if constexpr (!MULTI) __builtin_amdgcn_sched_barrier(0);
    // value nt of row (mt, r); every index is a constant once the loops are unrolled
    auto kword = [&](int j) -> uint32_t { return j < 4 * HFULL ? kh[j >> 2][j & 3] : kht[j & 1]; };  // dword j of the bit stream
    auto kval = [&](int mt, int r, int nt) -> double {
        if constexpr (PACKED) {
            const int v = (mt * 4 + r) * 4 + nt, j = R::word(v);
            const uint32_t hi = R::unpack(v, kword(j), kword(R::straddles(v) ? j + 1 : j), base);
            return __hiloint2double((int) hi, (int) kl[mt * 4 + r][nt]);
        } else {
            return kld[((mt * 4 + r) * 4 + nt) / 2][nt & 1];
        }
    };
    const double *pI = smem, *pJ = smem + KP_TILE;
    double *rowp = smem + KP_OFF_PAN + wc * KP_RHALF;
    const int q = tid >> 1, h = tid & 1;  // row / column q of the tile, half h
    if constexpr (!MULTI) {
        smem[tid] = pnext;
        __syncthreads();  // p_I, p_J visible
        double pj[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) pj[nt] = pJ[wc * 64 + nt * 16 + (lane & 15)];
        double cs[4] = { 0, 0, 0, 0 };
        double pi = pI[wr * 64 + M::row(lane, 0)];  // one row ahead: its LDS latency lies under the row before
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = wr * 64 + mt * 16 + M::row(lane, r);
                const int rn = mt * 4 + r + 1;  // the next row
                const double pin = rn < 16 ? pI[wr * 64 + (rn >> 2) * 16 + M::row(lane, rn & 3)] : 0.0;
                double s = 0;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const double kv = kval(mt, r, nt);
                    s = fma(kv, pj[nt], s);
                    cs[nt] = fma(kv, pi, cs[nt]);
                }
                rowp[il * KP_RSTR + (lane & 15)] = s;
                pi = pin;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        {  // also on a diagonal tile, whose column sums nobody reads: a store under `if (!diag)` lets the compiler sink
           // the cs chains into that branch, away from the just-decoded values
            double *colp = smem + KP_OFF_PAN + 2 * KP_RHALF + wr * KP_TILE * KP_CSTR;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) colp[(wc * 64 + nt * 16 + (lane & 15)) * KP_CSTR + (lane >> 4)] = cs[nt];
        }
        __syncthreads();
        const double *rp = smem + KP_OFF_PAN + h * KP_RHALF + q * KP_RSTR;
        double a = rp[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) a += rp[k];
        a += __shfl_xor(a, 1);
        if (!diag) {
            const double *cp = smem + KP_OFF_PAN + 2 * KP_RHALF + (h * KP_TILE + q) * KP_CSTR;
            double c = (cp[0] + cp[1]) + (cp[2] + cp[3]);
            c += __shfl_xor(c, 1);
            if (h == 1) kp_slab_store(partial + wg * KP_REC + KP_TILE + q, c);  // column sums of the J rows
        }
        if (h == 0) kp_slab_store(partial + wg * KP_REC + q, a);  // row sums of the I rows
    } else {
        double kv[16][4];  // decoded once; the record's registers die here
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) kv[mt * 4 + r][nt] = kval(mt, r, nt);
        while (true) {  // the next live vector's element is fetched while this one is multiplied
            smem[tid] = pnext;  // the previous turn's reads of p_I / p_J lie before its second barrier
            __syncthreads();    // p_c visible; every wave is done with the previous turn's sums
            const unsigned rest = live >> (c + 1);
            const int cn = rest != 0 ? c + 1 + __builtin_ctz(rest) : -1;
            if (cn >= 0) pnext = p[cn * pstride + pidx];
            double pj[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) pj[nt] = pJ[wc * 64 + nt * 16 + (lane & 15)];
            double cs[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int il = wr * 64 + mt * 16 + M::row(lane, r);
                    const double pi = pI[il];
                    double s = 0;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        s = fma(kv[mt * 4 + r][nt], pj[nt], s);
                        cs[nt] = fma(kv[mt * 4 + r][nt], pi, cs[nt]);
                    }
                    rowp[il * KP_RSTR + (lane & 15)] = s;
                }
            }
            {
                double *colp = smem + KP_OFF_PAN + 2 * KP_RHALF + wr * KP_TILE * KP_CSTR;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) colp[(wc * 64 + nt * 16 + (lane & 15)) * KP_CSTR + (lane >> 4)] = cs[nt];
            }
            __syncthreads();
            double *slab = partial + c * sstride;
            const double *rp = smem + KP_OFF_PAN + h * KP_RHALF + q * KP_RSTR;
            double a = rp[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) a += rp[k];
            a += __shfl_xor(a, 1);
            if (!diag) {
                const double *cp = smem + KP_OFF_PAN + 2 * KP_RHALF + (h * KP_TILE + q) * KP_CSTR;
                double cc = (cp[0] + cp[1]) + (cp[2] + cp[3]);
                cc += __shfl_xor(cc, 1);
                if (h == 1) kp_slab_store(slab + wg * KP_REC + KP_TILE + q, cc);  // column sums of the J rows
            }
            if (h == 0) kp_slab_store(slab + wg * KP_REC + q, a);  // row sums of the I rows
            if (cn < 0) break;
            c = cn;
        }
    }
}

// The fill's store of row `row` (0 .. 15, a constant once unrolled, and with it every position below) of a lane's packed
// record at rec: L_row, the row's four fields appended to the lane's bit stream w (carried across the rows; unrolled,
// every dword is a value of its own that lives from the first field that reaches it to the store of its group), and
// the H groups this row completed.
template <int BITS, typename T>
__device__ __forceinline__ void kp_store_row(uint32_t *rec, int tid, int row, const T *kv, uint32_t base, uint32_t *w) {
    using R = kp_record<BITS>;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x4 lo;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        lo[nt] = (uint32_t) __double2loint((double) kv[nt]);
        R::put(row * 4 + nt, (uint32_t) __double2hiint((double) kv[nt]) - base, w);
    }
    *reinterpret_cast<u32x4 *>(rec + R::group_dword(R::lo_group(row), tid)) = lo;
#pragma unroll
    for (int h = 0; h < R::HGROUPS; ++h) {
        if (h >= R::hi_done(row) || (row > 0 && h < R::hi_done(row - 1))) continue;
        uint32_t *at = rec + R::group_dword(R::hi_group(h), tid);
        if (h < R::HDW / 4) *reinterpret_cast<u32x4 *>(at) = u32x4{ w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3] };
        else *reinterpret_cast<u32x2 *>(at) = u32x2{ w[4 * h], w[4 * h + 1] };
    }
}

// MODE (kernels.hpp): KP_COMPUTE forms the tile's kernel values from the data; KP_COMPUTE_STORE also writes them
// to the tile's cache record kcache[wg]; KP_LOAD reads them from there and runs the same epilogue from "times p_j"
// on — the same fma order, LDS park and sums, so the slab record is bitwise the computed one. A cache record is
// in register layout, [value group][thread][VEC]: a lane's 64 values in (mt, r, nt) order, 16 bytes per lane and
// group, so every wave-instruction moves one contiguous KiB. wg_base: the first workgroup (tile) of this launch.
// fp64 records come raw or in one of the two packed forms of kp_record.hpp (wide: 7 bytes per value, narrow: 53 bits),
// per tile (kdesc[wg]: 0 = raw, the tile's largest exponent E = wide, E | KP_DESC_NARROW = narrow): the fp64 KP_COMPUTE_STORE instance
// finds the tile's exponent range, writes the descriptor, counts the packed tiles of both forms in kcount[0] and the
// narrow ones in kcount[1] (pack = 0: every tile raw, 1: no narrow tile) and stores the form; the fp64 KP_LOAD
// instance is kp_load_f64 above, so the KP_LOAD statements in this body serve fp32 only. fp32 records are always raw.
//
// MULTI: nvec (<= KP_MULTI_W) vectors per visit of a tile (the single-vector instances ignore nvec and the
// strides). Vector c is p + c * pstride, its slab partial + c * sstride, its stop flag status[c]. The tile's kernel
// values are formed (or loaded) once and stay in the accumulator registers; the "times p" epilogue then runs once per
// vector with that vector's p_I / p_J staged in LDS, in the single-vector kernel's fma, park and summation order:
// slab c is bitwise the slab the single-vector kernel writes for p_c. A vector whose flag says converged is skipped
// (its slab is left alone). Every MULTI statement sits in an `if constexpr`, and the MULTI epilogue is written out
// beside the single one instead of sharing a helper with it: the single-vector instances must keep their registers,
// scratch and LDS (a shared body or lambda moved them).
template <typename T, int KERNEL, int MODE, bool MULTI = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kp_mode_waves<T, KERNEL, MODE, MULTI>(), kp_mode_waves<T, KERNEL, MODE, MULTI>()))) void kp_tile_kernel(kfun<T> kf, const T *__restrict__ XT,
                                                         const T *__restrict__ norms, const T *__restrict__ p,
                                                         T *__restrict__ partial, int64_t n_pad, int64_t d_pad,
                                                         int64_t nb, int64_t s0, int64_t nsuper,
                                                         const int32_t *__restrict__ wg_off,
                                                         const cg_scalars<T> *__restrict__ status, int64_t wg_base,
                                                         T *__restrict__ kcache, int nvec, int64_t pstride,
                                                         int64_t sstride, int32_t *__restrict__ kdesc,
                                                         int32_t *__restrict__ kcount, int pack) {
    static_assert(!MULTI || MODE != KP_COMPUTE_STORE, "the tile cache is filled by the single-vector kernel");
    using M = mfma16<T>;
    using acc_t = typename M::acc_t;
    using vec_t = typename kp_vec<T>::type;
    constexpr int BK = kp_bk<T, KERNEL>();
    constexpr int PANEL = BK * KP_TILE;            // elements of one [BK][128] panel
    constexpr int EPP = 1024 / (int) sizeof(T);    // elements per 1 KiB wave-instruction
    constexpr int PIECES = PANEL / EPP / 4;        // wave-instructions per wave per panel
    constexpr int VEC = 16 / (int) sizeof(T);
    // LDS: p_I, p_J, n_I, n_J, then the two double-buffered panel pairs; once the K loop is done the
    // epilogue's reduction buffers overlay the panels: row partials [wc][128 rows][16 (+1 pad)],
    // column partials [wr][128 cols][4 (+1 pad)]
    constexpr int OFF_PAN = KP_OFF_PAN;
    constexpr int RSTR = KP_RSTR, RHALF = KP_RHALF, CSTR = KP_CSTR;
    constexpr int RED = 2 * RHALF + 2 * KP_TILE * CSTR;
    constexpr int SMEM = OFF_PAN + ((MODE != KP_LOAD && 4 * PANEL > RED) ? 4 * PANEL : RED);
    __shared__ __attribute__((aligned(16))) T smem[SMEM];
    constexpr bool FAST_EXP = (KERNEL == 2) && sizeof(T) == 8 && MODE != KP_LOAD;
    constexpr int NGRP = 64 / VEC;  // 16-byte groups of a lane's 64 values
    __shared__ double exp_tab[FAST_EXP ? EXP_TAB : 1];

    unsigned live = 1;  // MULTI: bit c = vector c is still iterating
    if constexpr (MULTI) {
        live = 0;
        for (int c = 0; c < nvec; ++c)
            if (status == nullptr || !status[c].converged) live |= 1u << c;
        if (live == 0) return;
    } else {
        if (status != nullptr && status->converged) return;
    }

    // workgroups: one per real tile. wg_off[k] = first workgroup of the rank's super-block s0 + k (a full
    // super-block has 64 tiles, a diagonal one 36, the ragged last super-block row fewer): no empty
    // workgroups, so the XCDs' contiguous ranges carry equal work (empty ones bunched at the end of a
    // range made the last rank of 8 3.9 % slower than the others)
    // (KP_LOAD has no panels to keep in an L2: its workgroups walk the records in order)
    const int64_t wg = wg_base + (MODE == KP_LOAD ? (int64_t) blockIdx.x : xcd_remap(blockIdx.x, gridDim.x));
    // fp64 records may be in a packed form (kp_record.hpp): the tile's descriptor, one wave-uniform load issued
    // ahead of the table search below so that its latency hides there
    constexpr bool PACK_LOAD = MODE == KP_LOAD && sizeof(T) == 8, PACK_STORE = MODE == KP_COMPUTE_STORE && sizeof(T) == 8;
    uint32_t desc = KP_DESC_RAW;
    if constexpr (PACK_LOAD) desc = (uint32_t) kdesc[wg];
    int lo = 0, hi = (int) nsuper;  // largest k with wg_off[k] <= wg
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t) wg_off[mid] <= wg) lo = mid;
        else hi = mid;
    }
    const int64_t sb = s0 + lo, local = wg - wg_off[lo];
    int64_t SI, SJ;
    tri_tile(sb, SI, SJ);
    int64_t ta, tb;  // tile row / column inside the super-block
    if (SI == SJ) {
        tri_tile(local, ta, tb);  // lower triangle, tb <= ta
    } else {
        const int64_t cols = min<int64_t>(KP_SUPER, nb - SJ * KP_SUPER);
        ta = local / cols;
        tb = local % cols;
    }
    const int64_t I = SI * KP_SUPER + ta, J = SJ * KP_SUPER + tb;
    if (I >= nb || J > I) return;  // uniform per workgroup
    const int64_t I0 = I * KP_TILE, J0 = J * KP_TILE;
    const bool diag = (I == J);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform, provably (scalar LDS bases)
    const int wr = w >> 1, wc = w & 1;

    const int64_t pidx = (tid < KP_TILE) ? I0 + tid : J0 + (tid - KP_TILE);
    if constexpr (PACK_LOAD) {
        if (kp_desc_is_narrow(desc))
            kp_load_f64<KP_FORM_NARROW, MULTI>(kcache, wg, kp_record<KP_BITS_NARROW>::base(kp_desc_exp(desc)), p, partial, smem, tid,
                                               lane, wr, wc, diag, pidx, live, pstride, sstride);
        else if (desc != KP_DESC_RAW)
            kp_load_f64<KP_FORM_WIDE, MULTI>(kcache, wg, kp_record<KP_BITS_WIDE>::base(desc), p, partial, smem, tid, lane, wr, wc, diag,
                                             pidx, live, pstride, sstride);
        else
            kp_load_f64<KP_FORM_RAW, MULTI>(kcache, wg, 0u, p, partial, smem, tid, lane, wr, wc, diag, pidx, live, pstride,
                                            sstride);
        return;
    }
    acc_t acc[4][4];
    vec_t kld[MODE == KP_LOAD ? NGRP : 1];
    if constexpr (MODE == KP_LOAD) {
        // all of the lane's loads are issued before the first use: the whole 128 KiB (fp64) record is in flight
        const vec_t *rec = reinterpret_cast<const vec_t *>(kcache + wg * KP_CACHE_REC) + tid;
#pragma unroll
        for (int g = 0; g < NGRP; ++g) kld[g] = rec[g * 256];
        if constexpr (!MULTI) {
            smem[tid] = p[pidx];
            __syncthreads();  // p_I, p_J visible
        }
    } else {
        // p and norms of the tile's rows/cols -> LDS (issued first: their wait must not drain the DMA)
        const T pin = MULTI ? T(0) : p[pidx];  // MULTI stages each vector's p after the K loop
        const T nin = (KERNEL == 2) ? norms[pidx] : T(0);
        // fast fp64 RBF: the accumulators start at -n_j / 2 (column j = lane & 15 of every block), so they
        // end at g_ij - n_j / 2 and y_ij = 2 g KEXP (g_ij - n_j / 2) - g KEXP n_i is one fma per element
        T acc0[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            acc0[nt] = FAST_EXP ? T(-0.5) * norms[J0 + wc * 64 + nt * 16 + (lane & 15)] : T(0);

        // per-lane byte offsets of this wave's DMA pieces inside a chunk (32-bit, reused for every chunk
        // and both panels: the chunk base and the panel offset are wave-uniform, see glds16_buf)
        uint32_t doff[PIECES];
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int elem = (w * PIECES + j) * EPP + lane * VEC;
            doff[j] = (uint32_t) (((int64_t) (elem / KP_TILE) * n_pad + elem % KP_TILE) * (int64_t) sizeof(T));
        }
        // LDS-DMA through a buffer descriptor: the chunk base is a scalar pointer (SALU), the per-lane part
        // is the constant doff and the panel offset goes in soffset — no VALU address math per chunk
        const uint32_t offI = __builtin_amdgcn_readfirstlane((uint32_t) (I0 * (int64_t) sizeof(T)));
        const uint32_t offJ = __builtin_amdgcn_readfirstlane((uint32_t) (J0 * (int64_t) sizeof(T)));
        auto issue = [&](int64_t kc, int buf) {
            const T *cb = XT + kc * BK * n_pad;
            T *pa = smem + OFF_PAN + (2 * buf) * PANEL;
            T *pb = pa + PANEL;
#pragma unroll
            for (int j = 0; j < PIECES; ++j) {
                const int u = w * PIECES + j;
                glds16_buf(cb, pa + u * EPP, doff[j], offI);
                glds16_buf(cb, pb + u * EPP, doff[j], offJ);
            }
        };

#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = acc_t{ acc0[b], acc0[b], acc0[b], acc0[b] };

        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (!MULTI) smem[tid] = pin;
        smem[2 * KP_TILE + tid] = nin;
        if constexpr (FAST_EXP) {
            if (tid < EXP_TAB) exp_tab[tid] = c_exp2_256[tid];  // visible after the first K-loop barrier
        }

        const int64_t nk = d_pad / BK;
        for (int64_t kc = 0; kc < nk; ++kc) {
            if (kc > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // chunk kc visible to all waves; every wave is done reading chunk kc-1
            if (!kp_dma_after_reads<T, KERNEL>() && kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1));
            const T *A = smem + OFF_PAN + (2 * (kc & 1)) * PANEL;
            const T *B = A + PANEL;
            if constexpr (KERNEL == KF_LAPLACIAN) {
                // no MFMA form: L1_CHUNK (kp_device.hpp), feature by feature in ascending k. Chunk kc+1's DMA goes
                // out behind the chunk's last LDS reads, under the last feature's 128 VALU operations (an LDS read issued
                // after the DMA would wait for it, see below)
                L1_CHUNK(T, BK, A, B, wr, wc, lane, acc, if (kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1)));
            } else {
                // fp64 RBF: the whole chunk's operands come out of LDS before chunk kc+1's DMA is issued — the compiler cannot
                // tell the DMA's LDS target from the buffer being read, so an LDS read issued after the DMA waits for it
                // (vmcnt(0)) and the prefetch sits on each wave's critical path instead of under its MFMAs (the other instances
                // measured faster with the DMA first, see kp_dma_after_reads)
                T a[BK / 4][4], b[BK / 4][4];
#pragma unroll
                for (int ks = 0; ks < BK / 4; ++ks) {
                    const int kr = ks * 4 + (lane >> 4);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) a[ks][mt] = A[kr * KP_TILE + wr * 64 + mt * 16 + (lane & 15)];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) b[ks][nt] = B[kr * KP_TILE + wc * 64 + nt * 16 + (lane & 15)];
                }
                if (kp_dma_after_reads<T, KERNEL>() && kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1));
#pragma unroll
                for (int ks = 0; ks < BK / 4; ++ks)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = M::op(a[ks][mt], b[ks][nt], acc[mt][nt]);
            }
        }
    }

    // ---- epilogue: kernel function, times p, row and column partial sums ----
    if constexpr (!MULTI) {
        const T *pI = smem, *pJ = smem + KP_TILE, *nI = smem + 2 * KP_TILE, *nJ = smem + 3 * KP_TILE;
        T pj[4], nj[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int jl = wc * 64 + nt * 16 + (lane & 15);
            pj[nt] = pJ[jl];
            nj[nt] = (KERNEL == 2 && !FAST_EXP) ? nJ[jl] : T(0);
        }
        T cs[4] = { 0, 0, 0, 0 };
        const T c2 = FAST_EXP ? T(2) * kf.gamma * T(KEXP) : T(0);
        // Each row has 32 partials (16 lanes x 2 column-half waves), each column 8 (4 lane groups x 2
        // row-half waves). They are parked in LDS and every thread then sums one half-row and one
        // half-column: ~20 adds per lane instead of a 4-level shuffle tree per row (64 adds + 128
        // ds_bpermute); the fixed summation order keeps K·p bitwise reproducible.
        uint32_t pk_desc = KP_DESC_RAW;  // fp64 KP_COMPUTE_STORE: the tile's descriptor, uniform in the workgroup
        if constexpr (PACK_STORE) {
            // The kernel function once, in place (the call and its arguments are those of the loop below, as in the
            // MULTI branch: the values are bitwise the same), tracking the range of the lane's high dwords; the four
            // waves' ranges meet in LDS behind the barrier that ends the K loop anyway.
            __shared__ uint32_t pk_red[8];
            uint32_t mn = KP_PACK_MN0, mx = KP_PACK_MX0;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const T ni = nI[wr * 64 + mt * 16 + M::row(lane, r)];
                    const T ai = FAST_EXP ? -kf.gamma * T(KEXP) * ni : T(0);
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        if constexpr (FAST_EXP)
                            acc[mt][nt][r] = (T) exp_scaled_f64(fma(c2, acc[mt][nt][r], ai), exp_tab);
                        else
                            acc[mt][nt][r] = kernel_apply<T>(KERNEL, kf.degree, kf.gamma, kf.coef0, acc[mt][nt][r], ni, nj[nt]);
                        kp_pack_track((uint32_t) __double2hiint((double) acc[mt][nt][r]), mn, mx);
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                mn = min(mn, (uint32_t) __shfl_xor((int) mn, o));
                mx = max(mx, (uint32_t) __shfl_xor((int) mx, o));
            }
            if (lane == 0) {
                pk_red[2 * w] = mn;
                pk_red[2 * w + 1] = mx;
            }
            __syncthreads();  // every wave is done with the last K chunk: the panels become reduction buffers
            mn = min(min(pk_red[0], pk_red[2]), min(pk_red[4], pk_red[6]));
            mx = max(max(pk_red[1], pk_red[3]), max(pk_red[5], pk_red[7]));
            pk_desc = __builtin_amdgcn_readfirstlane(kp_desc(mn, mx, pack));
            if (tid == 0) {
                kdesc[wg] = (int32_t) pk_desc;
                if (pk_desc != KP_DESC_RAW) atomicAdd(kcount, 1);            // one per packed tile, either form
                if (kp_desc_is_narrow(pk_desc)) atomicAdd(kcount + 1, 1);  // one per narrow tile
            }
        } else {
            __syncthreads();  // every wave is done with the last K chunk: the panels become reduction buffers
        }
        const bool pk_narrow = kp_desc_is_narrow(pk_desc);  // uniform
        const uint32_t pk_base = pk_narrow ? kp_record<KP_BITS_NARROW>::base(kp_desc_exp(pk_desc)) : kp_record<KP_BITS_WIDE>::base(pk_desc);
        uint32_t pk_w[PACK_STORE ? kp_record<KP_BITS_WIDE>::HDW : 1];  // the lane's bit stream of either width (kp_store_row)
        T *rowp = smem + OFF_PAN + wc * RHALF;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = wr * 64 + mt * 16 + M::row(lane, r);
                const T pi = pI[il];
                const T ni = MODE == KP_LOAD ? T(0) : nI[il];
                const T ai = FAST_EXP ? -kf.gamma * T(KEXP) * ni : T(0);
                T s = 0;
                T kvs[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    T kv;
                    if constexpr (MODE == KP_LOAD)
                        kv = kld[((mt * 4 + r) * 4 + nt) / VEC][nt % VEC];
                    else if constexpr (PACK_STORE)
                        kv = acc[mt][nt][r];
                    else if constexpr (FAST_EXP)
                        kv = (T) exp_scaled_f64(fma(c2, acc[mt][nt][r], ai), exp_tab);
                    else
                        kv = kernel_apply<T>(KERNEL, kf.degree, kf.gamma, kf.coef0, acc[mt][nt][r], ni, nj[nt]);
                    kvs[nt] = kv;
                    s = fma(kv, pj[nt], s);
                    cs[nt] = fma(kv, pi, cs[nt]);
                }
                rowp[il * RSTR + (lane & 15)] = s;
                if constexpr (MODE == KP_COMPUTE_STORE) {
                    bool raw = true;  // uniform, like the two tests below
                    if constexpr (PACK_STORE) {
                        uint32_t *rec = reinterpret_cast<uint32_t *>(kcache + wg * KP_CACHE_REC);
                        raw = pk_desc == KP_DESC_RAW;
                        if (pk_narrow) kp_store_row<KP_BITS_NARROW>(rec, tid, mt * 4 + r, kvs, pk_base, pk_w);
                        else if (!raw) kp_store_row<KP_BITS_WIDE>(rec, tid, mt * 4 + r, kvs, pk_base, pk_w);
                    }
                    if (raw) {
                        vec_t *rec = reinterpret_cast<vec_t *>(kcache + wg * KP_CACHE_REC) + tid;
#pragma unroll
                        for (int h = 0; h < 4 / VEC; ++h) {
                            vec_t v;
#pragma unroll
                            for (int e = 0; e < VEC; ++e) v[e] = kvs[h * VEC + e];
                            rec[((mt * 4 + r) * (4 / VEC) + h) * 256] = v;
                        }
                    }
                }
            }
        }
        if (!diag) {
            T *colp = smem + OFF_PAN + 2 * RHALF + wr * KP_TILE * CSTR;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) colp[(wc * 64 + nt * 16 + (lane & 15)) * CSTR + (lane >> 4)] = cs[nt];
        }
        __syncthreads();
        const int q = tid >> 1, h = tid & 1;  // row / column q of the tile, half h
        const T *rp = smem + OFF_PAN + h * RHALF + q * RSTR;
        T a = rp[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) a += rp[k];
        a += __shfl_xor(a, 1);
        if (!diag) {
            const T *cp = smem + OFF_PAN + 2 * RHALF + (h * KP_TILE + q) * CSTR;
            T c = (cp[0] + cp[1]) + (cp[2] + cp[3]);
            c += __shfl_xor(c, 1);
            if (h == 1) kp_slab_store(partial + wg * KP_REC + KP_TILE + q, c);  // column sums of the J rows
        }
        if (h == 0) kp_slab_store(partial + wg * KP_REC + q, a);  // row sums of the I rows
    } else {
        // The same epilogue in two steps. First the kernel function, once, in place: the call and its arguments are
        // the single-vector branch's, so the values are its values (KP_LOAD: they are the record). Then one turn per
        // live vector: its p_I / p_J staged where the single-vector kernel keeps them (LDS keeps its size for any
        // nvec), its fma chains, park and sums in the order above, its record of slab c.
        const T *pI = smem, *pJ = smem + KP_TILE, *nI = smem + 2 * KP_TILE, *nJ = smem + 3 * KP_TILE;
        if constexpr (MODE != KP_LOAD) {
            T nj[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) nj[nt] = (KERNEL == 2 && !FAST_EXP) ? nJ[wc * 64 + nt * 16 + (lane & 15)] : T(0);
            const T c2 = FAST_EXP ? T(2) * kf.gamma * T(KEXP) : T(0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const T ni = nI[wr * 64 + mt * 16 + M::row(lane, r)];
                    const T ai = FAST_EXP ? -kf.gamma * T(KEXP) * ni : T(0);
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        if constexpr (FAST_EXP)
                            acc[mt][nt][r] = (T) exp_scaled_f64(fma(c2, acc[mt][nt][r], ai), exp_tab);
                        else
                            acc[mt][nt][r] = kernel_apply<T>(KERNEL, kf.degree, kf.gamma, kf.coef0, acc[mt][nt][r], ni, nj[nt]);
                    }
                }
            }
        }
        T *rowp = smem + OFF_PAN + wc * RHALF;
        const int q = tid >> 1, h = tid & 1;  // row / column q of the tile, half h
        int c = __builtin_ctz(live);
        T pnext = p[c * pstride + pidx];  // the next live vector's element is fetched while this one is multiplied
        while (true) {
            smem[tid] = pnext;  // the previous turn's reads of p_I / p_J lie before its second barrier
            __syncthreads();    // p_c visible; every wave is done with the last K chunk / the previous turn's sums
            const unsigned rest = live >> (c + 1);
            const int cn = rest != 0 ? c + 1 + __builtin_ctz(rest) : -1;
            if (cn >= 0) pnext = p[cn * pstride + pidx];
            T pj[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) pj[nt] = pJ[wc * 64 + nt * 16 + (lane & 15)];
            T cs[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int il = wr * 64 + mt * 16 + M::row(lane, r);
                    const T pi = pI[il];
                    T s = 0;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        T kv;
                        if constexpr (MODE == KP_LOAD)
                            kv = kld[((mt * 4 + r) * 4 + nt) / VEC][nt % VEC];
                        else
                            kv = acc[mt][nt][r];
                        s = fma(kv, pj[nt], s);
                        cs[nt] = fma(kv, pi, cs[nt]);
                    }
                    rowp[il * RSTR + (lane & 15)] = s;
                }
            }
            if (!diag) {
                T *colp = smem + OFF_PAN + 2 * RHALF + wr * KP_TILE * CSTR;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) colp[(wc * 64 + nt * 16 + (lane & 15)) * CSTR + (lane >> 4)] = cs[nt];
            }
            __syncthreads();
            T *slab = partial + c * sstride;
            const T *rp = smem + OFF_PAN + h * RHALF + q * RSTR;
            T a = rp[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) a += rp[k];
            a += __shfl_xor(a, 1);
            if (!diag) {
                const T *cp = smem + OFF_PAN + 2 * RHALF + (h * KP_TILE + q) * CSTR;
                T cc = (cp[0] + cp[1]) + (cp[2] + cp[3]);
                cc += __shfl_xor(cc, 1);
                if (h == 1) kp_slab_store(slab + wg * KP_REC + KP_TILE + q, cc);  // column sums of the J rows
            }
            if (h == 0) kp_slab_store(slab + wg * KP_REC + q, a);  // row sums of the I rows
            if (cn < 0) break;
            c = cn;
        }
    }
}

// raw[i] = sum of the slab values of the super-blocks [s0, s1) (a rank's share, or the whole triangle), in a fixed
// order: sixteen chains g = 0 .. 15, each from 0; chain g walks the column super-blocks CS = g, g + 16, ... in
// ascending order (skipping those outside [s0, s1)) and inside one the column blocks c = 8 CS + u, u = 0 .. cnt - 1,
// adding one value at a time — tile (Ib, c)'s row sum for c <= Ib, tile (c, Ib)'s column sum for c > Ib; then the
// chains are added in g order. That order is the interface (tests/test_gpu_kp_reduce_order.py pins it bitwise); the
// shape below only decides how fast the slab arrives:
//   * one block per row block Ib, a lane holds rows 2 lane and 2 lane + 1 of it, so one wave instruction reads a
//     whole half record (128 row sums or 128 column sums): 16 bytes per lane, 1 KiB contiguous in fp64;
//   * KP_RED_WAVES waves per block, wave w carries the chains w, w + KP_RED_WAVES, ...: with 4 waves a block is 256
//     threads and every block of the flagship's grid (782) is resident at once, so there is no last, nearly empty
//     round;
//   * a step is one super-block of one chain (8 loads); the loads of KP_RED_BATCH steps (of different chains) are
//     issued together, then their adds follow. Nothing is carried in registers from one batch to the next: a loop
//     that kept the next step's loads in flight under the adds (two buffers) spilled at 128 VGPRs in fp64.
// Every index but the lane's offset is wave-uniform. Rows past m are read (the records are whole) but not stored.
constexpr int KP_RED_G = 16;
#ifndef KP_RED_WAVES
#define KP_RED_WAVES 4
#endif
#ifndef KP_RED_BATCH
#define KP_RED_BATCH 2
#endif
static_assert(KP_RED_G % KP_RED_WAVES == 0 && KP_RED_WAVES >= 1 && KP_RED_WAVES <= KP_RED_G, "waves must divide the 16 chains");
template <typename T>
using kp_row2 = T __attribute__((ext_vector_type(2)));

// One step: the values of row block Ib in column super-block CS, i.e. the column blocks c = 8 CS + u, u < cnt. With
// t = Ib % 8 and base = the first record of the super-block holding those tiles (kp_tile_offsets' table; tiles inside
// a super-block are numbered row-major, a diagonal one: its lower triangle, ta (ta + 1) / 2 + tb):
//   * CS below the row's own super-block RS: tile (Ib, c), record base + 8 t + u, its row sums;
//   * CS above RS: tile (c, Ib), record base + 8 u + t, its column sums (both super-block columns are full ones);
//   * CS = RS, the diagonal super-block: u <= t is tile (Ib, c), record base + t (t + 1) / 2 + u, row sums; u > t is
//     tile (c, Ib), record base + u (u + 1) / 2 + t, column sums.
// Off the diagonal value u therefore sits at byte off0 + u stride of the slab (stride: one record, or eight): no
// compare between the loads. The one diagonal step of a row block picks per u between its row part (off0, stride one
// record) and its column part (col0 + u (u + 1) / 2 records). All of it is wave-uniform.
struct kp_red_step {
    int cnt;  // column blocks of the step's super-block, 0: nothing to add (not the rank's, or past the last)
    int t;    // >= 0: the diagonal step, the last u that reads row sums; -1: off the diagonal
    int64_t off0, stride, col0;  // bytes
};

// at least 4 waves per SIMD (<= 128 VGPRs): with 4-wave blocks that is at least 4 blocks per CU
template <typename T>
__global__ __launch_bounds__(64 * KP_RED_WAVES) __attribute__((amdgpu_waves_per_eu(4))) void kp_reduce_share_kernel(
    const T *__restrict__ partial, int64_t nb, int64_t m, int64_t s0, int64_t s1, const int32_t *__restrict__ wg_off,
    T *__restrict__ raw, const cg_scalars<T> *__restrict__ status) {
    if (status != nullptr && status->converged) return;
    constexpr int W = KP_RED_WAVES, CPW = KP_RED_G / W;  // chains per wave
    constexpr int B = CPW < KP_RED_BATCH ? CPW : KP_RED_BATCH;  // steps whose loads are issued together
    static_assert(CPW % B == 0, "the batch must divide the wave's chains");
    using row2 = kp_row2<T>;
    __shared__ row2 red[KP_RED_G][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int64_t Ib = blockIdx.x;
    const int64_t ns = (nb + KP_SUPER - 1) / KP_SUPER, RS = Ib / KP_SUPER;
    const int t = (int) (Ib % KP_SUPER);
    const int64_t turns = (ns + KP_RED_G - 1) / KP_RED_G;

    // the wave's chain k (g = w + W k) in turn `turn`: the chain's super-block number `turn`
    auto step = [&](int64_t turn, int k) -> kp_red_step {
        const int64_t CS = (w + W * k) + KP_RED_G * turn;
        kp_red_step st{ 0, -1, 0, 0, 0 };
        if (CS < ns) {
            const int64_t sb = (RS >= CS) ? tri_index(RS, CS) : tri_index(CS, RS);
            if (sb >= s0 && sb < s1) {
                const int64_t base = wg_off[sb - s0];
                const int64_t col0 = ((base + t) * KP_REC + KP_TILE) * (int64_t) sizeof(T);
                st.cnt = (int) min<int64_t>(KP_SUPER, nb - CS * KP_SUPER);
                st.t = CS == RS ? t : -1;
                st.off0 = CS > RS ? col0 : (base + (CS == RS ? t * (t + 1) / 2 : t * KP_SUPER)) * KP_REC * (int64_t) sizeof(T);
                st.stride = (CS > RS ? KP_SUPER : 1) * KP_REC * (int64_t) sizeof(T);
                st.col0 = col0;
            }
        }
        return st;
    };
    // A full step off the diagonal (all but a row block's one diagonal step and the ragged last super-block): eight
    // loads from one scalar base, the multiples of the stride in the lane's 32-bit offset (at most 112 KiB), nothing
    // else between them; then the eight adds.
    const char *slab = reinterpret_cast<const char *>(partial);
    const uint32_t lane_off = (uint32_t) lane * (uint32_t) sizeof(row2);
    auto full = [](const kp_red_step &st) { return st.t < 0 && st.cnt == KP_SUPER; };
    auto fetch = [&](const kp_red_step &st, row2 *v) {
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t) st.off0);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t) ((uint64_t) st.off0 >> 32));
        const uint32_t stride = __builtin_amdgcn_readfirstlane((uint32_t) st.stride);
        const char *base = slab + (((uint64_t) hi << 32) | lo);
#pragma unroll
        for (int u = 0; u < KP_SUPER; ++u) {
            const row2 *at = reinterpret_cast<const row2 *>(base + (lane_off + (uint32_t) u * stride));
            v[u] = KP_SLAB_NT ? __builtin_nontemporal_load(at) : *at;
        }
    };
    // The other steps, at most two per chain: one value at a time (a loop that is not unrolled keeps this rare path
    // out of the registers and the schedule of the one above). Nothing to do for cnt = 0.
    auto slow = [&](row2 &s, const kp_red_step &st) {
#pragma nounroll
        for (int u = 0; u < st.cnt; ++u) {
            const int64_t off = (st.t < 0 || u <= st.t) ? st.off0 + u * st.stride
                                                        : st.col0 + (int64_t) (u * (u + 1) / 2) * KP_REC * (int64_t) sizeof(T);
            const row2 *at = reinterpret_cast<const row2 *>(slab + off) + lane;
            s += KP_SLAB_NT ? __builtin_nontemporal_load(at) : *at;
        }
    };

    row2 acc[CPW];
#pragma unroll
    for (int k = 0; k < CPW; ++k) acc[k] = row2{ T(0), T(0) };
    for (int64_t turn = 0; turn < turns; ++turn) {
#pragma unroll
        for (int k0 = 0; k0 < CPW; k0 += B) {  // unrolled: the chains k0 + b are constants
            kp_red_step st[B];
            row2 v[B][KP_SUPER];
#pragma unroll
            for (int b = 0; b < B; ++b) st[b] = step(turn, k0 + b);
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (full(st[b])) fetch(st[b], v[b]);
#pragma unroll
            for (int b = 0; b < B; ++b) {  // both rows of the lane: one add each per value, in u order
                if (full(st[b])) {
#pragma unroll
                    for (int u = 0; u < KP_SUPER; ++u) acc[k0 + b] += v[b][u];
                } else {
                    slow(acc[k0 + b], st[b]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CPW; ++k) red[w + W * k][lane] = acc[k];
    __syncthreads();
    if (w == 0) {
        row2 a = red[0][lane];
#pragma unroll
        for (int h = 1; h < KP_RED_G; ++h) a += red[h][lane];
        const int64_t i = Ib * KP_TILE + 2 * lane;
        if (i < m) raw[i] = a[0];
        if (i + 1 < m) raw[i + 1] = a[1];
    }
}

}  // namespace

namespace {

// one launch of `count` workgroups (tiles [base, base + count) of the rank's table) in one mode
template <typename T, int MODE>
void launch_kp_mode(const kp_geom<T> &g, const T *p, T *partial, int64_t base, int64_t count, const cg_scalars<T> *status,
                    const kp_cache_view<T> &kc, hipStream_t s) {
    if (count <= 0) return;
    const dim3 grid((unsigned) count), block(256);
#define KP_LAUNCH(KERNEL)                                                                                               \
    hipLaunchKernelGGL((kp_tile_kernel<T, KERNEL, MODE>), grid, block, 0, s, g.kf, g.XT, g.norms, p, partial, g.n_pad,    \
                       g.d_pad, g.nb, g.s0, g.nsuper, g.wg_off, status, base, kc.rec, 1, (int64_t) 0, (int64_t) 0, kc.desc, \
                       kc.count, kc.pack)
    if constexpr (MODE == KP_LOAD) {
        KP_LAUNCH(0);  // one instance per real type: the stored values are past the kernel function
    } else {
        switch (g.kf.kernel) {
            case 0: KP_LAUNCH(0); break;
            case 1: KP_LAUNCH(1); break;
            case 2: KP_LAUNCH(2); break;
            case KF_LAPLACIAN: KP_LAUNCH(KF_LAPLACIAN); break;
            default: throw mi_error(-5, "unknown kernel function for the pairwise tile kernel");
        }
    }
#undef KP_LAUNCH
    MI_LAUNCH_CHECK();
}

// what both launchers check first; returns the cached prefix of the rank's tiles that the launch may use
template <typename T>
int64_t kp_cached_prefix(const kp_geom<T> &g, const kp_cache_view<T> &kc, bool need_count) {
    // 32-bit DMA offsets inside a chunk (kp_tile_kernel): (BK - 1) rows of n_pad plus a tile row
    if ((int64_t) kp_dpad<T>() * g.n_pad * (int64_t) sizeof(T) >= ((int64_t) 1 << 31))
        throw mi_error(-5, "too many points for the pairwise tile kernel's 32-bit chunk offsets");
    const int64_t cached = (kc.rec == nullptr || kc.cached < 0) ? 0 : (kc.cached > g.wgs ? g.wgs : kc.cached);
    if (cached > 0 && sizeof(T) == 8 && (kc.desc == nullptr || (need_count && kc.count == nullptr)))
        throw mi_error(-1, "fp64 tile records need their descriptors");
    return cached;
}

}  // namespace

// Tiles [0, cached) of the rank's table have a record in the cache: they are streamed from it (KP_LOAD), or, with
// `fill`, computed and stored (KP_COMPUTE_STORE); tiles [cached, wgs) are computed. cached = 0: one KP_COMPUTE
// launch over all tiles. Every mode writes the same slab records, so the split never shows in K·p.
template <typename T>
void launch_kp_tiles(const kp_geom<T> &g, const T *p, T *partial, const cg_scalars<T> *status, hipStream_t s,
                     const kp_cache_view<T> &kc, bool fill) {
    if (g.nsuper <= 0 || g.nb <= 0 || g.wgs <= 0) return;
    const int64_t cached = kp_cached_prefix(g, kc, true);
    if (fill) launch_kp_mode<T, KP_COMPUTE_STORE>(g, p, partial, 0, cached, status, kc, s);
    else launch_kp_mode<T, KP_LOAD>(g, p, partial, 0, cached, status, kc, s);
    launch_kp_mode<T, KP_COMPUTE>(g, p, partial, cached, g.wgs - cached, status, {}, s);
}

// The batched form: nvec vectors p + c * pstride into the slabs partial + c * sstride, stop flags status[c] (null:
// none). The cached prefix must be filled already (the single-vector path's first K·p does that): tiles [0, cached)
// are streamed, the rest computed, each once for all vectors.
template <typename T>
void launch_kp_tiles_multi(const kp_geom<T> &g, const T *p, int64_t pstride, T *partial, int64_t sstride, int nvec,
                           const cg_scalars<T> *status, hipStream_t s, const kp_cache_view<T> &kc) {
    if (g.nsuper <= 0 || g.nb <= 0 || g.wgs <= 0) return;
    if (nvec < 1 || nvec > KP_MULTI_W) throw mi_error(-1, "bad vector count for the batched tile kernel");
    const int64_t cached = kp_cached_prefix(g, kc, false);
    const dim3 block(256);
#define KP_LAUNCH(KERNEL, MODE, base, count)                                                                               \
    hipLaunchKernelGGL((kp_tile_kernel<T, KERNEL, MODE, true>), dim3((unsigned) (count)), block, 0, s, g.kf, g.XT, g.norms, p, \
                       partial, g.n_pad, g.d_pad, g.nb, g.s0, g.nsuper, g.wg_off, status, (int64_t) (base), kc.rec, nvec,      \
                       pstride, sstride, kc.desc, (int32_t *) nullptr, 0)
    if (cached > 0) {
        KP_LAUNCH(0, KP_LOAD, 0, cached);
        MI_LAUNCH_CHECK();
    }
    if (g.wgs > cached) {
        switch (g.kf.kernel) {
            case 0: KP_LAUNCH(0, KP_COMPUTE, cached, g.wgs - cached); break;
            case 1: KP_LAUNCH(1, KP_COMPUTE, cached, g.wgs - cached); break;
            case 2: KP_LAUNCH(2, KP_COMPUTE, cached, g.wgs - cached); break;
            case KF_LAPLACIAN: KP_LAUNCH(KF_LAPLACIAN, KP_COMPUTE, cached, g.wgs - cached); break;
            default: throw mi_error(-5, "unknown kernel function for the batched pairwise tile kernel");
        }
        MI_LAUNCH_CHECK();
    }
#undef KP_LAUNCH
}

// Both the whole triangle and a rank's share use the chain-split reduction (one block per row block of 128 rows,
// 16 chains of column super-blocks dealt to its waves, the chains added in order): one thread per row walking all
// nb records (round 1's kp_reduce_kernel) was latency-bound — 0.43 ms for config 2's 627 MB slab.
template <typename T>
void launch_kp_reduce(const T *partial, int64_t nb, int64_t m, int64_t s0, int64_t s1, const int32_t *wg_off, T *raw,
                      const cg_scalars<T> *status, hipStream_t s) {
    if (m <= 0) return;
    if (ceil_div(m, (int64_t) KP_TILE) > nb) throw mi_error(-1, "the slab pass needs a row block for every row");
    hipLaunchKernelGGL(kp_reduce_share_kernel<T>, dim3((unsigned) ceil_div(m, (int64_t) KP_TILE)), dim3(64 * KP_RED_WAVES), 0,
                       s, partial, nb, m, s0, s1, wg_off, raw, status);
    MI_LAUNCH_CHECK();
}

#define INST(T)                                                                                                     \
    template void launch_kp_tiles<T>(const kp_geom<T> &, const T *, T *, const cg_scalars<T> *, hipStream_t,       \
                                     const kp_cache_view<T> &, bool);                                                \
    template void launch_kp_tiles_multi<T>(const kp_geom<T> &, const T *, int64_t, T *, int64_t, int,              \
                                           const cg_scalars<T> *, hipStream_t, const kp_cache_view<T> &);            \
    template void launch_kp_reduce<T>(const T *, int64_t, int64_t, int64_t, int64_t, const int32_t *, T *,         \
                                      const cg_scalars<T> *, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace plssvm_mi
