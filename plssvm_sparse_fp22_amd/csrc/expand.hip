// Sparse polynomial / RBF K·p by kernel expansion.
//
// For sparse data most pairs share no feature, and a pair that shares exactly one feature f has
// s_ij = x_if x_jf. Write the pair part of the kernel as a function of s:
//   rbf  (factored):  k_ij = e_i e_j (1 + E(s_ij)),   E(s) = expm1(2 g s),  e_i = exp(-g |x_i|^2)
//   poly:             k_ij = kappa + c(s_ij),          c(s) = (g s + c0)^deg - c0^deg,  kappa = c0^deg
// and let phi be E or c. Then, exactly,
//   phi(s_ij) = sum_{f shared by i, j} phi(x_if x_jf) + H_ij,
// where the remainder H_ij is non-zero only for pairs sharing two or more features (and i == j).
// phi is a polynomial (c exactly, of degree deg; E as its Taylor series, truncated at the degree K
// whose remainder is below the real type's rounding for every |2 g x_if x_jf| of the data), so the
// per-feature part of a row is separable through the column moments:
//   sum_j sum_{f shared} phi(x_if x_jf) w_j = sum_{f in x_i} sum_{k=1..K} coef_k x_if^k M_k(f),
//   M_k(f) = sum_{j in column f} x_jf^k w_j,   w_j = e_j p_j (rbf) | p_j (poly).
// One K·p = the moments (one CSC pass), a CSR pass (Horner per entry), and the stored remainder H of
// the multi-feature pairs (symmetric rows, padded to 8 slots): O(nnz K + #multi pairs) instead of the
// O(sum_f c_f^2) pairs of the Gram pattern, and O(nnz + #multi pairs) memory.
//   rbf : sum_j k_ij p_j = e_i [ S + J_i + H_ii w_i + sum_j H_ij w_j ],  S = sum_j e_j p_j
//   poly: sum_j k_ij p_j = kappa S + J_i + H_ii p_i + sum_j H_ij p_j,     S = sum_j p_j
// (J_i = the moment sum, including j = i). The reference evaluates k(x_i, x_j) for every pair from the
// dense rows (include/plssvm/backends/HIP/svm_kernel.hip.hpp:206-268); the results agree to rounding.
//
// This file holds what runs per K·p and per predict; the setup that builds the stored remainder is
// expand_setup.hip, and expand.hpp holds what both need.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "../../include/plssvm_mi355x.h"
#include "expand.hpp"

namespace plssvm_mi {

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---- per K·p ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void exp_w_kernel(const T *__restrict__ e, const T *__restrict__ p, int64_t m,
                                                    T *__restrict__ w, const cg_scalars<T> *__restrict__ status) {
    if (status != nullptr && status->converged) return;
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) w[i] = e[i] * p[i];
}

// M[f][k] = coef_{k+1} mom[k][f] (the CSR pass gathers the KC channels of a feature together)
template <typename T>
__global__ __launch_bounds__(256) void exp_mscale_kernel(const T *__restrict__ mom, int64_t d, int kc, coefs cf,
                                                         T *__restrict__ M, const cg_scalars<T> *__restrict__ status) {
    if (status != nullptr && status->converged) return;
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d * kc) return;
    const int64_t f = t / kc;
    const int k = (int) (t % kc);
    M[t] = (T) (cf.c[k + 1] * (double) mom[(int64_t) k * d + f]);
}

// the moment pass's P panel slabs reduced straight into the Horner coefficients: M[f][k] = coef_{k+1} sum_q
// partial[q][k d + f], the sum in panel_reduce_kernel's order (quarters combined in order when split), so M is
// bitwise that of panel_reduce + exp_mscale_kernel — one launch fewer per K·p
template <typename T>
__global__ __launch_bounds__(256) void exp_mom_reduce_kernel(const T *__restrict__ partial, int64_t P, int64_t d, int kc,
                                                             int split, coefs cf, T *__restrict__ M,
                                                             const T *__restrict__ spart, int sG, T *__restrict__ sout,
                                                             const cg_scalars<T> *__restrict__ status) {
    if (spart != nullptr && blockIdx.x == gridDim.x - 1) {
        // the extra last block: S = sum_j w_j from w's RED_BLOCKS partials, dot_final_kernel's sum (FIN_PLAIN, which
        // also runs after convergence) — one launch fewer
        __shared__ T red[8];
        T r1, r2;
        cgk::partials_final(spart, sG, red, r1, r2);
        if (threadIdx.x == 0) sout[0] = r1, sout[1] = r2;
        return;
    }
    if (status != nullptr && status->converged) return;
    __shared__ T part[3][64];
    const int64_t ns = d * kc;
    const int lane = split ? (threadIdx.x & 63) : threadIdx.x, quarter = split ? (threadIdx.x >> 6) : 0;
    const int64_t s = (int64_t) blockIdx.x * (split ? 64 : 256) + lane;
    const int64_t per = split ? (P + 3) / 4 : P, q0 = quarter * per, q1 = min(P, q0 + per);
    T a = 0;
    if (s < ns) {
        int64_t q = q0;
        for (; q + 8 <= q1; q += 8) {
            T v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(q + u) * ns + s];
#pragma unroll
            for (int u = 0; u < 8; ++u) a += v[u];
        }
        for (; q < q1; ++q) a += partial[q * ns + s];
    }
    if (split) {
        if (quarter > 0) part[quarter - 1][lane] = a;
        __syncthreads();
        if (quarter != 0) return;
        a = ((a + part[0][lane]) + part[1][lane]) + part[2][lane];
    }
    if (s >= ns) return;
    const int64_t k = s / d, f = s % d;
    M[f * kc + k] = (T) (cf.c[k + 1] * (double) a);
}

// S = sum_j w_j (cw non-null: the centered S_c = sum_j cw_j w_j, engine.hpp ctr_*) as RED_BLOCKS block partials
// in dot2_kernel's grid, order and block reduction (bitwise the same partials), writing the remainder stream's
// bfloat16 copy of w on the way (w16 non-null: hbf16 layouts)
template <typename T>
__global__ __launch_bounds__(256) void exp_wsum_kernel(const T *__restrict__ w, int64_t n, uint16_t *__restrict__ w16,
                                                       const T *__restrict__ cw, T *__restrict__ partials,
                                                       const cg_scalars<T> *__restrict__ status) {
    if (status != nullptr && status->converged) return;
    __shared__ T red[4];
    T s1 = 0;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const T v = w[i];
        s1 += cw != nullptr ? cw[i] * v : v;
        if (w16 != nullptr) w16[i] = bf16_rne((float) v);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s1 += __shfl_xor(s1, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s1;
    __syncthreads();
    if (threadIdx.x == 0) {
        T t = 0;
        for (int v = 0; v < 4; ++v) t += red[v];
        partials[blockIdx.x] = t;
        partials[RED_BLOCKS + blockIdx.x] = T(0);
    }
}

// sharded groups with bfloat16 windows: the rank's rows only — w_i = e_i p_i (rbf; e null: w = p, nothing
// written), its bfloat16 copy, and the rows' share of S = sum_j w_j as RED_BLOCKS block partials (gathered
// with the group's other partials and summed in rank order: the same S on every rank)
// (cw non-null: the rows' share of the centered S_c = sum_j cw_j w_j instead, engine.hpp ctr_*)
template <typename T>
__global__ __launch_bounds__(cgk::CG_NT) void exp_wown_kernel(const T *__restrict__ e, const T *__restrict__ p,
                                                             int64_t ib, int64_t ie, T *__restrict__ w,
                                                             uint16_t *__restrict__ w16, const T *__restrict__ cw,
                                                             T *__restrict__ partials,
                                                             const cg_scalars<T> *__restrict__ status) {
    if (status != nullptr && status->converged) return;
    __shared__ T red[cgk::CG_NT / 64];
    T s1 = 0;
    // the fused CG kernels' grid and element order (cg_dir_sums_kernel carries this pass in a CG iteration: the
    // same partials bit for bit); four elements' loads in flight per thread, summed in the thread's element order
    const int64_t n = ie - ib, st = (int64_t) gridDim.x * blockDim.x;
    const T *pp = p + ib, *ep = e != nullptr ? e + ib : nullptr, *cp = cw != nullptr ? cw + ib : nullptr;
    T *wp = w + ib;
    uint16_t *w16p = w16 + ib;
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * st < n; i += 4 * st) {
        T pv[4], ev[4], cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            pv[u] = pp[i + u * st];
            ev[u] = ep != nullptr ? ep[i + u * st] : T(1);
            cv[u] = cp != nullptr ? cp[i + u * st] : T(0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) cgk::w_elem(i + u * st, pv[u], ev[u], cv[u], ep, cp, wp, w16p, s1);
    }
    for (; i < n; i += st)
        cgk::w_elem(i, pp[i], ep != nullptr ? ep[i] : T(1), cp != nullptr ? cp[i] : T(0), ep, cp, wp, w16p, s1);
    cgk::store_partial1(s1, red, partials);
}

#ifndef EXP_DPP
#define EXP_DPP 1  // remainder stream: segmented row sums by DPP row shifts / broadcasts (0: ds_bpermute shuffles)
#endif
#ifndef EXP_PSCAN
#define EXP_PSCAN 1  // bfloat16 remainder: row sums as differences of one unsegmented lane prefix (0: segmented scan)
#endif
#ifndef EXP_COLPROBE
// cost probe of the one-triangle stream (built only as a variant, -DEXP_COLPROBE=1): every bfloat16
// slot also adds H_ij times a stand-in for w_i into an LDS float at its partner's index with ds_add_f32 — the column
// scatter that design needs — into the row accumulator's LDS (the window already takes the rest), so the results
// are wrong by construction; the timing bounds the design from below
#define EXP_COLPROBE 0
#endif
#ifndef EXP_DOT2
// bfloat16 remainder: a chunk's 4 products as two v_dot2_f32_bf16 (the stream is VALU-bound). The instruction
// pair is inline assembly whose hazard padding (the s_nop in exp_hcell_kernel) was verified on the GPU with the
// ROCm 7.2 compiler (clang 22, tests/test_gpu_sparse.py::test_expansion_dot2_equals_fma_path); any other
// compiler builds the FMA chain until the sequence is re-verified there.
#if HIP_VERSION_MAJOR == 7 && HIP_VERSION_MINOR == 2 && __clang_major__ == 22
#define EXP_DOT2 1
#else
#define EXP_DOT2 0
#endif
#endif

// v added to a row accumulator in LDS (read-add-write; each wave owns its rows). LDS float atomics (ds_add_f32, no
// wait for the read) measured slower in round 6: config 5's pair-flag stream 0.842 -> 1.045 ms, 3-RBF unchanged
template <typename T>
__device__ __forceinline__ void racc_add(T *p, T v) {
    *p += v;
}

// one step of a segmented inclusive lane scan keyed by k (keys non-decreasing in lane order): v += the DPP
// source lane's v when that lane holds the same key. A lane without a source (or in a masked DPP row) reads
// value 0 and key 0 (bound_ctrl / old = 0: no initialising moves) — a false key match then adds +0, which
// changes no sum
template <int CTRL, int ROWS>
__device__ __forceinline__ void seg_step(float &v, int k) {
    const float vs = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xF, true));
    const int ks = __builtin_amdgcn_update_dpp(0, k, CTRL, ROWS, 0xF, true);
    if (ks == k) v += vs;
}
template <int CTRL, int ROWS>
__device__ __forceinline__ void seg_step(double &v, int k) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int) (uint32_t) b, CTRL, ROWS, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int) (b >> 32), CTRL, ROWS, 0xF, false);
    const double vs = __longlong_as_double((long long) (((uint64_t) (uint32_t) hi << 32) | (uint32_t) lo));
    const int ks = __builtin_amdgcn_update_dpp(-2, k, CTRL, ROWS, 0xF, false);
    if (ks == k) v += vs;
}

// hs[i] = sum_j H_ij w_j. One 1024-thread workgroup per block of RB rows walks the windows of
// partners: the window of w (CW values) is staged in LDS (the next window is loaded into registers
// while the current one is used, then stored between two barriers), each wave streams its rows' 4-slot chunks (one
// contiguous range across all windows, coalesced, nontemporal so the stream does not evict w from L2,
// software-pipelined one step ahead, also across window boundaries), gathers w_j from LDS and adds its
// rows' partial sums (segmented shuffle reduction) into an LDS row accumulator only it writes.
// Fixed order, no atomics: bitwise reproducible.
// D2 (bfloat16 H only): the dot instructions (EXP_DOT2) or the FMA chain (PLSSVM_MI_EXP_DOT2=0: tests, A/B)
// RF: 0 = a stored row index per chunk, 1 = row-start flags per chunk, 2 = row-start flags per slot pair (cells
// padded to 2 slots instead of 4, see "pair flags" below)
template <typename T, int RBB, bool HB, int RF = 0, bool D2 = true>
__global__ __launch_bounds__(EXP_NWV * 64) void exp_hcell_kernel(const int64_t *__restrict__ woff,
                                                                 const uint16_t *__restrict__ hrow,
                                                                 const uint16_t *__restrict__ hjl,
                                                                 const T *__restrict__ hv,
                                                                 const uint16_t *__restrict__ hv16, const T *__restrict__ w,
                                                                 const uint16_t *__restrict__ w16,
                                                                 int64_t m, int64_t r0, int64_t R, int64_t nW,
                                                                 int64_t RB, int64_t nI, int G, T *__restrict__ hs,
                                                                 T *__restrict__ hslab,
                                                                 const cg_scalars<T> *__restrict__ status, int wdrop = 0) {
    // wdrop = 1: test-only ablation (PLSSVM_MI_EXP_ABLATE bit 2), the last window of every row block is skipped
    // RB (rows per block, a multiple of 16) <= RBC, the accumulator's capacity. G > 1 window groups:
    // block (I, g) streams only windows [g nW / G, (g + 1) nW / G) of its rows and writes its row sums
    // to hslab[g][rows] (summed in g order by exp_combine_kernel); the blocks of one XCD share g,
    // so they share w's windows in L2
    // HB: H and the window of w in bfloat16 (twice the partners per window; expand_setup.hip "H storage")
    using WT = std::conditional_t<HB, uint16_t, T>;
    constexpr int CW = HB ? exp_cw16_of<RBB>() : exp_cw_of<T, RBB>(), RBC = exp_rb_of<T, RBB>(), NT = EXP_NWV * 64;
    static_assert(CW <= 65536, "window-local partner indices are 16-bit");
    __shared__ __attribute__((aligned(16))) WT wl[CW];
    __shared__ T racc[RBC];
    const WT *wsrc;
    if constexpr (HB) wsrc = w16;
    else wsrc = w;
    if (status != nullptr && status->converged) return;
    const int64_t bx = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t I = bx % nI, g = bx / nI;
    const int64_t W0 = g * nW / G, W1 = (g + 1) * nW / G - (wdrop && g == G - 1 && nW > 0 ? 1 : 0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform: the wave's offsets are scalar loads
    for (int t = tid; t < RB; t += NT) racc[t] = T(0);
    // the window of w moves as 16-byte vectors: thread tid takes vectors tid, tid + NT, ... (PV of them)
    constexpr int VE = 16 / (int) sizeof(WT), NV = CW / VE, PV = (NV + NT - 1) / NT;
    using wvec = __attribute__((ext_vector_type(VE))) WT;
    wvec reg[PV];
    auto load_win = [&](int64_t W) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const int v = q * NT + tid;
            if (NV % NT == 0 || v < NV) {
                const int64_t idx = W * CW + (int64_t) v * VE;
                if (idx + VE <= m) {
                    reg[q] = *reinterpret_cast<const wvec *>(wsrc + idx);
                } else {
#pragma unroll
                    for (int e = 0; e < VE; ++e) reg[q][e] = idx + e < m ? wsrc[idx + e] : WT(0);
                }
            }
        }
    };
    auto wat = [&](uint32_t j) __attribute__((always_inline)) -> T {  // w_j from the staged window
        if constexpr (HB) return (T) __uint_as_float((uint32_t) wl[j] << 16);
        else return wl[j];
    };
    auto store_win = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < PV; ++q) {
            const int v = q * NT + tid;
            if (NV % NT == 0 || v < NV) reinterpret_cast<wvec *>(wl)[v] = reg[q];
        }
    };
    const int64_t *wo = woff + (I * EXP_NWV + wave) * (nW + 1);
    const int64_t s_end = wo[W1];
    // one step of the stream in registers: EXP_NH groups of 64 chunks (group h: chunk step start + 64 h +
    // lane), loads clamped to the stream; prefetched one step ahead
    struct group_regs {
        int rl = 0;
        u32x2 jj = { 0u, 0u };
        T h[4] = { T(0), T(0), T(0), T(0) };
        u32x2 hb = { 0u, 0u };  // bfloat16 H, kept raw until the step uses it (a conversion here would wait for the load)
    };
    group_regs nx[EXP_NH];
    const bool empty = s_end == wo[W0];
    auto fetch = [&](int64_t c) __attribute__((always_inline)) {
        if (empty) return;  // empty stream (wave-uniform)
#pragma unroll
        for (int hh = 0; hh < EXP_NH; ++hh) {
            const int64_t cl = c + 64 * hh;  // past s_end: the stream's zeroed padding (masked by have)
            group_regs &g = nx[hh];
            if constexpr (!RF) g.rl = (int) __builtin_nontemporal_load(hrow + cl);
            if constexpr (RF && EXP_JH) {  // indices and H of the chunk in one 16-byte load
                const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(hjl + 8 * cl));
                g.jj = u32x2{ v.x, v.y };
                g.hb = u32x2{ v.z, v.w };
                continue;
            }
            g.jj = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(hjl + 4 * cl));
            if constexpr (HB) {
                g.hb = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(hv16 + 4 * cl));
            } else if constexpr (sizeof(T) == 4) {
                const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(hv + 4 * cl));
                g.h[0] = v.x, g.h[1] = v.y, g.h[2] = v.z, g.h[3] = v.w;
            } else {
                const f64x2 v0 = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(hv + 4 * cl));
                const f64x2 v1 = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(hv + 4 * cl + 2));
                g.h[0] = v0.x, g.h[1] = v0.y, g.h[2] = v1.x, g.h[3] = v1.y;
            }
        }
    };
    // one group of 64 chunks: the 4 slots times w from the window, then the rows' sums into racc
    // RF: the rows of a window's chunks from their row-start flags (carry = the row before the step's first chunk + 1)
    int carry = 0;
#if EXP_COLPROBE
    auto col_probe = [&](u32x2 jj, uint32_t hx, uint32_t hy, float wi) __attribute__((always_inline)) {
        if constexpr (HB && sizeof(T) == 4) {
            constexpr uint32_t MSK = (uint32_t) RBC - 1u;  // RBC: a power of two
            atomicAdd(&racc[(jj.x & 0xFFFFu) & MSK], __uint_as_float(hx << 16) * wi);
            atomicAdd(&racc[(jj.x >> 16) & MSK], __uint_as_float(hx & 0xFFFF0000u) * wi);
            atomicAdd(&racc[(jj.y & 0xFFFFu) & MSK], __uint_as_float(hy << 16) * wi);
            atomicAdd(&racc[(jj.y >> 16) & MSK], __uint_as_float(hy & 0xFFFF0000u) * wi);
        }
    };
#endif
    auto group = [&](const group_regs &g, bool have) __attribute__((always_inline)) {
        if constexpr (RF == 2) {
            static_assert(HB && EXP_JH && sizeof(T) == 4, "pair flags: bfloat16 H, side-by-side chunks");
            // pair flags: bit 14 of the chunk's H0 / H2 marks a row starting at slot 0 / 2. A lane's two pairs give
            // a01 (slots 0, 1) and a23 (slots 2, 3); t = a01 + a23. With P the inclusive lane prefix of t and E the
            // exclusive one, a row that starts in lane A (its tail there) and ends in lane B (its head there) sums to
            // tail_A - P_A + E_B + head_B: lanes with a flag add tail - P to the row they leave open and E + head to
            // the row their first flag closes; a row inside one lane (pair 0 flagged and pair 1 flagged) adds a01;
            // lane 63 adds P_63 to the row open at the group's end. Each phase writes distinct rows (one instruction
            // never updates a row twice); fixed order: bitwise reproducible. The cancellation bound of the prefix
            // differences is the one of the chunk-flag layout below (bfloat16 H: <= 2^-24 of the group's |H w|).
            const bool f0 = have && (g.hb.x & 0x4000u) != 0u, f1 = have && (g.hb.y & 0x4000u) != 0u;
            const uint32_t hx = g.hb.x & ~0x4000u, hy = g.hb.y & ~0x4000u;
            float a01 = 0.f, a23 = 0.f;
            if (have) {
                const u32x2 jj = g.jj;
                const uint32_t w01 = (uint32_t) wl[jj.x & 0xFFFFu] | ((uint32_t) wl[jj.x >> 16] << 16);
                const uint32_t w23 = (uint32_t) wl[jj.y & 0xFFFFu] | ((uint32_t) wl[jj.y >> 16] << 16);
                if constexpr (D2 && EXP_DOT2) {
                    asm("v_dot2_f32_bf16 %0, %2, %3, 0\n\tv_dot2_f32_bf16 %1, %4, %5, 0\n\ts_nop 1"
                        : "=&v"(a01), "=&v"(a23)
                        : "v"(hx), "v"(w01), "v"(hy), "v"(w23));
                } else {
                    a01 = __uint_as_float(hx << 16) * __uint_as_float(w01 << 16);
                    a01 = fmaf(__uint_as_float(hx & 0xFFFF0000u), __uint_as_float(w01 & 0xFFFF0000u), a01);
                    a23 = __uint_as_float(hy << 16) * __uint_as_float(w23 << 16);
                    a23 = fmaf(__uint_as_float(hy & 0xFFFF0000u), __uint_as_float(w23 & 0xFFFF0000u), a23);
                }
#if EXP_COLPROBE
                col_probe(jj, hx, hy, a01);
#endif
            }
            const float t = a01 + a23;
            float P = t;
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x111, 0xF, 0xF, true));  // row_shr:1
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x112, 0xF, 0xF, true));  // row_shr:2
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x114, 0xF, 0xF, true));  // row_shr:4
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x118, 0xF, 0xF, true));  // row_shr:8
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x142, 0xA, 0xF, true));  // row_bcast:15
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x143, 0xC, 0xF, true));  // row_bcast:31
            const float E = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x138, 0xF, 0xF, true));  // wave_shr:1
            const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1), bh = __ballot(have);
            const int below = (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) b0, 0u)) +
                              (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) b1, 0u));
            const int row0 = carry + below + (f0 ? 1 : 0) - 1, row1 = row0 + (f1 ? 1 : 0);
            carry += __popcll(b0) + __popcll(b1);
            if (bh == 0ull) return;  // a group wholly past the window's end
            if (f0 || f1) racc_add(&racc[f1 ? row1 : row0], (f1 ? a23 : t) - P);  // tail: the row left open in this lane
            if (f0 && f1) racc_add(&racc[row0], a01);                             // a row inside this lane
            // head: not for a row that starts at the group's first valid lane (its predecessor is no row of this pass)
            const int lead = __builtin_ctzll(bh);
            if ((f0 || f1) && !(lane == lead && f0)) racc_add(&racc[(f0 ? row0 : row1) - 1], E + (f0 ? 0.f : a01));
            if (lane == 63) racc_add(&racc[row1], P);                             // the row open at the group's end
            return;
        }
        int rl = have ? g.rl : -1;
        uint32_t hx = g.hb.x;
        if constexpr (RF) {
            const uint32_t fb = (hx >> 14) & 1u;  // the row-start flag as 0 / 1
            const unsigned long long bal = __ballot((hx & 0x4000u) != 0u) & __ballot(have);
            const int below = (int) __builtin_amdgcn_mbcnt_hi((uint32_t) (bal >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t) bal, 0u));
            rl = have ? carry + below + (int) fb - 1 : -1;
            carry += __popcll(bal);
            hx &= ~0x4000u;
        }
        const u32x2 jj = g.jj;
        T h0 = g.h[0], h1 = g.h[1], h2 = g.h[2], h3 = g.h[3];
        if constexpr (HB) {  // bfloat16 H: the float's top 16 bits
            h0 = (T) __uint_as_float(hx << 16), h1 = (T) __uint_as_float(hx & 0xFFFF0000u);
            h2 = (T) __uint_as_float(g.hb.y << 16), h3 = (T) __uint_as_float(g.hb.y & 0xFFFF0000u);
        }
        T acc = T(0);
        if constexpr (HB && D2 && EXP_DOT2 && sizeof(T) == 4) {
            // bfloat16 H and w: the pairs' products (exact in fp32) summed by two bf16 dot instructions, H and w
            // packed as they are stored (the window holds w's bfloat16 bits)
            (void) h0, (void) h1, (void) h2, (void) h3;
            if (have) {
                const uint32_t w01 = (uint32_t) wl[jj.x & 0xFFFFu] | ((uint32_t) wl[jj.x >> 16] << 16);
                const uint32_t w23 = (uint32_t) wl[jj.y & 0xFFFFu] | ((uint32_t) wl[jj.y >> 16] << 16);
                // VOP3P form in inline assembly: the compiler's v_dot2c lowering of two chained
                // __builtin_amdgcn_fdot2_f32_bf16 calls read the same H register twice here (ROCm 7.2 clang);
                // the s_nop covers the DPP read of acc that follows (2 wait states after a VALU write)
                asm("v_dot2_f32_bf16 %0, %1, %2, 0\n\tv_dot2_f32_bf16 %0, %3, %4, %0\n\ts_nop 1"
                    : "=&v"(acc)
                    : "v"(hx), "v"(w01), "v"(g.hb.y), "v"(w23));
#if EXP_COLPROBE
                col_probe(jj, hx, g.hb.y, acc);
#endif
            }
        } else if (have) {
            acc = h0 * wat(jj.x & 0xFFFFu);
            acc = fma(h1, wat(jj.x >> 16), acc);
            acc = fma(h2, wat(jj.y & 0xFFFFu), acc);
            acc = fma(h3, wat(jj.y >> 16), acc);
        }
#if EXP_DPP
        if constexpr (HB && EXP_PSCAN && sizeof(T) == 4) {
            // bfloat16 H (|H w| <= 2^-16 |k w| per pair): an unsegmented inclusive prefix P of the 64 chunk sums (six
            // DPP adds, no keys); a row ending at lane e adds P_e to its accumulator and the row that starts at
            // e + 1 subtracts it — the row's sum as a difference of prefixes. The cancellation costs at most
            // 2^-24 of the group's |H w| (<= 256 pair terms of <= 2^-16 |k w| each), far below the float rounding
            // of the row's K·p; fixed order, bitwise reproducible.
            float P = acc;
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x111, 0xF, 0xF, true));  // row_shr:1
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x112, 0xF, 0xF, true));  // row_shr:2
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x114, 0xF, 0xF, true));  // row_shr:4
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x118, 0xF, 0xF, true));  // row_shr:8
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x142, 0xA, 0xF, true));  // row_bcast:15
            P += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(P), 0x143, 0xC, 0xF, true));  // row_bcast:31
            const int rnext = __builtin_amdgcn_update_dpp(-1, rl, 0x130, 0xF, 0xF, false);  // wave_shl:1 (lane 63: -1)
            const bool end = rl >= 0 && (lane == 63 || rnext != rl);
            if (end) racc_add(&racc[rl], (T) P);  // rows of this wave only
            if (end && lane != 63 && rnext >= 0) racc_add(&racc[rnext], -(T) P);
            return;
        }
        // segmented inclusive prefix sums over the lanes by DPP (rows are non-decreasing in lane order):
        // row_shr 1/2/4/8 inside each 16-lane row, then row_bcast 15 / 31 across rows; the total of a
        // row's run lands on its last lane, which adds it to the row accumulator
        T sacc = acc;
        seg_step<0x111, 0xF>(sacc, rl);  // row_shr:1
        seg_step<0x112, 0xF>(sacc, rl);  // row_shr:2
        seg_step<0x114, 0xF>(sacc, rl);  // row_shr:4
        seg_step<0x118, 0xF>(sacc, rl);  // row_shr:8
        seg_step<0x142, 0xA>(sacc, rl);  // row_bcast:15 (rows 1, 3)
        seg_step<0x143, 0xC>(sacc, rl);  // row_bcast:31 (rows 2, 3)
        const int rnext = __builtin_amdgcn_update_dpp(0, rl, 0x130, 0xF, 0xF, true);  // wave_shl:1 (lane 63: tested apart)
        if (rl >= 0 && (lane == 63 || rnext != rl)) racc_add(&racc[rl], sacc);  // rows of this wave only
#else
        // segmented suffix sums: rows are non-decreasing in lane order
        T sacc = acc;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const T so = __shfl_down(sacc, off);
            const int rr = __shfl_down(rl, off);
            if (lane + off < 64 && rr == rl) sacc += so;
        }
        const int rprev = __shfl_up(rl, 1);
        if (rl >= 0 && (lane == 0 || rprev != rl)) racc[rl] += sacc;  // rows of this wave only
#endif
    };
    if (W0 < W1) {
        load_win(W0);
        store_win();
        fetch(wo[W0] + lane);
    }
    __syncthreads();
    constexpr int STEP = 64 * EXP_NH;
    // Steps restart at every window: the part of a window's last step past its end is masked and loaded again as the
    // next window's first step (mostly from L2). Round 6 measured a walk that ignores the window boundaries (a
    // straddling step processed for both windows, nothing loaded twice): 3-RBF 0.766 vs 0.770 ms over three same-box
    // pairs and FETCH 4.915 vs 4.93 GB — nothing to show for it; with pair flags 4.5 % slower (registers, a spill).
    for (int64_t W = W0; W < W1; ++W) {
        if (W + 1 < W1) load_win(W + 1);  // lands in registers while this window is processed
        const int64_t c_end = wo[W + 1];
        carry = wave * (int) (RB / EXP_NWV);  // RF: the wave's first row starts every window
        for (int64_t cb = wo[W]; cb < c_end; cb += STEP) {  // wave-uniform trip count
            group_regs cur[EXP_NH];
#pragma unroll
            for (int hh = 0; hh < EXP_NH; ++hh) cur[hh] = nx[hh];
            // next step (next window's first at c_end; groups past a window's end are loaded, masked, and
            // loaded again as the next window's)
            fetch((cb + STEP < c_end ? cb + STEP : c_end) + lane);
#pragma unroll
            for (int hh = 0; hh < EXP_NH; ++hh) group(cur[hh], cb + 64 * hh + lane < c_end);  // groups in order
        }
        if (W + 1 < W1) {
            __syncthreads();  // every wave is done with window W
            store_win();
        }
        __syncthreads();
    }
    const int64_t rb0 = I * RB;
    const int rows = (int) min<int64_t>(RB, R - rb0);
    if (G == 1) {
        for (int t = tid; t < rows; t += NT) hs[r0 + rb0 + t] = racc[t];
    } else {
        for (int t = tid; t < rows; t += NT) hslab[g * R + rb0 + t] = racc[t];
    }
}

// raw_i for rows [r0, r1) (0 elsewhere), raw holding J_i there (the CSR pass): base + scale (J_i +
// H_ii w_i + hs_i, hs_i = the remainder stream's row sum) [- the diagonal's pair part when only the overlap part is asked for], in fp64.
// jslab != null: the CSR pass left its P < 16 panel slabs (jslab[q][i - r0]) and J_i is their sum from 0 in
// panel order — panel_reduce_kernel's sum, bit for bit, without its launch
// one row of the combine (rows [r0, r1)): the body of exp_combine_kernel, shared with the fused combine +
// CG finalize so both compile the same arithmetic
// cb non-null: the centered base cb_i S (engine.hpp ctr_*) in place of e_i S / kappa S
template <typename T>
__device__ __forceinline__ T exp_combine_row(const T *__restrict__ e, const T *__restrict__ cb, const T *__restrict__ w,
                                             const T *__restrict__ hdiag,
                                             const T *__restrict__ phin, const T *__restrict__ hs,
                                             const T *__restrict__ hslab, int G, const T *__restrict__ jslab, int P,
                                             const T *__restrict__ raw, const T *__restrict__ ssc, T kappa, int64_t i,
                                             int64_t r0, int64_t r1, int overlap_only) {
    const double wi = (double) w[i];
    T h = 0;  // the remainder stream's row sum (G window groups: their slabs in g order)
    if (G > 1) {
        for (int g = 0; g < G; ++g) h += hslab[(int64_t) g * (r1 - r0) + (i - r0)];
    } else {
        h = hs[i];
    }
    T J;
    if (jslab != nullptr) {
        J = T(0);
        for (int q = 0; q < P; ++q) J += jslab[(int64_t) q * (r1 - r0) + (i - r0)];
    } else {
        J = raw[i];
    }
    const double t = (double) J + (double) hdiag[i] * wi + (double) h;
    const double sc = e != nullptr ? (double) e[i] : 1.0;
    double v;
    if (overlap_only == 2) {  // PLSSVM_MI_PART_REMAINDER: the remainder stream's row sum alone
        v = sc * (double) h;
    } else if (overlap_only) {
        v = sc * (t - (double) phin[i] * wi);
    } else {
        const double base =
            (cb != nullptr ? (double) cb[i] : e != nullptr ? (double) e[i] : (double) kappa) * (double) ssc[0];
        v = base + sc * t;
    }
    return (T) v;
}

template <typename T>
__global__ __launch_bounds__(256) void exp_combine_kernel(const T *__restrict__ e, const T *__restrict__ cb,
                                                          const T *__restrict__ w,
                                                          const T *__restrict__ hdiag, const T *__restrict__ phin,
                                                          const T *__restrict__ hs, const T *__restrict__ hslab, int G,
                                                          const T *__restrict__ jslab, int P,
                                                          const T *__restrict__ ssc, T kappa,
                                                          int64_t ib, int64_t ie, int64_t r0, int64_t r1, int overlap_only,
                                                          T *__restrict__ raw, const cg_scalars<T> *__restrict__ status) {
    if (status != nullptr && status->converged) return;
    const int64_t i = ib + (int64_t) blockIdx.x * blockDim.x + threadIdx.x;  // rows [ib, ie)
    if (i >= ie) return;
    if (i < r0 || i >= r1) {
        raw[i] = T(0);
        return;
    }
    raw[i] = exp_combine_row<T>(e, cb, w, hdiag, phin, hs, hslab, G, jslab, P, raw, ssc, kappa, i, r0, r1, overlap_only);
}

// the combine of a CG iteration's K·p fused with the iteration's finalize (cg_fin_dad_kernel): rows [r0, r1) =
// the CG's own rows, in cg_fin_dad_kernel's grid (RED_BLOCKS x CG_NT), element order and partials — Ad and the
// d.Ad partials bit for bit those of the two launches, raw is not written
// DG = T: the scalar diagonal 1/C; DG = row_diag<T>: (1/C)(1/s_i) with point weights (kernels.hpp; sinv is whole-length
// like q here)
template <typename T, typename DG>
__global__ __launch_bounds__(cgk::CG_NT) void exp_combine_fin_kernel(
    const T *__restrict__ e, const T *__restrict__ cb, const T *__restrict__ w, const T *__restrict__ hdiag, const T *__restrict__ hs,
    const T *__restrict__ hslab, int G, const T *__restrict__ jslab, int P, const T *__restrict__ raw,
    const T *__restrict__ ssc, T kappa, int64_t r0, int64_t r1, const T *__restrict__ q, const T *__restrict__ d,
    const T *__restrict__ psum, int GP, T QA_cost, DG cost_inv, T *__restrict__ Ad, T *__restrict__ pdad,
    cg_scalars<T> *sc) {
    if (sc->converged) return;
    __shared__ T red[cgk::CG_NT / 64], bc[1];
    T sp, sqp;
    cgk::partials_total(psum, GP, red, bc, sp, sqp);
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->sp = sp, sc->sqp = sqp;
    const int64_t st = (int64_t) gridDim.x * blockDim.x;
    T s1 = 0;
    for (int64_t k = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; k < r1 - r0; k += st) {
        const int64_t i = r0 + k;
        const T rw = exp_combine_row<T>(e, cb, w, hdiag, nullptr, hs, hslab, G, jslab, P, raw, ssc, kappa, i, r0, r1, 0);
        const T di = d[i];
        const T v = cgk::cg_fin_value(rw, q[i], di, sp, sqp, QA_cost, diag_at(cost_inv, i), 0);
        Ad[i] = v;
        s1 = cgk::cg_acc(s1, di, v);
    }
    cgk::store_partial_first(s1, red, pdad);  // (consumers read the first partial of the pair only)
}

}  // namespace

// timing/test-only ablations (results are wrong when non-zero): PLSSVM_MI_EXP_ABLATE bit 0 = drop the
// stored remainder H of the multi-feature pairs, bit 1 = keep only the first term of phi's polynomial, bit 2 =
// the remainder stream skips the last partner window of every row block (chunk layouts)
int exp_ablate() {
    static const int v = [] {
        const char *s = std::getenv("PLSSVM_MI_EXP_ABLATE");
        return s ? std::atoi(s) : 0;
    }();
    return v;
}

// the remainder stream alone (the dominant kernel of the expansion's K·p; time_kp / bench roofline)
template <typename T>
void engine<T>::expansion_dominant(const T *w, const cg_scalars<T> *status) {
    auto &ex = csr.ex;
    if (ex.nblk > 0 && !(exp_ablate() & 1)) {
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned) (ex.nblk * ex.G)), dim3(EXP_NWV * 64), 0, stream, ex.woff.get(),
                               ex.hrow.get(), ex.hjl.get(), ex.hv.get(), ex.hv16.get(), w, ex.wv16.get(), m, r0, r1 - r0, ex.nW,
                               (int64_t) ex.RB, ex.nblk, ex.G, ex.hs.get(), ex.hslab.get(), status, (exp_ablate() & 4) ? 1 : 0);
        };
        {
            auto pick = [&](auto hb, auto rf, auto d2) {
                constexpr bool HB = decltype(hb)::value, D2 = decltype(d2)::value;
                constexpr int RF = decltype(rf)::value;
                switch (ex.RBB) {
                    case 4096: launch(exp_hcell_kernel<T, 4096, HB, RF, D2>); break;
                    case 8192: launch(exp_hcell_kernel<T, 8192, HB, RF, D2>); break;
                    case 32768: launch(exp_hcell_kernel<T, 32768, HB, RF, D2>); break;
                    default: launch(exp_hcell_kernel<T, 16384, HB, RF, D2>);
                }
            };
            const bool dot2 = ex.dot2;
            using R0 = std::integral_constant<int, 0>;
            using R1 = std::integral_constant<int, 1>;
            using R2 = std::integral_constant<int, 2>;
            if constexpr (sizeof(T) == 4) {
                if (ex.hbf16 && ex.rpairs && dot2) pick(std::true_type{}, R2{}, std::true_type{});
                else if (ex.hbf16 && ex.rpairs) pick(std::true_type{}, R2{}, std::false_type{});
                else if (ex.hbf16 && ex.rflags && dot2) pick(std::true_type{}, R1{}, std::true_type{});
                else if (ex.hbf16 && ex.rflags) pick(std::true_type{}, R1{}, std::false_type{});
                else if (ex.hbf16 && dot2) pick(std::true_type{}, R0{}, std::true_type{});
                else if (ex.hbf16) pick(std::true_type{}, R0{}, std::false_type{});
                else pick(std::false_type{}, R0{}, std::true_type{});
            } else {
                pick(std::false_type{}, R0{}, std::true_type{});
            }
        }
        MI_LAUNCH_CHECK();  // G > 1: the row sums stay in hslab, summed in g order by exp_combine_kernel
    } else if (r1 > r0) {
        MI_HIP_CHECK(hipMemsetAsync(ex.hs.get() + r0, 0, sizeof(T) * (size_t) (r1 - r0), stream));
        if (ex.G > 1) MI_HIP_CHECK(hipMemsetAsync(ex.hslab.get(), 0, sizeof(T) * (size_t) (ex.G * (r1 - r0)), stream));
    }
}

// the column-moment pass (SELL CSC pass, mode 1) over rows [csc_r0, csc_r1); several panels: their slabs are
// reduced straight into the scaled Horner coefficients M (returns true), one panel: the pass wrote the raw
// moments mom, scaled by expansion_mscale after the group's all-reduce (returns false)
template <typename T>
bool engine<T>::expansion_moments_fused() const {
    const auto &pl = csr.spmv_csc;
    return pl.P > 1 && pl.nseg == d && pl.nblocks > 0;
}

// spart != null (fused passes only): the moment reduce also forms S = csr.ssc from w's partials (sG sets)
template <typename T>
bool engine<T>::expansion_moment_pass(const T *w, const cg_scalars<T> *status, const T *spart, int sG) {
    auto &ex = csr.ex;
    const auto &pl = csr.spmv_csc;
    const bool fused = expansion_moments_fused();
    launch_panel_spmv<T>(pl, w + csr.csc_r0, csr.csc_r1 - csr.csc_r0, ex.mom.get(), status, stream, ex.KM, 1, !fused);
    if (fused) {
        const int split = pl.P >= 16 ? 1 : 0;
        const unsigned nb = (unsigned) ceil_div(d * ex.KM, split ? 64 : 256) + (spart != nullptr ? 1u : 0u);
        hipLaunchKernelGGL(exp_mom_reduce_kernel<T>, dim3(nb), dim3(256), 0, stream, pl.partial.get(), pl.P, d, ex.KM, split,
                           expansion_coefs(), ex.M.get(), spart, sG, csr.ssc.get(), status);
        MI_LAUNCH_CHECK();
    }
    return fused;
}

template <typename T>
void engine<T>::expansion_moments(const T *w, const cg_scalars<T> *status, const T *spart, int sG) {
    auto &ex = csr.ex;
    if (d > 0) {  // column moments, then the coefficients (a real group: each rank's rows, then one
        // all-reduce of the d x K values — linear, so the scaled coefficients are all-reduced when fused)
        const bool fused = expansion_moment_pass(w, status, spart, sG);
        if (csr.csc_r1 - csr.csc_r0 < m) allreduce(fused ? ex.M.get() : ex.mom.get(), d * ex.KM);
        if (!fused) expansion_mscale(status);
    }
}

template <typename T>
coefs engine<T>::expansion_coefs() const {
    coefs cf;
    std::memcpy(cf.c, csr.ex.coef, sizeof(cf.c));
    if (exp_ablate() & 2)
        for (int k = 2; k <= EXP_KMAX; ++k) cf.c[k] = 0.0;
    return cf;
}

// M[f][k] = coef_{k+1} mom[k][f] (after the group's all-reduce of the moments)
template <typename T>
void engine<T>::expansion_mscale(const cg_scalars<T> *status) {
    auto &ex = csr.ex;
    if (d <= 0) return;
    hipLaunchKernelGGL(exp_mscale_kernel<T>, dim3((unsigned) ceil_div(d * ex.KM, 256)), dim3(256), 0, stream,
                       ex.mom.get(), d, ex.KM, expansion_coefs(), ex.M.get(), status);
    MI_LAUNCH_CHECK();
}

// The CG direction update carries the next K·p's w pass (round 5): with bfloat16 windows the K·p of d starts with
// exp_wown_kernel over the rows the direction update has just written (w = e d, its bfloat16 copy, S partials); the
// update forms them in its own element loop (cgk::w_elem, the same grid and order: the same bits) and the K·p skips
// the launch. Sharded: the rank's rows, whose w the group then gathers as before. (Measured neutral, round 5.)
template <typename T>
bool engine<T>::dir_w_fill(dir_w_t<T> &o) {
    if (!sparse_stored() || factored() || csr.otf_on || !csr.ex.on || !csr.ex.hbf16) return false;
    if (shard) {  // expansion_kp_raw's g16 over [r0, r1)
        const bool rgrp = comm != nullptr && cstream != nullptr;
        if (d <= 0 || !(rgrp || sim_world > 0) || v0 != r0 || vn != r1 - r0) return false;
    } else if (v0 != 0 || vn != m) {  // wown_all over [0, m)
        return false;
    }
    o.e = kernel == 2 ? csr.e.get() + v0 : nullptr;
    o.w = kernel == 2 ? csr.ex.wv.get() + v0 : nullptr;
    o.w16 = csr.ex.wv16.get() + v0;
    o.cw = ctr_active() && kernel == 2 ? ctr_cw.get() + v0 : nullptr;
    o.spart = wsp.get();
    return true;
}

template <typename T>
void engine<T>::expansion_kp_raw(const T *p, const cg_scalars<T> *status, bool with_base) {
    auto &ex = csr.ex;
    // sharded: w of this rank's rows, then gathered from every rank (the remainder stream reads partners of
    // all rows); the raw of this rank's rows stays local (no row gather)
    const int64_t ib = shard ? r0 : 0, ie = shard ? r1 : m;
    const T *w = p;
    // sharded RCCL group with bfloat16 windows: the bfloat16 w (2 B per row) is what the group gathers
    // (a simulated rank of such a group runs the same kernels without the collectives: timing only)
    const bool rgrp = shard && comm != nullptr && cstream != nullptr && d > 0;
    const bool g16 = shard && d > 0 && ex.hbf16 && (rgrp || sim_world > 0);
    // unsharded with bfloat16 windows: w, its bfloat16 copy and the S partials in one pass (exp_wown_kernel over
    // all rows: exp_w_kernel's w and exp_wsum_kernel's partials, bit for bit)
    const bool wown_all = !shard && ex.hbf16;
    // centered finalize (engine.hpp ctr_*): S becomes S_c = sum_j cw_j w_j, the combine's base c_i S_c (rbf) / 0 (poly)
    const T *cw = ctr_now && kernel == 2 ? ctr_cw.get() : nullptr;
    // the w pass's S partials (spt): wsp for exp_wown_kernel and the direction update that carries it (w_pre == p:
    // done, dir_w_fill), red for exp_wsum_kernel
    T *spt = (g16 || wown_all) ? wsp.get() : red.get();
    const bool pre = (g16 || wown_all) && w_pre != nullptr && w_pre == p;
    w_pre = nullptr;  // any other w pass below overwrites w, its copy and the partials
    if (g16 || wown_all) {
        if (!pre) {
            hipLaunchKernelGGL(exp_wown_kernel<T>, dim3(RED_BLOCKS), dim3(cgk::CG_NT), 0, stream,
                               kernel == 2 ? csr.e.get() : nullptr, p, ib, ie, ex.wv.get(), ex.wv16.get(), cw, spt, status);
            MI_LAUNCH_CHECK();
        }
        if (kernel == 2) w = ex.wv.get();
    } else if (kernel == 2) {
        if (ie > ib)
            hipLaunchKernelGGL(exp_w_kernel<T>, dim3((unsigned) ceil_div(ie - ib, 256)), dim3(256), 0, stream,
                               csr.e.get() + ib, p + ib, ie - ib, ex.wv.get() + ib, status);
        MI_LAUNCH_CHECK();
        w = ex.wv.get();
    }
    if (rgrp) {
        // sharded RCCL group: the all-gather of w (with the pending CG partials) and the all-reduce of the
        // moments run on the collective stream, overlapping the moments pass and the remainder stream
        MI_HIP_CHECK(hipEventRecord(cev[0], stream));
        MI_HIP_CHECK(hipStreamWaitEvent(cstream, cev[0], 0));
        MI_NCCL_CHECK(ncclGroupStart());
        if (psum_pending) {  // the previous CG step's direction partials ride along
            MI_NCCL_CHECK(ncclAllGather(cgp.get(), cgp_g.get(), (size_t) (2 * RED_BLOCKS), nccl_type<T>(), comm, cstream));
            psum_pending = false;
        }
        T *sg = cgp_g.get() + (int64_t) 4 * G * 2 * RED_BLOCKS;  // slot 4: the ranks' S partials
        if (g16) {
            MI_NCCL_CHECK(ncclAllGather(ex.wv16.get() + (int64_t) rank * chunk, ex.wv16.get(), (size_t) chunk, ncclBfloat16,
                                        comm, cstream));
            MI_NCCL_CHECK(ncclAllGather(spt, sg, (size_t) (2 * RED_BLOCKS), nccl_type<T>(), comm, cstream));
        } else {
            MI_NCCL_CHECK(ncclAllGather(const_cast<T *>(w) + (int64_t) rank * chunk, const_cast<T *>(w), (size_t) chunk,
                                        nccl_type<T>(), comm, cstream));
        }
        MI_NCCL_CHECK(ncclGroupEnd());
        MI_HIP_CHECK(hipEventRecord(cev[1], cstream));
        const bool fused = expansion_moment_pass(w, status);
        T *mt = fused ? ex.M.get() : ex.mom.get();
        MI_HIP_CHECK(hipEventRecord(cev[2], stream));
        MI_HIP_CHECK(hipStreamWaitEvent(cstream, cev[2], 0));
        MI_NCCL_CHECK(ncclAllReduce(mt, mt, (size_t) (d * ex.KM), nccl_type<T>(), ncclSum, comm, cstream));
        MI_HIP_CHECK(hipEventRecord(cev[3], cstream));
        MI_HIP_CHECK(hipStreamWaitEvent(stream, cev[1], 0));  // w of every rank
        if (g16) {  // S from the ranks' partials, in rank order
            launch_dot_final<T>(sg, sc.get(), FIN_PLAIN, 0, nullptr, 0, csr.ssc.get(), stream, G);
        } else {
            hipLaunchKernelGGL(exp_wsum_kernel<T>, dim3(RED_BLOCKS), dim3(256), 0, stream, w, m,
                               ex.hbf16 ? ex.wv16.get() : nullptr, cw, red.get(), status);  // S = sum_j w_j (+ bf16 w)
            MI_LAUNCH_CHECK();
            launch_dot_final<T>(red.get(), sc.get(), FIN_PLAIN, 0, nullptr, 0, csr.ssc.get(), stream);
        }
        expansion_dominant(w, status);
        MI_HIP_CHECK(hipStreamWaitEvent(stream, cev[3], 0));  // the group's moments
        if (!fused) expansion_mscale(status);
    } else if (g16) {
        // S from w's partials: inside the moment reduce when the moment pass has one (one launch fewer)
        const bool sfold = d > 0 && expansion_moments_fused();
        if (!sfold) launch_dot_final<T>(spt, sc.get(), FIN_PLAIN, 0, nullptr, 0, csr.ssc.get(), stream);
        expansion_moments(w, status, sfold ? spt : nullptr, 1);
        expansion_dominant(w, status);
    } else {
        gather_input(w);
        if (!wown_all) {
            hipLaunchKernelGGL(exp_wsum_kernel<T>, dim3(RED_BLOCKS), dim3(256), 0, stream, w, m,
                               ex.hbf16 ? ex.wv16.get() : nullptr, cw, red.get(), status);  // S = sum_j w_j (+ bf16 w)
            MI_LAUNCH_CHECK();
        }
        const bool sfold = d > 0 && expansion_moments_fused();
        if (!sfold) launch_dot_final<T>(spt, sc.get(), FIN_PLAIN, 0, nullptr, 0, csr.ssc.get(), stream);
        expansion_moments(w, status, sfold ? spt : nullptr, 1);
        expansion_dominant(w, status);
    }
    T kappa = 0;
    if (kernel == 1 && !ctr_now) {
        kappa = 1;
        for (int q2 = 0; q2 < degree; ++q2) kappa *= coef0;
    }
    const T *cb = ctr_now && kernel == 2 ? ctr_c.get() : nullptr;
    // J_i = sum_{f in x_i} sum_k x_if^(k+1) M[f][k]: one SELL pass over this rank's CSR rows (mode 2)
    // (few panels: the combine sums the pass's panel slabs itself, one launch fewer)
    const auto &pc = csr.spmv_csr;
    const bool jfuse = pc.P > 1 && pc.P < 16 && pc.nseg == r1 - r0 && pc.nblocks > 0;
    if (r1 > r0) launch_panel_spmv<T>(pc, ex.M.get(), d, raw.get() + r0, status, stream, ex.KM, 2, !jfuse);
    // a CG iteration on its own rows (one GPU, or a sharded rank): the combine and the iteration's finalize in
    // one launch (the gathered partials it needs are in place: carried by the K·p's collective or flushed here)
    if (kp_fin_req != nullptr && with_base && r1 > r0 && ib == r0 && ie == r1 && ib == v0 && ie - ib == vn &&
        (shard || (world == 1 && sim_world == 0))) {
        flush_psum();
        const kp_fin_t &f = *kp_fin_req;
        auto fin = [&](auto kern, auto dg) {
            hipLaunchKernelGGL(kern, dim3(RED_BLOCKS), dim3(cgk::CG_NT), 0, stream,
                               kernel == 2 ? csr.e.get() : nullptr, cb, w, ex.hdiag.get(), ex.hs.get(),
                               ex.G > 1 ? ex.hslab.get() : nullptr, ex.G, jfuse ? pc.partial.get() : nullptr, (int) pc.P,
                               raw.get(), csr.ssc.get(), kappa, r0, r1, f.q, f.d, f.psum, f.G, f.QA_cost, dg, f.Ad,
                               f.pdad, sc.get());
        };
        if (f.sinv == nullptr) fin(exp_combine_fin_kernel<T, T>, f.cost_inv);
        else fin(exp_combine_fin_kernel<T, row_diag<T>>, row_diag<T>{ f.cost_inv, f.sinv });
        MI_LAUNCH_CHECK();
        kp_fin_done = true;
        return;  // sharded (or one rank): nothing to gather
    }
    if (ie > ib)
        hipLaunchKernelGGL(exp_combine_kernel<T>, dim3((unsigned) ceil_div(ie - ib, 256)), dim3(256), 0, stream,
                           kernel == 2 ? csr.e.get() : nullptr, cb, w, ex.hdiag.get(), ex.phin.get(), ex.hs.get(),
                           ex.G > 1 ? ex.hslab.get() : nullptr, ex.G, jfuse ? pc.partial.get() : nullptr, (int) pc.P,
                           csr.ssc.get(), kappa, ib, ie, r0, r1, with_base ? 0 : (part_mode == 2 ? 2 : 1), raw.get(), status);
    MI_LAUNCH_CHECK();
    if (!shard) allgather_rows(raw.get());
}

// ---- centered rank-1 terms of the finalize (engine.hpp ctr_*) -------------------------------------------------
// per row i < m, in fp64 from the row's entries and the last point x_m (dense, xlast):
//   rbf:  c_i = e_i - e_m = e_m expm1(gamma (|x_m|^2 - |x_i|^2)),  cw_i = c_i / e_i = -expm1(gamma (|x_i|^2 - |x_m|^2)),
//         h_i = e_i e_m expm1(2 gamma x_i.x_m)
//   poly: h_i = (gamma x_i.x_m + c0)^deg - c0^deg as its binomial sum (no cancellation)
// bad = 1 when a value does not fit the real type (then the plain finalize is used)
template <typename T>
__global__ __launch_bounds__(256) void exp_ctr_kernel(int kernel, int degree, double gamma, double coef0,
                                                      const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      vals_t<T> val, int64_t m, const T *__restrict__ xlast, double nlast,
                                                      const T *__restrict__ norms, double em, T *__restrict__ c,
                                                      T *__restrict__ cw, T *__restrict__ h, int *__restrict__ bad) {
    const int64_t row = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    double s = 0;
    for (int64_t k = rowptr[row]; k < rowptr[row + 1]; ++k) s = fma((double) val[k], (double) xlast[col[k]], s);
    const double lim = sizeof(T) == 4 ? 1e37 : 1e307;
    if (kernel == 2) {
        const double ni = (double) norms[row];
        const double ei = exp(-gamma * ni);
        const double ci = em * expm1(gamma * (nlast - ni)), cwi = -expm1(gamma * (ni - nlast));
        const double hi = ei * em * expm1(2.0 * gamma * s);
        if (!(fabs(cwi) < lim) || !(fabs(hi) < lim)) *bad = 1;
        c[row] = (T) ci;
        cw[row] = (T) cwi;
        h[row] = (T) hi;
    } else {
        const double u = gamma * s;
        double hi = 0, binom = 1, uk = 1;
        for (int k = 1; k <= degree; ++k) {
            binom = binom * (double) (degree - k + 1) / (double) k;
            uk *= u;
            double c0p = 1;
            for (int t = 0; t < degree - k; ++t) c0p *= coef0;
            hi += binom * c0p * uk;
        }
        if (!(fabs(hi) < lim)) *bad = 1;
        h[row] = (T) hi;
    }
}

template <typename T>
bool engine<T>::ctr_active() const {
    return ctr_ok && q_gen && sparse && !csr.dense_on && csr.ex.on && !csr.otf_on && (kernel == 1 || kernel == 2);
}

template <typename T>
T engine<T>::QAf() const {
    if (!ctr_active()) return QA_cost;
    // a caller's QA_cost (plssvm_mi_set_qa_cost) that differs from k_mm + 1/C keeps its difference
    return (T) (ctr_hm + (double) diag_m()) + (QA_cost - (ctr_kmm + diag_m()));
}

template <typename T>
void engine<T>::ctr_setup() {
    ctr_ok = false;
    const char *cv = std::getenv("PLSSVM_MI_CTR");  // read per setup: tests compare both finalizes in one process
    const int mode = cv == nullptr ? 1 : std::atoi(cv);
    if (mode == 0 || !sparse || csr.dense_on || !csr.ex.on || csr.otf_on || (kernel != 1 && kernel != 2) || m <= 0) return;
    double nlast = 0;
    for (int64_t k = 0; k < d; ++k) nlast = std::fma((double) xlast_h[k], (double) xlast_h[k], nlast);
    const double g = (double) gamma, em = std::exp(-g * nlast);
    if (kernel == 2) {
        ctr_hm = -std::expm1(-2.0 * g * nlast);  // e_m^2 expm1(2 gamma |x_m|^2) = 1 - e_m^2
    } else {
        double hm = 0, binom = 1, uk = 1;
        for (int k = 1; k <= degree; ++k) {
            binom = binom * (double) (degree - k + 1) / (double) k;
            uk *= g * nlast;
            double c0p = 1;
            for (int t = 0; t < degree - k; ++t) c0p *= (double) coef0;
            hm += binom * c0p * uk;
        }
        ctr_hm = hm;
    }
    const int64_t len = q.size();
    ctr_h.alloc(len, stream);
    if (kernel == 2) {
        ctr_c.alloc(len, stream);
        ctr_cw.alloc(len, stream);
    }
    dev_buf<int> bad;
    bad.alloc(1, stream);
    hipLaunchKernelGGL(exp_ctr_kernel<T>, dim3((unsigned) ceil_div(m, 256)), dim3(256), 0, stream, kernel, degree, g,
                       (double) coef0, csr.rowptr.get(), csr.col.get(), csr.rvals(), m, xlast.get(), nlast, norms.get(),
                       em, ctr_c.get(), ctr_cw.get(), ctr_h.get(), bad.get());
    MI_LAUNCH_CHECK();
    int hb = 0;
    MI_HIP_CHECK(hipMemcpyAsync(&hb, bad.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
    MI_HIP_CHECK(hipStreamSynchronize(stream));
    ctr_ok = hb == 0;
}

// ---- predict through the expansion (csvm::predict on sparse poly / rbf models) -----------------------
// sum_{i<m} alpha_i k(x_i, z) = base_z (S + J_z + sum_{i sharing >= 2 features with z} w_i H_iz), with
// w = alpha e (rbf) / alpha (poly), S = sum w, J_z = sum_{f in z} sum_k coef_k z_f^k M_k(f) from the
// model's column moments M_k(f) = sum_{i in col f} x_if^k w_i (once per call), and H_iz = phi(s_iz) -
// sum_{f shared} phi(x_if z_f) for the support vectors sharing two or more features with z: per point,
// the CSC columns of z's features are walked with an LDS bitmap of rows (seen once / twice), the repeat
// rows are enumerated in ascending order and their exact s_iz and phi sums formed by merging row i with
// z. Fixed orders throughout: deterministic. O(nnz_z K + sum_{f in z} c_f) per point instead of O(nnz_X).
constexpr int PRED_NT = 1024;
constexpr int PRED_BMW = 24576;             // bitmap words (96 KiB): rows per pass = 786 432
constexpr int PRED_ZCAP = 2048;             // entries of one point held in LDS
constexpr int PRED_MCAP = 4096;             // repeat rows per pass

template <typename T>
__global__ __launch_bounds__(256) void exp_pred_w_kernel(const T *__restrict__ alpha, const T *__restrict__ e, int64_t m,
                                                         T *__restrict__ w) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) w[i] = e != nullptr ? alpha[i] * e[i] : alpha[i];
}

// M[f][k] = coef_{k+1} sum_{t in col f} cval[t]^(k+1) w[crow[t]], one wave per column (lane-strided,
// then a butterfly: fixed order)
template <typename T>
__global__ __launch_bounds__(256) void exp_pred_moments_kernel(const int64_t *__restrict__ colptr,
                                                               const int32_t *__restrict__ crow,
                                                               const T *__restrict__ cval, const T *__restrict__ w,
                                                               int64_t d, int K, int KM, coefs cf, T *__restrict__ M) {
    const int64_t f = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= d) return;
    double acc[EXP_KMAX];
#pragma unroll
    for (int k = 0; k < EXP_KMAX; ++k) acc[k] = 0.0;
    for (int64_t t = colptr[f] + lane; t < colptr[f + 1]; t += 64) {
        const double v = (double) cval[t];
        double pw = v * (double) w[crow[t]];
#pragma unroll
        for (int k = 0; k < EXP_KMAX; ++k) {
            if (k < K) acc[k] += pw;
            pw *= v;
        }
    }
#pragma unroll
    for (int k = 0; k < EXP_KMAX; ++k) {
        if (k < K) {  // K is uniform
            double a = acc[k];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
            if (lane == 0) M[f * KM + k] = (T) (cf.c[k + 1] * a);
        }
    }
    if (lane == 0)
        for (int k = K; k < KM; ++k) M[f * KM + k] = T(0);
}

template <typename T>
__device__ __forceinline__ double pred_block_sum(double v, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w2 = 0; w2 < PRED_NT / 64; ++w2) s += red[w2];
    return s;
}

// one point per workgroup, nc <= NC classes per launch: the walk, the bitmap, the enumeration and the merge that
// forms s_iz and the phi sum do not depend on the class and run once; only w_c[i] H_iz, the Horner sum over class
// c's moments and the closing expression run per class, each in the single-class order (row c is bitwise the
// nc = 1 launch). zr/zc/zv: the points' CSR (columns ascending); class c: w + c ldw, M + c ldm, S[2 c] (sum w),
// am[c] (alpha_m) and bias[c], out + c ldo. flag[0] set when a pass held more than PRED_MCAP repeat rows (the
// caller then recomputes brute force)
template <typename T, int NC>
__global__ __launch_bounds__(PRED_NT) void exp_pred_point_kernel(
    const int64_t *__restrict__ zr, const int32_t *__restrict__ zc, const T *__restrict__ zv, const int64_t *__restrict__ colptr,
    const int32_t *__restrict__ crow, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const T *__restrict__ val, const T *__restrict__ w, int64_t ldw, const T *__restrict__ M, int64_t ldm, int KM,
    phi_fn phi, int64_t m, const T *__restrict__ S, const T *__restrict__ xlast, T nlast, const T *__restrict__ am,
    kfun<T> kf, T kappa, const T *__restrict__ bias, int nc, T *__restrict__ out, int64_t ldo, int *__restrict__ flag) {
    __shared__ uint32_t bm[PRED_BMW];
    __shared__ int32_t zcol_s[PRED_ZCAP];
    __shared__ T zval_s[PRED_ZCAP];
    __shared__ int32_t multi[PRED_MCAP];
    __shared__ int64_t zoff[PRED_ZCAP + 1];
    __shared__ double red[PRED_NT / 64];
    __shared__ int nmulti, wcnt[PRED_NT];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int64_t e0 = zr[p];
    const int nz = (int) (zr[p + 1] - e0);
    // the point's entries, x_m at its columns and its columns' CSC lengths: one parallel read each (a serial
    // loop of dependent global reads in one thread cost ~1 us per entry); x_m's values borrow the bitmap's LDS,
    // which every pass below clears before use
    static_assert(PRED_ZCAP * sizeof(T) <= PRED_BMW * sizeof(uint32_t), "x_m staging must fit the bitmap");
    T *xl_s = reinterpret_cast<T *>(bm);
    for (int e = tid; e < nz; e += PRED_NT) {
        const int32_t f = zc[e0 + e];
        zcol_s[e] = f;
        zval_s[e] = zv[e0 + e];
        xl_s[e] = xlast[f];
        zoff[e + 1] = colptr[f + 1] - colptr[f];
    }
    __syncthreads();
    // |z|^2 (column order) and x_m . z (entry order), thread 0, from LDS
    if (tid == 0) {
        T nzz = 0, dl = 0;
        for (int e = 0; e < nz; ++e) {
            nzz = fma(zval_s[e], zval_s[e], nzz);
            dl = fma(xl_s[e], zval_s[e], dl);
        }
        red[0] = (double) nzz;
        red[1] = (double) dl;
        // CSC offsets of z's columns (flattened incidences)
        zoff[0] = 0;
        for (int e = 0; e < nz; ++e) zoff[e + 1] += zoff[e];
    }
    __syncthreads();
    const T nzz = (T) red[0], dl = (T) red[1];
    const int64_t inc = zoff[nz];
    // J_z = sum_e z_e (M0 + z_e (M1 + ...)) in the real type's Horner order, per class
    double J[NC], hs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        J[c] = 0.0;
        hs[c] = 0.0;
        if (c < nc) {  // uniform
            double js = 0.0;
            for (int e = tid; e < nz; e += PRED_NT) {
                const T z = zval_s[e];
                const T *Mf = M + c * ldm + (int64_t) zcol_s[e] * KM;
                T h = Mf[KM - 1];
                for (int k = KM - 2; k >= 0; --k) h = fma(h, z, Mf[k]);
                js += (double) (h * z);
            }
            J[c] = pred_block_sum<T>(js, red);
        }
    }
    const int64_t BMBITS = (int64_t) PRED_BMW * 32;
    for (int64_t R0 = 0; R0 < m; R0 += BMBITS) {
        const int64_t R1 = min(m, R0 + BMBITS);
        for (int q = tid; q < PRED_BMW; q += PRED_NT) bm[q] = 0u;
        if (tid == 0) nmulti = 0;
        __syncthreads();
        // rows seen once -> bit set; seen again -> appended (duplicates for 3+ shared features)
        for (int64_t t = tid; t < inc; t += PRED_NT) {
            int lo = 0, hi = nz - 1;  // entry e with zoff[e] <= t < zoff[e + 1]
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (zoff[mid] <= t) lo = mid;
                else hi = mid - 1;
            }
            const int64_t i = crow[colptr[zcol_s[lo]] + (t - zoff[lo])];
            if (i < R0 || i >= R1) continue;
            const uint32_t bit = 1u << ((i - R0) & 31);
            const uint32_t old = atomicOr(&bm[bm_addr<PRED_BMW / PRED_NT, PRED_NT>((i - R0) >> 5)], bit);
            if (old & bit) {
                const int q = atomicAdd(&nmulti, 1);
                if (q < PRED_MCAP) multi[q] = (int32_t) i;
            }
        }
        __syncthreads();
        const int nm = nmulti;
        if (nm > PRED_MCAP) {
            if (tid == 0) flag[0] = 1;
            return;  // uniform: every thread read the same nmulti
        }
        // the repeat rows as a set in the bitmap, then enumerated in ascending row order
        for (int q = tid; q < PRED_BMW; q += PRED_NT) bm[q] = 0u;
        __syncthreads();
        for (int q = tid; q < nm; q += PRED_NT) {
            const int64_t i = multi[q] - R0;
            atomicOr(&bm[bm_addr<PRED_BMW / PRED_NT, PRED_NT>(i >> 5)], 1u << (i & 31));
        }
        __syncthreads();
        constexpr int WPT = PRED_BMW / PRED_NT;
        int c = 0;
        for (int q = 0; q < WPT; ++q) c += __popc(bm[q * PRED_NT + tid]);
        // exclusive block scan of the counts (wave scans, then the wave totals), not a serial loop over 1024
        const int lane = tid & 63, wave = tid >> 6;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wcnt[wave] = incl;
        __syncthreads();
        int before = 0, tot = 0;
        for (int w2 = 0; w2 < PRED_NT / 64; ++w2) {
            const int v = wcnt[w2];
            if (w2 < wave) before += v;
            tot += v;
        }
        if (tid == 0) nmulti = tot;
        {
            int pos = before + incl - c;
            for (int q = 0; q < WPT; ++q) {
                uint32_t word = bm[q * PRED_NT + tid];
                while (word) {
                    const int b = __ffs(word) - 1;
                    word &= word - 1;
                    multi[pos++] = (int32_t) (R0 + (int64_t) (tid * WPT + q) * 32 + b);
                }
            }
        }
        __syncthreads();
        const int U = nmulti;
        // H_iz = phi(s) - sum phi(x_if z_f) over the shared features (fp64), times w_i
        for (int q = tid; q < U; q += PRED_NT) {
            const int64_t i = multi[q];
            double sdot = 0.0, sphi = 0.0;
            for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
                const int32_t f = col[k];
                int lo = 0, hi = nz - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (zcol_s[mid] < f) lo = mid + 1;
                    else hi = mid;
                }
                if (nz > 0 && zcol_s[lo] == f) {
                    const double a = (double) val[k] * (double) zval_s[lo];
                    sdot += a;
                    sphi += phi(a);
                }
            }
            const double hiz = phi(sdot) - sphi;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nc) hs[c] += (double) w[c * ldw + i] * hiz;
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < nc) hs[c] = pred_block_sum<T>(hs[c], red);
    if (tid == 0) {
        // the last training point (kept apart, as the reference's data_last)
        T kl;
        if (kf.kernel == 1) {
            const T base = fma(kf.gamma, dl, kf.coef0);
            kl = T(1);
            for (int e = 0; e < kf.degree; ++e) kl *= base;
        } else {
            T dist = nlast + nzz - T(2) * dl;
            dist = dist > T(0) ? dist : T(0);
            kl = exp(-kf.gamma * dist);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < nc) {
                double v;
                if (phi.rbf) {
                    const double ez = exp(-(double) kf.gamma * (double) nzz);
                    v = ez * ((double) S[2 * c] + J[c] + hs[c]);
                } else {
                    v = (double) kappa * (double) S[2 * c] + J[c] + hs[c];
                }
                out[c * ldo + p] = (T) (v + (double) (am[c] * kl)) + bias[c];
            }
        }
    }
}

// predict nclass models through the expansion, at most KP_MULTI_W classes per pass over the points; false when it
// does not apply (the caller predicts brute force). Every condition depends on the points and the model's data
// alone, so the decision holds for all classes together. alpha_dev: [nclass][lda]; ab_dev: the classes' alpha_m,
// then their biases; out_dev: [nclass][ldo]
template <typename T>
bool engine<T>::expansion_predict(const T *alpha_dev, int64_t lda, int64_t nclass, const T *ab_dev, const int64_t *zr_dev,
                                  const int32_t *zc_dev, const T *zv_dev, int64_t np, int64_t max_nnz_z, double zabs_max,
                                  double znorm_max, T nlast, T *out_dev, int64_t ldo) {
    auto &ex = csr.ex;
    if (!ex.on || kernel == 0 || m <= 0 || max_nnz_z > PRED_ZCAP) return false;
    if (std::getenv("PLSSVM_MI_PRED_BRUTE") != nullptr) return false;
    // the model's Taylor degree covers |2 g x z| up to umax; the factored rbf form |z|^2 in range
    // (|2 g x z| <= umax = 2 |g| max x^2 for every x of the model iff max z^2 <= max x^2; formed like umax, so points
    // whose largest |z| equals the model's largest |x| stay in range exactly — through sqrt(umax / 2 |g|) the
    // comparison rounded either way there)
    if (kernel == 2 && 2.0 * std::fabs((double) gamma) * (zabs_max * zabs_max) > ex.umax) return false;
    if (kernel == 2 && std::fabs((double) gamma) * znorm_max > (sizeof(T) == 8 ? 300.0 : 40.0)) return false;
    const phi_fn phi = make_phi<T>(kernel, degree, gamma, coef0);
    const int ncp = (int) std::min<int64_t>(nclass, KP_MULTI_W);  // classes per pass
    const int64_t ldw = std::max<int64_t>(m, 1), ldm = std::max<int64_t>(d, 1) * ex.KM;
    dev_buf<T> wv, Md, Sd;
    wv.alloc(ncp * ldw, stream, false);
    Md.alloc(ncp * ldm, stream, false);
    Sd.alloc(2 * ncp, stream);
    coefs cf;
    std::memcpy(cf.c, ex.coef, sizeof(cf.c));
    T kappa = 0;
    if (kernel == 1) {
        kappa = 1;
        for (int q2 = 0; q2 < degree; ++q2) kappa *= coef0;
    }
    dev_buf<int> flag;
    flag.alloc(1, stream);
    for (int64_t c0 = 0; c0 < nclass; c0 += ncp) {
        const int nc = (int) std::min<int64_t>(ncp, nclass - c0);
        // w_c, S_c and M_c per class: O(nnz)
        for (int c = 0; c < nc; ++c) {
            T *wc = wv.get() + c * ldw;
            hipLaunchKernelGGL(exp_pred_w_kernel<T>, dim3((unsigned) ceil_div(m, 256)), dim3(256), 0, stream,
                               alpha_dev + (c0 + c) * lda, kernel == 2 ? csr.e.get() : nullptr, m, wc);
            MI_LAUNCH_CHECK();
            launch_dot2<T>(wc, nullptr, nullptr, nullptr, m, red.get(), nullptr, stream);
            launch_dot_final<T>(red.get(), sc.get(), FIN_PLAIN, 0, nullptr, 0, Sd.get() + 2 * c, stream);
            if (d > 0)
                hipLaunchKernelGGL(exp_pred_moments_kernel<T>, dim3((unsigned) ceil_div(d, 4)), dim3(256), 0, stream,
                                   csr.colptr.get(), csr.crow.get(), csr.cval.get(), wc, d, ex.K, ex.KM, cf,
                                   Md.get() + c * ldm);
            MI_LAUNCH_CHECK();
        }
        auto point_kernel = nc == 1 ? exp_pred_point_kernel<T, 1> : exp_pred_point_kernel<T, KP_MULTI_W>;
        hipLaunchKernelGGL(point_kernel, dim3((unsigned) np), dim3(PRED_NT), 0, stream, zr_dev, zc_dev, zv_dev,
                           csr.colptr.get(), csr.crow.get(), csr.rowptr.get(), csr.col.get(), csr.val.get(), wv.get(), ldw,
                           Md.get(), ldm, ex.KM, phi, m, Sd.get(), xlast.get(), nlast, ab_dev + c0, kf(), kappa,
                           ab_dev + nclass + c0, nc, out_dev + c0 * ldo, ldo, flag.get());
        MI_LAUNCH_CHECK();
        int hf = 0;
        MI_HIP_CHECK(hipMemcpyAsync(&hf, flag.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        if (hf != 0) return false;  // PRED_MCAP overflow: a property of the points, the same in every pass
    }
    return true;
}

int exp_dot2_built() { return EXP_DOT2 ? 1 : 0; }

void exp_load_code_object() {
    hipFuncAttributes a;
    (void) hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&exp_w_kernel<float>));
    exp_setup_load_code_object();
}

#define INST(T)                                                                              \
    template void engine<T>::expansion_dominant(const T *, const cg_scalars<T> *);           \
    template void engine<T>::expansion_moments(const T *, const cg_scalars<T> *, const T *, int);            \
    template void engine<T>::expansion_mscale(const cg_scalars<T> *);                        \
    template bool engine<T>::expansion_moment_pass(const T *, const cg_scalars<T> *, const T *, int);         \
    template bool engine<T>::expansion_moments_fused() const;        \
    template coefs engine<T>::expansion_coefs() const;                                       \
    template void engine<T>::expansion_kp_raw(const T *, const cg_scalars<T> *, bool);      \
    template bool engine<T>::dir_w_fill(dir_w_t<T> &);                                        \
    template bool engine<T>::ctr_active() const;                                              \
    template T engine<T>::QAf() const;                                                        \
    template void engine<T>::ctr_setup();                                                     \
    template bool engine<T>::expansion_predict(const T *, int64_t, int64_t, const T *, const int64_t *, const int32_t *, \
                                               const T *, int64_t, int64_t, double, double, T, T *, int64_t);
INST(float)
INST(double)
#undef INST

}  // namespace plssvm_mi
