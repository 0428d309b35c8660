// Gamma lanes of the dense K·p: one pass over the implicit 128 x 128 tiles for up to KP_MULTI_W
// (gamma_l, p_l) pairs of the RBF or the Laplacian kernel.
//
// Both kernels are exp(-gamma dist_ij), and nearly all of a tile's work is dist_ij: the Gram block on MFMA plus the
// norms (RBF), or the VALU L1 chain (Laplacian). kp_gamma_kernel forms the tile's distances once, exactly as
// kp_tile_kernel's KP_COMPUTE mode does (same tiling, same LDS panels and DMA order, same accumulator ownership, the RBF
// centring included: it is in the data), and keeps them in the accumulator registers. Then one turn per live lane:
// the lane's p_I / p_J are staged in the 256 LDS slots where the single kernel keeps them, every value goes through
// the single kernel's kernel-function call with gamma_l and straight into its two fma chains (times p_j: row sums,
// times p_i: mirrored column sums), the partials are parked in the reduction buffers that overlay the panels and summed
// in the single kernel's fixed order into the tile's record of slab l. Nothing but gamma differs from the single
// kernel's epilogue, so slab l is BITWISE the slab launch_kp_tiles writes for p_l on a context created with gamma_l
// (stored or implicit tiles alike). No atomics, no tile store. A lane whose stop flag says converged is skipped.
//
// Registers: the distances stay live across the turns (fp64: 128 VGPRs), a turn needs the single epilogue's
// temporaries on top. That does not fit the 168 VGPRs of three workgroups per CU in fp64, and a spill inside the lane
// loop would be paid once per lane, so both fp64 instances run 2 workgroups per CU (256 VGPRs); fp32 keeps 3. LDS is
// the single kernel's: the lanes add none (one lane's p at a time), so the fp64 Laplacian instance stays at 2 per CU.
#include "kernels.hpp"
#include "kp_device.hpp"

namespace plssvm_mi {

namespace {

// (kp_gammas / kp_gamma_at, the lanes' gammas in the kernel arguments: kp_device.hpp; LW = 1 has no lane loop and no
// stop-flag mask)
template <typename T>
constexpr int kpg_waves() { return sizeof(T) == 8 ? 2 : 3; }

// KERNEL: 2 (RBF) or KF_LAPLACIAN; kf carries the kernel id only (its gamma is not read). Vector c is p + c * pstride,
// its slab partial + c * sstride, its stop flag status[c] (null: none). The geometry arguments are kp_tile_kernel's.
template <typename T, int KERNEL, int LW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kpg_waves<T>(), kpg_waves<T>()))) void kp_gamma_kernel(
    kfun<T> kf, kp_gammas<T, LW> gam, const T *__restrict__ XT, const T *__restrict__ norms, const T *__restrict__ p,
    T *__restrict__ partial, int64_t n_pad, int64_t d_pad, int64_t nb, int64_t s0, int64_t nsuper,
    const int32_t *__restrict__ wg_off, const cg_scalars<T> *__restrict__ status, int nvec, int64_t pstride, int64_t sstride) {
    static_assert(KERNEL == 2 || KERNEL == KF_LAPLACIAN, "gamma lanes: kernels of the form exp(-gamma dist)");
    using M = mfma16<T>;
    using acc_t = typename M::acc_t;
    constexpr int BK = kp_bk<T, KERNEL>();
    constexpr int PANEL = BK * KP_TILE;          // elements of one [BK][128] panel
    constexpr int EPP = 1024 / (int) sizeof(T);  // elements per 1 KiB wave-instruction
    constexpr int PIECES = PANEL / EPP / 4;      // wave-instructions per wave per panel
    constexpr int VEC = 16 / (int) sizeof(T);
    // LDS as in kp_tile_kernel: p_I, p_J, n_I, n_J, the two double-buffered panel pairs, overlaid by the reduction buffers
    constexpr int OFF_PAN = KP_OFF_PAN;
    constexpr int RSTR = KP_RSTR, RHALF = KP_RHALF, CSTR = KP_CSTR;
    constexpr int RED = 2 * RHALF + 2 * KP_TILE * CSTR;
    constexpr int SMEM = OFF_PAN + (4 * PANEL > RED ? 4 * PANEL : RED);
    __shared__ __attribute__((aligned(16))) T smem[SMEM];
    constexpr bool FAST_EXP = (KERNEL == 2) && sizeof(T) == 8;
    __shared__ double exp_tab[FAST_EXP ? EXP_TAB : 1];

    unsigned live = 0;  // bit c = lane c is still iterating
    for (int c = 0; c < (LW < nvec ? LW : nvec); ++c)
        if (status == nullptr || !status[c].converged) live |= 1u << c;
    if (live == 0) return;

    // one workgroup per real tile, found as in kp_tile_kernel
    const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
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

    // ---- the tile's distances: kp_tile_kernel's KP_COMPUTE prologue and K loop ----
    acc_t acc[4][4];
    {
        const T nin = (KERNEL == 2) ? norms[pidx] : T(0);
        // fast fp64 RBF: the accumulators start at -n_j / 2, so they end at g_ij - n_j / 2 (gamma enters in the epilogue)
        T acc0[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            acc0[nt] = FAST_EXP ? T(-0.5) * norms[J0 + wc * 64 + nt * 16 + (lane & 15)] : T(0);
        uint32_t doff[PIECES];
#pragma unroll
        for (int j = 0; j < PIECES; ++j) {
            const int elem = (w * PIECES + j) * EPP + lane * VEC;
            doff[j] = (uint32_t) (((int64_t) (elem / KP_TILE) * n_pad + elem % KP_TILE) * (int64_t) sizeof(T));
        }
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
                L1_CHUNK(T, BK, A, B, wr, wc, lane, acc, if (kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1)));
            } else {
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

    // ---- one turn per live lane: kp_tile_kernel's single-vector epilogue with the lane's gamma, p and slab ----
    const T *pI = smem, *pJ = smem + KP_TILE, *nI = smem + 2 * KP_TILE, *nJ = smem + 3 * KP_TILE;
    T nj[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) nj[nt] = (KERNEL == 2 && !FAST_EXP) ? nJ[wc * 64 + nt * 16 + (lane & 15)] : T(0);
    T *rowp = smem + OFF_PAN + wc * RHALF;
    const int q = tid >> 1, h = tid & 1;  // row / column q of the tile, half h
    int c = LW == 1 ? 0 : __builtin_ctz(live);
    T pnext = p[c * pstride + pidx];  // the next live lane's element is fetched while this one is multiplied
    while (true) {
        smem[tid] = pnext;  // the previous turn's reads of p_I / p_J lie before its second barrier
        __syncthreads();    // p_c visible; every wave is done with the last K chunk / the previous turn's sums
        const unsigned rest = LW == 1 ? 0u : live >> (c + 1);
        const int cn = rest != 0 ? c + 1 + __builtin_ctz(rest) : -1;
        if (cn >= 0) pnext = p[cn * pstride + pidx];
        const T gamma = kp_gamma_at(gam, c);
        T pj[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) pj[nt] = pJ[wc * 64 + nt * 16 + (lane & 15)];
        T cs[4] = { 0, 0, 0, 0 };
        const T c2 = FAST_EXP ? T(2) * gamma * T(KEXP) : T(0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = wr * 64 + mt * 16 + M::row(lane, r);
                const T pi = pI[il];
                const T ni = nI[il];
                const T ai = FAST_EXP ? -gamma * T(KEXP) * ni : T(0);
                T s = 0;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    T kv;
                    if constexpr (FAST_EXP)
                        kv = (T) exp_scaled_f64(fma(c2, acc[mt][nt][r], ai), exp_tab);
                    else
                        kv = kernel_apply<T>(KERNEL, kf.degree, gamma, kf.coef0, acc[mt][nt][r], ni, nj[nt]);
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

// q_l[i] = exp(-gamma_l dist(x_i, x_last)), i < m, for nvec lanes in one pass over X: q_dense_kernel's distance chain,
// then its exp per lane (bitwise launch_q_dense at gamma_l). Lane l's vector is q + l * qstride.
template <typename T, int KERNEL>
__global__ __launch_bounds__(256) void q_gamma_kernel(kp_gammas<T, KP_MULTI_W> gam, int nvec, const T *__restrict__ XT,
                                                      int64_t n_pad, int64_t d, int64_t m, const T *__restrict__ xlast,
                                                      T *__restrict__ q, int64_t qstride) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    T v = 0;
    if constexpr (KERNEL == 2) {
        for (int64_t k = 0; k < d; ++k) {
            const T diff = XT[k * n_pad + i] - xlast[k];
            v = fma(diff, diff, v);
        }
    } else {
        for (int64_t k = 0; k < d; ++k) v += __builtin_elementwise_abs(XT[k * n_pad + i] - xlast[k]);
    }
#pragma unroll
    for (int l = 0; l < KP_MULTI_W; ++l)
        if (l < nvec) q[l * qstride + i] = exp(-gam.g[l] * v);
}

template <typename T, int KERNEL, int LW>
void launch_kpg(const kp_geom<T> &g, const T *gammas, const T *p, int64_t pstride, T *partial, int64_t sstride, int nvec,
                const cg_scalars<T> *status, hipStream_t s) {
    kp_gammas<T, LW> gam;
    for (int l = 0; l < LW; ++l) gam.g[l] = gammas[l < nvec ? l : nvec - 1];
    hipLaunchKernelGGL((kp_gamma_kernel<T, KERNEL, LW>), dim3((unsigned) g.wgs), dim3(256), 0, s, g.kf, gam, g.XT, g.norms, p,
                       partial, g.n_pad, g.d_pad, g.nb, g.s0, g.nsuper, g.wg_off, status, nvec, pstride, sstride);
    MI_LAUNCH_CHECK();
}

template <typename T, int KERNEL>
void launch_kpg_width(const kp_geom<T> &g, const T *gammas, const T *p, int64_t pstride, T *partial, int64_t sstride,
                      int nvec, const cg_scalars<T> *status, hipStream_t s) {
    if (nvec == 1) launch_kpg<T, KERNEL, 1>(g, gammas, p, pstride, partial, sstride, nvec, status, s);
    else if (nvec == 2) launch_kpg<T, KERNEL, 2>(g, gammas, p, pstride, partial, sstride, nvec, status, s);
    else if (nvec <= 4) launch_kpg<T, KERNEL, 4>(g, gammas, p, pstride, partial, sstride, nvec, status, s);
    else launch_kpg<T, KERNEL, 8>(g, gammas, p, pstride, partial, sstride, nvec, status, s);
}

}  // namespace

template <typename T>
void launch_kp_tiles_gamma(const kp_geom<T> &g, const T *gammas, const T *p, int64_t pstride, T *partial, int64_t sstride,
                           int nvec, const cg_scalars<T> *status, hipStream_t s) {
    if (g.nsuper <= 0 || g.nb <= 0 || g.wgs <= 0) return;
    if (nvec < 1 || nvec > KP_MULTI_W) throw mi_error(-1, "bad lane count for the gamma tile kernel");
    // 32-bit DMA offsets inside a chunk, as for kp_tile_kernel
    if ((int64_t) kp_dpad<T>() * g.n_pad * (int64_t) sizeof(T) >= ((int64_t) 1 << 31))
        throw mi_error(-5, "too many points for the pairwise tile kernel's 32-bit chunk offsets");
    if (g.kf.kernel == 2) launch_kpg_width<T, 2>(g, gammas, p, pstride, partial, sstride, nvec, status, s);
    else if (g.kf.kernel == KF_LAPLACIAN) launch_kpg_width<T, KF_LAPLACIAN>(g, gammas, p, pstride, partial, sstride, nvec, status, s);
    else throw mi_error(-5, "gamma lanes exist for the rbf and the laplacian kernel");
}

template <typename T>
void launch_q_gammas(int kernel, const T *gammas, int nvec, const T *XT, int64_t n_pad, int64_t d, int64_t m, const T *xlast,
                     T *q, int64_t qstride, hipStream_t s) {
    if (m <= 0) return;
    if (nvec < 1 || nvec > KP_MULTI_W) throw mi_error(-1, "bad lane count for the gamma q kernel");
    kp_gammas<T, KP_MULTI_W> gam;
    for (int l = 0; l < KP_MULTI_W; ++l) gam.g[l] = gammas[l < nvec ? l : nvec - 1];
    const dim3 grid((unsigned) ceil_div(m, 256)), block(256);
    if (kernel == 2) hipLaunchKernelGGL((q_gamma_kernel<T, 2>), grid, block, 0, s, gam, nvec, XT, n_pad, d, m, xlast, q, qstride);
    else if (kernel == KF_LAPLACIAN)
        hipLaunchKernelGGL((q_gamma_kernel<T, KF_LAPLACIAN>), grid, block, 0, s, gam, nvec, XT, n_pad, d, m, xlast, q, qstride);
    else throw mi_error(-5, "gamma lanes exist for the rbf and the laplacian kernel");
    MI_LAUNCH_CHECK();
}

#define INST(T)                                                                                                       \
    template void launch_kp_tiles_gamma<T>(const kp_geom<T> &, const T *, const T *, int64_t, T *, int64_t, int,      \
                                           const cg_scalars<T> *, hipStream_t);                                       \
    template void launch_q_gammas<T>(int, const T *, int, const T *, int64_t, int64_t, int64_t, const T *, T *, int64_t, \
                                     hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace plssvm_mi
