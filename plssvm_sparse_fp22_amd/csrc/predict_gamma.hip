// Gamma lanes of the fused dense predict: the decision values of up to KP_MULTI_W models of the RBF or
// the Laplacian kernel, each with its own width gamma_l and its own alpha_l, in one pass over the pair distances.
//
//     out[l][p] = ((sum_{j < m} alpha_l[j] exp(-gamma_l dist(x_j, z_p))) + alpha_l[m] exp(-gamma_l dist(x_m, z_p))) + bias_l
//
// Both kernels are exp(-gamma dist), and dist — the Gram block on MFMA plus the norms (RBF), the L1 chain on the VALU
// (Laplacian) — is nearly all of a predict tile's work and does not depend on gamma. predict_gamma_kernel is
// predict_tile_kernel (predict_tiles.hip) up to the end of the K loop: the same work unit (a 128-point tile x a segment
// of PRED_SEG support-vector tiles), workgroup mapping, LDS panels, DMA order and accumulator ownership, the fp64 RBF
// accumulators starting at -n_j / 2. Where the single kernel then applies the kernel function in place and takes one
// turn per class, this kernel leaves the DISTANCES in the accumulator registers and takes one turn per lane: alpha_l of
// the tile's support vectors is staged in LDS (the next lane's prefetched under the turn), every distance goes through
// the single kernel's kernel-function expression with gamma_l and straight into its fma chain in (mt, r, nt) order, the
// 32 partials of a point are parked in the row-partial buffers over the panels, summed in the single kernel's fixed
// order and added to run[l][point]. The kernel values of a lane are never kept: 8 lanes x 64 values do not fit, and
// recomputing exp per lane is the point. No atomics; no tile and no value leaves the registers.
//
// Contract: nothing but gamma differs from predict_tile_kernel's arithmetic, so row l is BITWISE what a context
// created with gamma_l predicts with (alpha_l, bias_l), and it depends on nothing else — not on the number of lanes,
// the lane's position, the points' number or order, the chunking or the run. Lanes equal in gamma are not merged.
//
// Registers: the distances stay live across the turns (fp64: 128 VGPRs) under a turn's temporaries, so the fp64
// instances run 2 workgroups per CU (256 VGPRs) and fp32 keeps 3, as kp_gamma_kernel. LDS is the single kernel's.
// The file is built without the packed fp32 instructions, like kp_gamma.hip.
#include "kernels.hpp"
#include "kp_device.hpp"

namespace plssvm_mi {

namespace {

template <typename T>
constexpr int pg_waves() { return sizeof(T) == 8 ? 2 : 3; }
// tiles of a super-block edge, as predict_tile_kernel
constexpr int PG_SUPER = 8;

// KERNEL: 2 (RBF) or KF_LAPLACIAN; kf carries degree / coef0 only (its gamma is not read). Lane l's alpha is
// A + l * n_pad (zero from row m on), its sums go to part[l][segment][point]. The other arguments are predict_tile_kernel's.
template <typename T, int KERNEL, int LW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(pg_waves<T>(), pg_waves<T>()))) void predict_gamma_kernel(
    kfun<T> kf, kp_gammas<T, LW> gam, const T *__restrict__ XT, const T *__restrict__ norms, int64_t n_pad, int64_t nb,
    const T *__restrict__ ZT, const T *__restrict__ znorms, int64_t np_pad, int64_t npt, int64_t nseg, int64_t d_pad,
    const T *__restrict__ A, int nlane, T *__restrict__ part) {
    static_assert(KERNEL == 2 || KERNEL == KF_LAPLACIAN, "gamma lanes: kernels of the form exp(-gamma dist)");
    using M = mfma16<T>;
    using acc_t = typename M::acc_t;
    constexpr int BK = kp_bk<T, KERNEL>();
    constexpr int PANEL = BK * KP_TILE;          // elements of one [BK][128] panel
    constexpr int EPP = 1024 / (int) sizeof(T);  // elements per 1 KiB wave-instruction
    constexpr int PIECES = PANEL / EPP / 4;      // wave-instructions per wave per panel
    constexpr int VEC = 16 / (int) sizeof(T);
    // LDS as in predict_tile_kernel: (unused), alpha_J, n_I (points), n_J (support vectors), the two double-buffered
    // panel pairs, overlaid after the K loop by the row partials [wc][128 points][16 (+1 pad)]
    constexpr int OFF_PAN = 4 * KP_TILE;
    constexpr int RSTR = 17, RHALF = KP_TILE * RSTR + 1;
    constexpr int RED = 2 * RHALF;
    constexpr int SMEM = OFF_PAN + (4 * PANEL > RED ? 4 * PANEL : RED);
    __shared__ __attribute__((aligned(16))) T smem[SMEM];
    __shared__ T run[KP_MULTI_W * KP_TILE];  // running sums [lane][point] of the segment
    constexpr bool FAST_EXP = (KERNEL == 2) && sizeof(T) == 8;
    constexpr bool DMA_LATE = FAST_EXP || KERNEL == KF_LAPLACIAN;  // the next chunk's DMA after this chunk's LDS reads
    __shared__ double exp_tab[FAST_EXP ? EXP_TAB : 1];
    const int nl = LW == 1 ? 1 : (nlane < LW ? nlane : LW);  // live lanes (the launcher keeps 1 <= nlane <= LW)

    // workgroup -> (point tile P, segment S), as predict_tile_kernel
    const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t band = wg / (PG_SUPER * nseg), wb = wg - band * PG_SUPER * nseg;
    const int64_t rows = min<int64_t>(PG_SUPER, npt - band * PG_SUPER);
    const int64_t SS = wb / (rows * PG_SUPER), rem = wb - SS * rows * PG_SUPER;
    const int64_t cols = min<int64_t>(PG_SUPER, nseg - SS * PG_SUPER);
    const int64_t P = band * PG_SUPER + rem / cols, S = SS * PG_SUPER + rem % cols;
    if (P >= npt || S >= nseg) return;  // uniform per workgroup (never taken: the grid is npt * nseg)
    const int64_t I0 = P * KP_TILE;
    const int64_t jb = S * PRED_SEG, je = min<int64_t>(nb, jb + PRED_SEG);

    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w >> 1, wc = w & 1;

    // DMA offsets inside a chunk (32-bit, checked by the launcher): the piece's first row is wave-uniform and goes
    // into the scalar offset with the tile's column offset, the per-lane part is the lane's place inside the piece
    constexpr int RPI = EPP / KP_TILE;
    uint32_t soffI[PIECES], rowJ[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const int64_t row = (int64_t) (w * PIECES + j) * RPI;
        soffI[j] = __builtin_amdgcn_readfirstlane((uint32_t) ((row * np_pad + I0) * (int64_t) sizeof(T)));
        rowJ[j] = __builtin_amdgcn_readfirstlane((uint32_t) (row * n_pad * (int64_t) sizeof(T)));
    }

    for (int i = tid; i < nl * KP_TILE; i += 256) run[i] = T(0);  // visible after the first K-loop barrier
    if (tid < KP_TILE) smem[2 * KP_TILE + tid] = (KERNEL == 2) ? znorms[I0 + tid] : T(0);
    if constexpr (FAST_EXP) {
        if (tid < EXP_TAB) exp_tab[tid] = c_exp2_256[tid];
    }
    const T *aJ = smem + KP_TILE, *nI = smem + 2 * KP_TILE, *nJ = smem + 3 * KP_TILE;
    const int64_t nk = d_pad / BK;

    for (int64_t J = jb; J < je; ++J) {
        const int64_t J0 = J * KP_TILE;
        // ---- the tile's distances: predict_tile_kernel's prologue and K loop (the lane's indices formed anew per tile
        // from a thread id the compiler cannot see through, so that they do not stay live across the K loop) ----
        int tk = tid;
        asm volatile("" : "+v"(tk));
        const int lane = tk & 63;
        const uint32_t vcol = (uint32_t) (((lane * VEC) % KP_TILE) * (int) sizeof(T));
        const uint32_t vrow = (uint32_t) ((lane * VEC) / KP_TILE);
        const uint32_t voffI = RPI == 1 ? vcol : vrow * (uint32_t) (np_pad * (int64_t) sizeof(T)) + vcol;
        const uint32_t voffJ = RPI == 1 ? vcol : vrow * (uint32_t) (n_pad * (int64_t) sizeof(T)) + vcol;
        const uint32_t offJ = __builtin_amdgcn_readfirstlane((uint32_t) (J0 * (int64_t) sizeof(T)));
        // the tile's norms (issued first: their wait must not drain the DMA)
        const T nin = (KERNEL == 2 && tk >= KP_TILE) ? norms[J0 + tk - KP_TILE] : T(0);
        T acc0[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc0[nt] = FAST_EXP ? T(-0.5) * norms[J0 + wc * 64 + nt * 16 + (lane & 15)] : T(0);
        auto issue = [&](int64_t kc, int buf) {
            const T *ca = ZT + kc * BK * np_pad;
            const T *cb = XT + kc * BK * n_pad;
            T *pa = smem + OFF_PAN + (2 * buf) * PANEL;
            T *pb = pa + PANEL;
#pragma unroll
            for (int j = 0; j < PIECES; ++j) {
                const int u = w * PIECES + j;
                glds16_buf(ca, pa + u * EPP, voffI, soffI[j]);
                glds16_buf(cb, pb + u * EPP, voffJ, offJ + rowJ[j]);
            }
        };
        acc_t acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = acc_t{ acc0[b], acc0[b], acc0[b], acc0[b] };

        __syncthreads();  // every wave is done with the previous tile's row partials: the panels may be overwritten
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tk >= KP_TILE) smem[2 * KP_TILE + tk] = nin;

        for (int64_t kc = 0; kc < nk; ++kc) {
            if (kc > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // chunk kc visible to all waves; every wave is done reading chunk kc-1
            if (!DMA_LATE && kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1));
            const T *Ap = smem + OFF_PAN + (2 * (kc & 1)) * PANEL;
            const T *Bp = Ap + PANEL;
            if constexpr (KERNEL == KF_LAPLACIAN) {
                L1_CHUNK(T, BK, Ap, Bp, wr, wc, lane, acc, if (kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1)));
            } else {
                T a[BK / 4][4], b[BK / 4][4];
#pragma unroll
                for (int ks = 0; ks < BK / 4; ++ks) {
                    const int kr = ks * 4 + (lane >> 4);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) a[ks][mt] = Ap[kr * KP_TILE + wr * 64 + mt * 16 + (lane & 15)];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) b[ks][nt] = Bp[kr * KP_TILE + wc * 64 + nt * 16 + (lane & 15)];
                }
                if (DMA_LATE && kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1));
#pragma unroll
                for (int ks = 0; ks < BK / 4; ++ks)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = M::op(a[ks][mt], b[ks][nt], acc[mt][nt]);
            }
        }

        // ---- one turn per lane over the register-resident distances: the single kernel's kernel function with the
        // lane's gamma, its fma chains in (mt, r, nt) order on the lane's alpha, its fixed-order sums ----
        int te = tid;
        asm volatile("" : "+v"(te));
        const int le = te & 63;
        const int q = te >> 1, h = te & 1;  // point q of the tile, half h of its partials
        T anext = te < KP_TILE ? A[J0 + te] : T(0);  // the first lane's alpha of the tile's support vectors
        T nj[4];
        T *rowp = smem + OFF_PAN + wc * RHALF;
        // the lane loop stays rolled: peeled into LW copies (the compiler does that for LW = 4) the turns spill
#pragma unroll 1
        for (int c = 0; c < nl; ++c) {
            if (te < KP_TILE) smem[KP_TILE + te] = anext;  // the previous turn's reads of alpha lie before its second barrier
            __syncthreads();  // alpha_c visible; every wave is done with the last K chunk / the previous turn's sums
            if (c + 1 < nl && te < KP_TILE) anext = A[(int64_t) (c + 1) * n_pad + J0 + te];
            const T gamma = kp_gamma_at(gam, c);
            const T c2 = FAST_EXP ? T(2) * gamma * T(KEXP) : T(0);
            T pj[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                pj[nt] = aJ[wc * 64 + nt * 16 + (le & 15)];
                nj[nt] = (KERNEL == 2 && !FAST_EXP) ? nJ[wc * 64 + nt * 16 + (le & 15)] : T(0);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int il = wr * 64 + mt * 16 + M::row(le, r);
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
                    }
                    rowp[il * RSTR + (le & 15)] = s;
                }
            }
            __syncthreads();
            const T *rp = smem + OFF_PAN + h * RHALF + q * RSTR;
            T a = rp[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) a += rp[k];
            a += __shfl_xor(a, 1);
            if (h == 0) run[c * KP_TILE + q] += a;  // only this thread touches the slot
        }
    }
    if ((tid & 1) == 0) {  // the thread that owns the slots of point tid / 2
        for (int c = 0; c < nl; ++c) part[((int64_t) c * nseg + S) * np_pad + I0 + (tid >> 1)] = run[c * KP_TILE + (tid >> 1)];
    }
}

// predict_finish_kernel with a gamma per lane: out[l][p] = ((sum over the segments, in order, of part[l][s][p]) +
// alpha_l[m] k_l(x_m, z_p)) + bias_l. One thread per point; the last support vector's distance is formed once (the
// single kernel's fma chain x_m . z_p, or its L1 chain), kernel_apply runs per lane. ab as for predict_finish_kernel.
template <typename T, int KERNEL>
__global__ __launch_bounds__(256) void predict_finish_gamma_kernel(kfun<T> kf, kp_gammas<T, KP_MULTI_W> gam,
                                                                   const T *__restrict__ part, int64_t nseg,
                                                                   const T *__restrict__ ZT, const T *__restrict__ znorms,
                                                                   int64_t np_pad, int64_t d, const T *__restrict__ xlast,
                                                                   T nlast, const T *__restrict__ ab, int nlane, int nall,
                                                                   int64_t np, T *__restrict__ out) {
    const int64_t p = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    T dl = 0;
    if constexpr (KERNEL == KF_LAPLACIAN) {
        for (int64_t k = 0; k < d; ++k) dl += __builtin_elementwise_abs(ZT[k * np_pad + p] - xlast[k]);
    } else {
        for (int64_t k = 0; k < d; ++k) dl = fma(xlast[k], ZT[k * np_pad + p], dl);
    }
    const T ni = KERNEL == 2 ? nlast : T(0), nj = KERNEL == 2 ? znorms[p] : T(0);
#pragma unroll
    for (int c = 0; c < KP_MULTI_W; ++c) {
        if (c < nlane) {
            const T kl = kernel_apply<T>(KERNEL, kf.degree, gam.g[c], kf.coef0, dl, ni, nj);
            T s = 0;
            for (int64_t g = 0; g < nseg; ++g) s += part[((int64_t) c * nseg + g) * np_pad + p];
            out[(int64_t) c * np_pad + p] = (s + ab[c] * kl) + ab[nall + c];
        }
    }
}

template <typename T, int KERNEL, int LW>
void launch_pg(kfun<T> kf, const T *gammas, const T *XT, const T *norms, int64_t n_pad, int64_t nb, int64_t d_pad, const T *ZT,
               const T *znorms, int64_t np_pad, int64_t npt, int64_t nseg, const T *A, int nlane, T *part, hipStream_t s) {
    kp_gammas<T, LW> gam;
    for (int l = 0; l < LW; ++l) gam.g[l] = gammas[l < nlane ? l : nlane - 1];
    hipLaunchKernelGGL((predict_gamma_kernel<T, KERNEL, LW>), dim3((unsigned) (npt * nseg)), dim3(256), 0, s, kf, gam, XT, norms,
                       n_pad, nb, ZT, znorms, np_pad, npt, nseg, d_pad, A, nlane, part);
    MI_LAUNCH_CHECK();
}

template <typename T, int KERNEL>
void launch_pg_width(kfun<T> kf, const T *gammas, const T *XT, const T *norms, int64_t n_pad, int64_t nb, int64_t d_pad,
                     const T *ZT, const T *znorms, int64_t np_pad, int64_t npt, int64_t nseg, const T *A, int nlane, T *part,
                     hipStream_t s) {
    if (nlane == 1) launch_pg<T, KERNEL, 1>(kf, gammas, XT, norms, n_pad, nb, d_pad, ZT, znorms, np_pad, npt, nseg, A, nlane, part, s);
    else if (nlane == 2) launch_pg<T, KERNEL, 2>(kf, gammas, XT, norms, n_pad, nb, d_pad, ZT, znorms, np_pad, npt, nseg, A, nlane, part, s);
    else if (nlane <= 4) launch_pg<T, KERNEL, 4>(kf, gammas, XT, norms, n_pad, nb, d_pad, ZT, znorms, np_pad, npt, nseg, A, nlane, part, s);
    else launch_pg<T, KERNEL, 8>(kf, gammas, XT, norms, n_pad, nb, d_pad, ZT, znorms, np_pad, npt, nseg, A, nlane, part, s);
}

}  // namespace

template <typename T>
void launch_predict_tiles_gamma(kfun<T> kf, const T *gammas, const T *XT, const T *norms, int64_t n_pad, int64_t nb,
                                int64_t d_pad, const T *ZT, const T *znorms, int64_t np_pad, int64_t npoints, const T *A,
                                int nlane, T *part, hipStream_t s) {
    if (nb <= 0 || npoints <= 0) return;
    if (nlane < 1 || nlane > KP_MULTI_W) throw mi_error(-1, "bad lane count for the gamma predict tile kernel");
    if (n_pad % KP_TILE != 0 || np_pad % KP_TILE != 0 || d_pad % kp_dpad<T>() != 0 || nb * KP_TILE > n_pad ||
        npoints > np_pad)
        throw mi_error(-1, "bad padding for the predict tile kernel");
    // 32-bit DMA offsets inside a chunk: (BK - 1) rows of the row stride plus the tile's column offset
    if ((int64_t) kp_dpad<T>() * std::max(n_pad, np_pad) * (int64_t) sizeof(T) >= ((int64_t) 1 << 31))
        throw mi_error(-5, "too many points for the predict tile kernel's 32-bit chunk offsets");
    const int64_t npt = ceil_div(npoints, KP_TILE), nseg = predict_segments(nb);
    if (npt * nseg >= ((int64_t) 1 << 31)) throw mi_error(-5, "too many tiles for one predict launch");
    if (kf.kernel == 2)
        launch_pg_width<T, 2>(kf, gammas, XT, norms, n_pad, nb, d_pad, ZT, znorms, np_pad, npt, nseg, A, nlane, part, s);
    else if (kf.kernel == KF_LAPLACIAN)
        launch_pg_width<T, KF_LAPLACIAN>(kf, gammas, XT, norms, n_pad, nb, d_pad, ZT, znorms, np_pad, npt, nseg, A, nlane, part, s);
    else
        throw mi_error(-5, "gamma lanes exist for the rbf and the laplacian kernel");
}

template <typename T>
void launch_predict_finish_gamma(kfun<T> kf, const T *gammas, const T *part, int64_t nseg, const T *ZT, const T *znorms,
                                 int64_t np_pad, int64_t d, const T *xlast, T nlast, const T *ab, int nlane, int nall,
                                 int64_t np, T *out, hipStream_t s) {
    if (np <= 0) return;
    if (nlane < 1 || nlane > KP_MULTI_W) throw mi_error(-1, "bad lane count for the gamma predict finish kernel");
    kp_gammas<T, KP_MULTI_W> gam;
    for (int l = 0; l < KP_MULTI_W; ++l) gam.g[l] = gammas[l < nlane ? l : nlane - 1];
    const dim3 grid((unsigned) ceil_div(np, 256)), block(256);
    if (kf.kernel == 2)
        hipLaunchKernelGGL((predict_finish_gamma_kernel<T, 2>), grid, block, 0, s, kf, gam, part, nseg, ZT, znorms, np_pad, d, xlast,
                           nlast, ab, nlane, nall, np, out);
    else if (kf.kernel == KF_LAPLACIAN)
        hipLaunchKernelGGL((predict_finish_gamma_kernel<T, KF_LAPLACIAN>), grid, block, 0, s, kf, gam, part, nseg, ZT, znorms,
                           np_pad, d, xlast, nlast, ab, nlane, nall, np, out);
    else
        throw mi_error(-5, "gamma lanes exist for the rbf and the laplacian kernel");
    MI_LAUNCH_CHECK();
}

#define INST(T)                                                                                                          \
    template void launch_predict_tiles_gamma<T>(kfun<T>, const T *, const T *, const T *, int64_t, int64_t, int64_t, const T *, \
                                                const T *, int64_t, int64_t, const T *, int, T *, hipStream_t);          \
    template void launch_predict_finish_gamma<T>(kfun<T>, const T *, const T *, int64_t, const T *, const T *, int64_t, int64_t, \
                                                 const T *, T, const T *, int, int, int64_t, T *, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace plssvm_mi
