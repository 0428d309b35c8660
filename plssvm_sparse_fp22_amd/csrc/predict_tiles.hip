// Fused dense poly / RBF predict on MFMA (gfx950): every class of a one-vs-all model in one pass over the kernel values.
//
//     out[c][p] = ((sum_{j < m} alpha_c[j] k(x_j, z_p)) + alpha_c[m] k(x_m, z_p)) + bias_c
//
// The kernel values k(x_j, z_p) do not depend on the class, so a 128 x 128 tile of them (128 points x 128 support
// vectors) is formed once, with kp_tile_kernel's K loop — both panels streamed global -> LDS (glds16_buf), double
// buffered, 2 x 2 waves of 4 x 4 v_mfma_*_16x16x4 accumulators — stays in the accumulator registers, gets the kernel
// function in place and is then multiplied with each class's alpha in turn. Nothing of the tile goes to HBM (the
// rocBLAS path of predict.hip writes and re-reads all m x np dot products, per class).
//
// Work unit: one workgroup = one 128-point tile x one SEGMENT of PRED_SEG consecutive support-vector tiles. The tile
// grid is rectangular (points x support vectors): no triangle, no diagonal case, no mirrored column sums. Per tile and
// class the 32 partials of a point (16 lanes x 2 column-half waves) are parked in LDS and summed in a fixed order, and
// the sum is added to the workgroup's running sum of (class, point), tile after tile; at the end of the segment the
// running sums go to part[class][segment][point]. predict_finish_kernel adds a point's segments in segment order,
// then the last support vector's term and the bias. No atomics.
//
// Contract: the decision value of (class c, point z) depends only on the model (X, alpha_c, bias_c, the kernel
// parameters) and on z — not on the number of classes, the class's position among them, the number of points, the
// point's position in the call, the chunking, or the run. The segment length is a compile-time constant, every point's
// values come from its own row of the tile, and every class's turn is the same code on its own alpha.
//
// Padding: padded support-vector rows have zero XT columns, zero norms and zero alpha; their kernel value is finite
// (poly: coef0^degree, RBF: exp(-gamma |z|^2) <= 1), so its product with alpha = 0 is exactly 0. Padded points are
// computed and never stored.
//
// The Laplacian kernel exp(-gamma ||x - z||_1) has no Gram form: its instance keeps the work units, the DMA, the
// accumulator ownership, the class turns and the sums, and replaces the MFMA K loop by L1 accumulation on the VALU
// (L1_CHUNK, kp_device.hpp). Its padding: zero features add |0 - 0|, a padded support-vector row gives
// exp(-gamma ||z||_1) in (0, 1] times alpha = 0.
#include "kernels.hpp"
#include "kp_device.hpp"

namespace plssvm_mi {

namespace {

// 3 workgroups per CU, as kp_tile_kernel (<= 168 VGPRs, <= 53 KB LDS); -DPRED_TILE_WAVES=2 builds the 2-per-CU
// variant with 256 VGPRs (A/B only)
#ifndef PRED_TILE_WAVES
#define PRED_TILE_WAVES 3
#endif
constexpr int PRED_WAVES = PRED_TILE_WAVES;
// the fp64 Laplacian instance: 2 per CU, as its kp_tile_kernel twin (kp_waves_per_eu: the VALU K loop's registers)
template <typename T, int KERNEL>
constexpr int pred_waves() { return (KERNEL == KF_LAPLACIAN && sizeof(T) == 8) ? 2 : PRED_WAVES; }
// tiles of a super-block edge: 8 point tiles x 8 segments share their panels in one XCD's L2
constexpr int PRED_SUPER = 8;

template <typename T, int KERNEL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(pred_waves<T, KERNEL>(), pred_waves<T, KERNEL>()))) void predict_tile_kernel(
    kfun<T> kf, const T *__restrict__ XT, const T *__restrict__ norms, int64_t n_pad, int64_t nb,
    const T *__restrict__ ZT, const T *__restrict__ znorms, int64_t np_pad, int64_t npt, int64_t nseg, int64_t d_pad,
    const T *__restrict__ A, int ncls, T *__restrict__ part) {
    static_assert(KERNEL == 1 || KERNEL == 2 || KERNEL == KF_LAPLACIAN, "linear predicts through w . z");
    using M = mfma16<T>;
    using acc_t = typename M::acc_t;
    constexpr int BK = kp_bk<T, KERNEL>();
    constexpr int PANEL = BK * KP_TILE;          // elements of one [BK][128] panel
    constexpr int EPP = 1024 / (int) sizeof(T);  // elements per 1 KiB wave-instruction
    constexpr int PIECES = PANEL / EPP / 4;      // wave-instructions per wave per panel
    constexpr int VEC = 16 / (int) sizeof(T);
    // LDS: (unused), alpha_J, n_I (points), n_J (support vectors), then the two double-buffered panel pairs; after
    // the K loop the row partials [wc][128 points][16 (+1 pad)] overlay the panels
    constexpr int OFF_PAN = 4 * KP_TILE;
    constexpr int RSTR = 17, RHALF = KP_TILE * RSTR + 1;
    constexpr int RED = 2 * RHALF;
    constexpr int SMEM = OFF_PAN + (4 * PANEL > RED ? 4 * PANEL : RED);
    __shared__ __attribute__((aligned(16))) T smem[SMEM];
    __shared__ T run[KP_MULTI_W * KP_TILE];  // running sums [class][point] of the segment
    constexpr bool FAST_EXP = (KERNEL == 2) && sizeof(T) == 8;
    constexpr bool DMA_LATE = FAST_EXP || KERNEL == KF_LAPLACIAN;  // the next chunk's DMA after this chunk's LDS reads
    __shared__ double exp_tab[FAST_EXP ? EXP_TAB : 1];

    // workgroup -> (point tile P, segment S): bands of PRED_SUPER point tiles, inside a band super-blocks of
    // PRED_SUPER segments, each XCD walking a contiguous range (speed only; ragged edges give smaller blocks)
    const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t band = wg / (PRED_SUPER * nseg), wb = wg - band * PRED_SUPER * nseg;
    const int64_t rows = min<int64_t>(PRED_SUPER, npt - band * PRED_SUPER);
    const int64_t SS = wb / (rows * PRED_SUPER), rem = wb - SS * rows * PRED_SUPER;
    const int64_t cols = min<int64_t>(PRED_SUPER, nseg - SS * PRED_SUPER);
    const int64_t P = band * PRED_SUPER + rem / cols, S = SS * PRED_SUPER + rem % cols;
    if (P >= npt || S >= nseg) return;  // uniform per workgroup (never taken: the grid is npt * nseg)
    const int64_t I0 = P * KP_TILE;
    const int64_t jb = S * PRED_SEG, je = min<int64_t>(nb, jb + PRED_SEG);

    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w >> 1, wc = w & 1;

    // DMA offsets inside a chunk (32-bit, checked by the launcher). A 1 KiB wave-instruction covers RPI rows of a
    // [BK][128] panel, so the per-lane part is the lane's place inside those rows (fp64: one row, the same for both
    // panels) and the piece's first row is wave-uniform: it goes into the scalar offset with the tile's column offset.
    // kp_tile_kernel keeps a per-lane offset per piece; here the point panel (row stride np_pad) and the
    // support-vector panel (row stride n_pad) would need two sets, and the K loop has no registers to spare.
    constexpr int RPI = EPP / KP_TILE;
    uint32_t soffI[PIECES], rowJ[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const int64_t row = (int64_t) (w * PIECES + j) * RPI;
        soffI[j] = __builtin_amdgcn_readfirstlane((uint32_t) ((row * np_pad + I0) * (int64_t) sizeof(T)));
        rowJ[j] = __builtin_amdgcn_readfirstlane((uint32_t) (row * n_pad * (int64_t) sizeof(T)));
    }

    for (int i = tid; i < ncls * KP_TILE; i += 256) run[i] = T(0);  // visible after the first K-loop barrier
    if (tid < KP_TILE) smem[2 * KP_TILE + tid] = (KERNEL == 2) ? znorms[I0 + tid] : T(0);
    if constexpr (FAST_EXP) {
        if (tid < EXP_TAB) exp_tab[tid] = c_exp2_256[tid];
    }
    const T *aJ = smem + KP_TILE, *nI = smem + 2 * KP_TILE, *nJ = smem + 3 * KP_TILE;
    const int64_t nk = d_pad / BK;

    for (int64_t J = jb; J < je; ++J) {
        const int64_t J0 = J * KP_TILE;
        // The lane's indices and addresses are formed anew for every tile, and again after the K loop, from a thread
        // id the compiler cannot see through: hoisted out of the tile loop they all stay live across the K loop, which
        // then spills operands of its own (scratch reloads behind every chunk barrier, measured 21 % slower).
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
                // kp_tile_kernel's Laplacian K loop: L1 distances on the VALU, feature by feature (L1_CHUNK, kp_device.hpp;
                // rows = points, columns = support vectors), the next chunk's DMA behind the chunk's last LDS reads
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
                // fp64 RBF: the next chunk's DMA after this chunk's LDS reads, every other MFMA instance right after the
                // barrier (kp_tile_kernel's measured order, kp_dma_after_reads)
                if (DMA_LATE && kc + 1 < nk) issue(kc + 1, (int) ((kc + 1) & 1));
#pragma unroll
                for (int ks = 0; ks < BK / 4; ++ks)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = M::op(a[ks][mt], b[ks][nt], acc[mt][nt]);
            }
        }

        int te = tid;
        asm volatile("" : "+v"(te));
        const int le = te & 63;
        const int q = te >> 1, h = te & 1;  // point q of the tile, half h of its partials
        // the first class's alpha of the tile's support vectors: its latency lies under the kernel function
        T anext = te < KP_TILE ? A[J0 + te] : T(0);
        // the kernel function, once, in place (kp_tile_kernel's MULTI epilogue; rows = points, columns = support vectors)
        {
            T nj[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) nj[nt] = (KERNEL == 2 && !FAST_EXP) ? nJ[wc * 64 + nt * 16 + (le & 15)] : T(0);
            const T c2 = FAST_EXP ? T(2) * kf.gamma * T(KEXP) : T(0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const T ni = nI[wr * 64 + mt * 16 + M::row(le, r)];
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

        // one turn per class: alpha_c of the tile's 128 support vectors staged in LDS, the fma chains in (mt, r, nt)
        // order, the 32 partials of each point parked and summed in a fixed order, added to the running sum
        T *rowp = smem + OFF_PAN + wc * RHALF;
        for (int c = 0; c < ncls; ++c) {
            if (te < KP_TILE) smem[KP_TILE + te] = anext;  // the previous turn's reads of alpha lie before its second barrier
            __syncthreads();  // alpha_c visible; every wave is done with the last K chunk / the previous turn's sums
            if (c + 1 < ncls && te < KP_TILE) anext = A[(int64_t) (c + 1) * n_pad + J0 + te];
            T pj[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) pj[nt] = aJ[wc * 64 + nt * 16 + (le & 15)];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int il = wr * 64 + mt * 16 + M::row(le, r);
                    T s = 0;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) s = fma(acc[mt][nt][r], pj[nt], s);
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
        for (int c = 0; c < ncls; ++c) part[((int64_t) c * nseg + S) * np_pad + I0 + (tid >> 1)] = run[c * KP_TILE + (tid >> 1)];
    }
}

// out[c][p] = ((sum over the segments, in order, of part[c][s][p]) + alpha_c[m] k(x_m, z_p)) + bias_c; one thread per
// point, x_m . z_p a sequential fma chain in feature order. ab = [alpha_c[m] for every class | bias_c for every class]
// L1 (the Laplacian kernel): the last support vector's term needs ||x_m - z_p||_1 instead of x_m . z_p and norms
template <typename T, bool L1>
__global__ __launch_bounds__(256) void predict_finish_kernel(kfun<T> kf, const T *__restrict__ part, int64_t nseg,
                                                             const T *__restrict__ ZT, const T *__restrict__ znorms,
                                                             int64_t np_pad, int64_t d, const T *__restrict__ xlast,
                                                             T nlast, const T *__restrict__ ab, int ncls, int nclass,
                                                             int64_t np, T *__restrict__ out) {
    const int64_t p = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    T dl = 0, kl;
    if constexpr (L1) {
        for (int64_t k = 0; k < d; ++k) dl += __builtin_elementwise_abs(ZT[k * np_pad + p] - xlast[k]);
        kl = kernel_apply<T>(KF_LAPLACIAN, kf.degree, kf.gamma, kf.coef0, dl, T(0), T(0));
    } else {
        __builtin_assume(kf.kernel != KF_LAPLACIAN);  // kernel_apply's Laplacian case is the L1 instance's alone
        for (int64_t k = 0; k < d; ++k) dl = fma(xlast[k], ZT[k * np_pad + p], dl);
        kl = kernel_apply<T>(kf.kernel, kf.degree, kf.gamma, kf.coef0, dl, nlast, kf.kernel == 2 ? znorms[p] : T(0));
    }
    for (int c = 0; c < ncls; ++c) {
        T s = 0;
        for (int64_t g = 0; g < nseg; ++g) s += part[((int64_t) c * nseg + g) * np_pad + p];
        out[(int64_t) c * np_pad + p] = (s + ab[c] * kl) + ab[nclass + c];
    }
}

}  // namespace

template <typename T>
void launch_predict_tiles(kfun<T> kf, const T *XT, const T *norms, int64_t n_pad, int64_t nb, int64_t d_pad,
                          const T *ZT, const T *znorms, int64_t np_pad, int64_t npoints, const T *A, int ncls, T *part,
                          hipStream_t s) {
    if (nb <= 0 || npoints <= 0) return;
    if (ncls < 1 || ncls > KP_MULTI_W) throw mi_error(-1, "bad class count for the predict tile kernel");
    if (kf.kernel != 1 && kf.kernel != 2 && kf.kernel != KF_LAPLACIAN)
        throw mi_error(-1, "the predict tile kernel serves the polynomial, rbf and Laplacian kernels");
    if (n_pad % KP_TILE != 0 || np_pad % KP_TILE != 0 || d_pad % kp_dpad<T>() != 0 || nb * KP_TILE > n_pad ||
        npoints > np_pad)
        throw mi_error(-1, "bad padding for the predict tile kernel");
    // 32-bit DMA offsets inside a chunk: (BK - 1) rows of the row stride plus the tile's column offset
    if ((int64_t) kp_dpad<T>() * std::max(n_pad, np_pad) * (int64_t) sizeof(T) >= ((int64_t) 1 << 31))
        throw mi_error(-5, "too many points for the predict tile kernel's 32-bit chunk offsets");
    const int64_t npt = ceil_div(npoints, KP_TILE), nseg = predict_segments(nb);
    if (npt * nseg >= ((int64_t) 1 << 31)) throw mi_error(-5, "too many tiles for one predict launch");
    const dim3 grid((unsigned) (npt * nseg)), block(256);
    if (kf.kernel == 1)
        hipLaunchKernelGGL((predict_tile_kernel<T, 1>), grid, block, 0, s, kf, XT, norms, n_pad, nb, ZT, znorms, np_pad, npt,
                           nseg, d_pad, A, ncls, part);
    else if (kf.kernel == 2)
        hipLaunchKernelGGL((predict_tile_kernel<T, 2>), grid, block, 0, s, kf, XT, norms, n_pad, nb, ZT, znorms, np_pad, npt,
                           nseg, d_pad, A, ncls, part);
    else
        hipLaunchKernelGGL((predict_tile_kernel<T, KF_LAPLACIAN>), grid, block, 0, s, kf, XT, norms, n_pad, nb, ZT, znorms,
                           np_pad, npt, nseg, d_pad, A, ncls, part);
    MI_LAUNCH_CHECK();
}

template <typename T>
void launch_predict_finish(kfun<T> kf, const T *part, int64_t nseg, const T *ZT, const T *znorms, int64_t np_pad,
                           int64_t d, const T *xlast, T nlast, const T *ab, int ncls, int nclass, int64_t np, T *out,
                           hipStream_t s) {
    if (np <= 0 || ncls <= 0) return;
    if (kf.kernel == KF_LAPLACIAN)
        hipLaunchKernelGGL((predict_finish_kernel<T, true>), dim3((unsigned) ceil_div(np, 256)), dim3(256), 0, s, kf, part, nseg,
                           ZT, znorms, np_pad, d, xlast, nlast, ab, ncls, nclass, np, out);
    else
        hipLaunchKernelGGL((predict_finish_kernel<T, false>), dim3((unsigned) ceil_div(np, 256)), dim3(256), 0, s, kf, part, nseg,
                           ZT, znorms, np_pad, d, xlast, nlast, ab, ncls, nclass, np, out);
    MI_LAUNCH_CHECK();
}

#define INST(T)                                                                                                       \
    template void launch_predict_tiles<T>(kfun<T>, const T *, const T *, int64_t, int64_t, int64_t, const T *, const T *, \
                                          int64_t, int64_t, const T *, int, T *, hipStream_t);                        \
    template void launch_predict_finish<T>(kfun<T>, const T *, int64_t, const T *, const T *, int64_t, int64_t,       \
                                           const T *, T, const T *, int, int, int64_t, T *, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace plssvm_mi
