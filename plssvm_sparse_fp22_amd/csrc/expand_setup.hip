// Setup of the sparse polynomial / RBF kernel expansion (the method: expand.hip): the remainder H of
// the pairs sharing two or more features, built once per setup as symmetric rows and scattered into the remainder
// stream that expand.hip's kernels read per K·p.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "../../include/plssvm_mi355x.h"
#include "expand.hpp"

namespace plssvm_mi {

namespace {

struct d2sum {
    __host__ __device__ double2 operator()(const double2 &a, const double2 &b) const {
        return make_double2(a.x + b.x, a.y + b.y);
    }
};

struct hpair {
    uint64_t key;  // (row - i0) << 32 | j
    double h;
};

// keep pairs with a non-zero remainder (in the real type) that touch this rank's rows
struct h_keep {
    int64_t i0, r0, r1;
    int f32;
    __host__ __device__ bool operator()(const hpair &p) const {
        if (f32 ? ((float) p.h == 0.0f) : (p.h == 0.0)) return false;
        const int64_t i = i0 + (int64_t) (p.key >> 32), j = (int64_t) (p.key & 0xFFFFFFFFull);
        return (i >= r0 && i < r1) || (j >= r0 && j < r1);
    }
};

// incidences of row i: sum over its entries e of #{ j < i in column col[e] }
__global__ __launch_bounds__(256) void exp_count_kernel(const int64_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ col,
                                                        const int64_t *__restrict__ cpos,
                                                        const int64_t *__restrict__ colptr, int64_t i0, int64_t i1,
                                                        int64_t *__restrict__ cnt) {
    const int64_t i = i0 + (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= i1) return;
    int64_t c = 0;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) c += cpos[k] - colptr[col[k]];
    cnt[i - i0] = c;
}

// one workgroup per row i: every incidence (i, j < i, f) -> key (i - i0, j), value (a, phi(a)), a = x_if x_jf
template <typename T>
__global__ __launch_bounds__(256) void exp_gen_kernel(const int64_t *__restrict__ rowptr,
                                                      const int32_t *__restrict__ col, const T *__restrict__ val,
                                                      const int64_t *__restrict__ cpos,
                                                      const int64_t *__restrict__ colptr,
                                                      const int32_t *__restrict__ crow, const T *__restrict__ cval,
                                                      int64_t i0, const int64_t *__restrict__ off,
                                                      uint64_t *__restrict__ keys, double2 *__restrict__ vals,
                                                      phi_fn phi) {
    const int64_t i = i0 + blockIdx.x;
    const uint64_t il = (uint64_t) blockIdx.x;
    int64_t out = off[blockIdx.x];
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int64_t c0 = colptr[col[k]], c1 = cpos[k];
        const double xi = (double) val[k];
        for (int64_t t = c0 + threadIdx.x; t < c1; t += blockDim.x) {
            const double a = xi * (double) cval[t];
            keys[out + (t - c0)] = (il << 32) | (uint64_t) (uint32_t) crow[t];
            vals[out + (t - c0)] = make_double2(a, phi(a));
        }
        out += c1 - c0;
    }
}

// remainder of every unique pair: H = phi(s) - sum_f phi(a_f)  (0 for single-feature pairs)
__global__ __launch_bounds__(256) void exp_h_kernel(const uint64_t *__restrict__ ukeys, const double2 *__restrict__ agg,
                                                    const int64_t *__restrict__ nruns, phi_fn phi,
                                                    hpair *__restrict__ out) {
    const int64_t u = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= *nruns) return;
    const double2 v = agg[u];
    out[u] = hpair{ ukeys[u], phi(v.x) - v.y };
}

template <typename T>
__global__ __launch_bounds__(256) void exp_append_kernel(const hpair *__restrict__ sel, const int64_t *__restrict__ nsel,
                                                         int64_t i0, int32_t *__restrict__ li, int32_t *__restrict__ lj,
                                                         T *__restrict__ lh) {
    const int64_t u = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= *nsel) return;
    const hpair p = sel[u];
    li[u] = (int32_t) (i0 + (int64_t) (p.key >> 32));
    lj[u] = (int32_t) (p.key & 0xFFFFFFFFull);
    lh[u] = (T) p.h;
}

// row histograms of the kept pairs: lower part (i in [r0, r1)) and upper part (j in [r0, r1))
__global__ __launch_bounds__(256) void exp_hist_kernel(const int32_t *__restrict__ li, const int32_t *__restrict__ lj,
                                                       int64_t P, int64_t r0, int64_t r1,
                                                       unsigned long long *__restrict__ clo,
                                                       unsigned long long *__restrict__ cup,
                                                       uint32_t *__restrict__ upflag) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P) return;
    const int64_t i = li[t], j = lj[t];
    if (i >= r0 && i < r1) atomicAdd(&clo[i - r0], 1ull);
    const bool up = j >= r0 && j < r1;
    if (up) atomicAdd(&cup[j - r0], 1ull);
    upflag[t] = up ? (uint32_t) (j - r0) : 0xFFFFFFFFu;  // sort key of the upper part (others sort last)
}

__global__ __launch_bounds__(256) void exp_pad8_kernel(const unsigned long long *__restrict__ clo,
                                                       const unsigned long long *__restrict__ cup, int64_t R,
                                                       int64_t *__restrict__ cnt8) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) cnt8[r] = (int64_t) ((clo[r] + cup[r] + 7ull) & ~7ull);
}

// slots of row r: j = r (pads), H = 0; chunk rows
template <typename T>
__global__ __launch_bounds__(256) void exp_init_rows_kernel(const int64_t *__restrict__ off8, int64_t R, int64_t r0,
                                                            int32_t *__restrict__ hj, T *__restrict__ hv,
                                                            int32_t *__restrict__ hcrow) {
    const int64_t r = (int64_t) blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    for (int64_t s = off8[r] + lane; s < off8[r + 1]; s += 64) {
        hj[s] = (int32_t) (r0 + r);
        hv[s] = T(0);
        if ((s & 7) == 0) hcrow[s >> 3] = (int32_t) (r0 + r);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void exp_place_lower_kernel(const int32_t *__restrict__ li,
                                                              const int32_t *__restrict__ lj, const T *__restrict__ lh,
                                                              int64_t P, int64_t r0, int64_t r1,
                                                              const int64_t *__restrict__ lo_start,
                                                              const int64_t *__restrict__ off8, int32_t *__restrict__ hj,
                                                              T *__restrict__ hv) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P) return;
    const int64_t i = li[t];
    if (i < r0 || i >= r1) return;
    const int64_t r = i - r0, pos = off8[r] + (t - lo_start[r]);
    hj[pos] = lj[t];
    hv[pos] = lh[t];
}

template <typename T>
__global__ __launch_bounds__(256) void exp_place_upper_kernel(const uint32_t *__restrict__ skey,
                                                              const uint32_t *__restrict__ sidx, int64_t nup,
                                                              const int32_t *__restrict__ li, const T *__restrict__ lh,
                                                              const unsigned long long *__restrict__ clo,
                                                              const int64_t *__restrict__ up_start,
                                                              const int64_t *__restrict__ off8, int32_t *__restrict__ hj,
                                                              T *__restrict__ hv) {
    const int64_t u = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nup) return;
    const int64_t r = skey[u], t = sidx[u];
    const int64_t pos = off8[r] + (int64_t) clo[r] + (u - up_start[r]);
    hj[pos] = li[t];
    hv[pos] = lh[t];
}

// H_ii = phi(|x_i|^2) - sum_f phi(x_if^2) and phi(|x_i|^2), rows 0..m-1
template <typename T>
__global__ __launch_bounds__(256) void exp_diag_kernel(const int64_t *__restrict__ rowptr, const T *__restrict__ val,
                                                       int64_t m, phi_fn phi, T *__restrict__ hdiag,
                                                       T *__restrict__ phin) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double n = 0.0, s = 0.0;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const double x = (double) val[k], a = x * x;
        n += a;
        s += phi(a);
    }
    const double pn = phi(n);
    hdiag[i] = (T) (pn - s);
    phin[i] = (T) pn;
}

__global__ __launch_bounds__(256) void exp_iota_kernel(uint32_t *__restrict__ v, int64_t n) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) v[t] = (uint32_t) t;
}

// lower-triangle join (build_expansion): a lower pair's row and H travel together through the transpose's sort
template <typename T>
struct lt_val {
    T h;
    int32_t i;
};

// row r's lower list (slots r cap .. r cap + cnt[r]) to the compact arrays at loff[r]: partner keys and (row, H);
// one wave per row, coalesced
template <typename T>
__global__ __launch_bounds__(256) void exp_lt_compact_kernel(const int32_t *__restrict__ sj, const T *__restrict__ sv,
                                                             const int64_t *__restrict__ cnt, const int64_t *__restrict__ loff,
                                                             int64_t R, int64_t cap, uint32_t *__restrict__ lk,
                                                             lt_val<T> *__restrict__ lv) {
    const int64_t r = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    const int64_t b = loff[r];
    for (int64_t k = lane; k < cnt[r]; k += 64) {
        lk[b + k] = (uint32_t) sj[r * cap + k];
        lv[b + k] = lt_val<T>{ sv[r * cap + k], (int32_t) r };
    }
}

// per row j: its upper pairs are the run of key j in the sorted keys: ustart[j] = first, tot[j] = lower + upper count
// (R + 1 entries: tot[R] = 0 for the scan's total)
__global__ __launch_bounds__(256) void exp_lt_runs_kernel(const uint32_t *__restrict__ ks, int64_t NL,
                                                          const int64_t *__restrict__ lcnt, int64_t R,
                                                          int64_t *__restrict__ ustart, int64_t *__restrict__ tot) {
    const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j > R) return;
    if (j == R) {
        tot[R] = 0;
        return;
    }
    auto lb = [&](uint32_t key) {
        int64_t lo = 0, hi = NL;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ks[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    const int64_t a = lb((uint32_t) j), b = lb((uint32_t) j + 1u);
    ustart[j] = a;
    tot[j] = lcnt[j] + (b - a);
}

// the symmetric rows: lower pair q (compact order) at off8[i] + (q - loff[i]); sorted pair p (partner j) at
// off8[j] + lcnt[j] + (p - ustart[j]) — both coalesced
template <typename T>
__global__ __launch_bounds__(256) void exp_lt_place_kernel(const uint32_t *__restrict__ lk, const lt_val<T> *__restrict__ lv,
                                                           const uint32_t *__restrict__ ks, const lt_val<T> *__restrict__ vs,
                                                           int64_t NL, const int64_t *__restrict__ loff,
                                                           const int64_t *__restrict__ lcnt,
                                                           const int64_t *__restrict__ ustart,
                                                           const int64_t *__restrict__ off8, int32_t *__restrict__ hj,
                                                           T *__restrict__ hv) {
    const int64_t q = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= NL) return;
    const lt_val<T> a = lv[q];
    const int64_t pl = off8[a.i] + (q - loff[a.i]);
    hj[pl] = (int32_t) lk[q];
    hv[pl] = a.h;
    const uint32_t j = ks[q];
    const lt_val<T> b = vs[q];
    const int64_t pu = off8[j] + lcnt[j] + (q - ustart[j]);
    hj[pu] = b.i;
    hv[pu] = b.h;
}

// ---- row join: the remainder's symmetric rows built per row (default; PLSSVM_MI_EXP_JOIN=sort keeps the
// column-join sort below) ------------------------------------------------------------------------------
// 512-thread workgroups with a 32 KiB bitmap (round 5): 47 KiB of LDS and 75 VGPRs each, so three rows are joined
// per CU at once (their incidence reads in flight together, one row's barriers and scans under the others' reads).
// The rounds-3/4 form (1024 threads, 128 KiB bitmap: `-DRJ_NT_OPT=1024 -DRJ_BMW_OPT=32768`) held one row per CU;
// same-box A/Bs (profiles/r05_join_ab.json): the 3-RBF / config-5 join 0.18–0.21 / 0.29 s there, 0.14–0.17 / 0.24–0.25 s
// with two rows per CU (512 threads, 64 KiB), 0.12 / 0.21 s with three — more passes per row (262 144 partner rows each)
// cost less than the parallelism gains
#ifndef RJ_NT_OPT
#define RJ_NT_OPT 512
#endif
#ifndef RJ_BMW_OPT
#define RJ_BMW_OPT 8192
#endif
constexpr int RJ_NT = RJ_NT_OPT;
constexpr int RJ_BMW = RJ_BMW_OPT;  // bitmap words: 262 144 partner rows per pass (32 KiB of LDS)
constexpr int RJ_LCAP = 2048;  // repeat sightings held per pass (more: the pass range is halved)
constexpr int RJ_ECAP = 256;   // entries of row i held in LDS (longer rows: the sort join)
constexpr int RJ_WPT = RJ_BMW / RJ_NT;
#ifndef RJ_U
#define RJ_U 4  // incidence reads in flight per thread in the join's walk
#endif
constexpr int RJ_PMAX = 256;   // passes per row at most (more: the rank takes the sort join; PLSSVM_MI_EXP_RJ_PMAX: tests)

// Rows [r0, r0 + gridDim.x) of the rank, one workgroup per row i: its partners j != i sharing two or more
// features, ascending, in both triangles. Per pass over a range of partner rows, the column entries of
// row i's features (the incidences, read coalesced from the CSC) mark an LDS bitmap; a second sighting of
// a row appends it to a list, the list becomes a set in the bitmap and is enumerated in ascending order
// (a block scan of per-thread popcounts). Count mode (sj == nullptr): cnt[r] = #partners. Write mode:
// partner k of row r at sj[off8[r] + k], pads up to off8[r + 1] marked -1 (exp_rowjoin_h_kernel then
// forms H). Both modes take the same passes (the halving decisions depend on the data only): deterministic.
// A halved span grows back (doubles) after every completed range, so one dense cluster of partners does not
// cut the rest of the row into small passes; a row needing more than RJ_PMAX passes (every pass rescans its
// incidences) sets *ovf in count mode and the host builds the rank's rows by the sort join instead.
// Slot mode (off8 == nullptr, sj != nullptr; the default one-pass join): partner k of row r at sj[r cap + k]
// for k < cap, cnt[r] = the row's count (also beyond cap: *cnt_max lets the host redo such rows by the two
// passes), no pads — the count pass is not needed.
// Lower mode (cposl != nullptr, round 5): only the partners j < i — the passes cover rows [0, i) and each column's
// range ends at row i's own entry (cposl: the CSR entry's CSC position), so a row reads on average half of its
// incidences; the other triangle is the transpose of these lists (build_expansion).
#if defined(RJ_WPE_OPT) && RJ_WPE_OPT > 0  // compile the join for this many waves per SIMD (a register cap)
#define RJ_WPE_ATTR __attribute__((amdgpu_waves_per_eu(RJ_WPE_OPT)))
#else
#define RJ_WPE_ATTR
#endif
__global__ __launch_bounds__(RJ_NT) RJ_WPE_ATTR void exp_rowjoin_kernel(const int64_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ col,
                                                            const int64_t *__restrict__ colptr,
                                                            const int32_t *__restrict__ crow, int64_t m, int64_t r0,
                                                            int64_t *__restrict__ cnt, const int64_t *__restrict__ off8,
                                                            int32_t *__restrict__ sj, unsigned int *__restrict__ ovf,
                                                            int pmax, int64_t cap, unsigned long long *__restrict__ cnt_max,
                                                            const int64_t *__restrict__ csplit, int nsplit,
                                                            const int64_t *__restrict__ cposl = nullptr) {
    __shared__ uint32_t bm[RJ_BMW];
    __shared__ int32_t rep[RJ_LCAP];
    __shared__ int32_t zcol[RJ_ECAP];
    __shared__ int32_t zoff[RJ_ECAP + 1];
    __shared__ int64_t cst[RJ_ECAP];
    __shared__ int64_t pst[RJ_ECAP];    // a partial pass: each column's first entry with a row in [R0, R1)
    __shared__ int32_t pzoff[RJ_ECAP + 1];
    __shared__ int32_t wtot[RJ_NT / 64];
    __shared__ int nrep_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x, i = r0 + r;
    const int64_t e0 = rowptr[i];
    const int ne = (int) (rowptr[i + 1] - e0);  // <= RJ_ECAP (host-checked)
    for (int e = tid; e < ne; e += RJ_NT) {  // column starts and lengths in parallel (one global read each)
        const int32_t f = col[e0 + e];
        zcol[e] = f;
        const int64_t c0 = colptr[f];
        cst[e] = c0;
        zoff[e + 1] = (int32_t) (colptr[f + 1] - c0);
    }
    __syncthreads();
    if (tid == 0) {  // prefix over LDS only
        zoff[0] = 0;
        for (int e = 0; e < ne; ++e) zoff[e + 1] += zoff[e];
    }
    __syncthreads();
    const bool wr = sj != nullptr, slots = wr && off8 == nullptr;
    int64_t written = 0;
    constexpr int64_t SPAN_MAX = (int64_t) RJ_BMW * 32;
    int64_t span = SPAN_MAX;
    int passes = 0;
    const bool lower = cposl != nullptr;
    const int64_t Rend = lower ? i : m;  // partner rows [0, Rend)
    for (int64_t R0 = 0; R0 < Rend;) {
        if (++passes > pmax) {  // uniform
            if ((!wr || slots) && tid == 0) {
                cnt[r] = 0;
                atomicOr(ovf, 1u);
            }
            return;
        }
        const int64_t R1 = min(Rend, R0 + span);
        // the bitmap words of this pass's range only (words L < nw, owned by threads < tcnt): a short range — every
        // lower-triangle row's first pass is [0, i) — clears, counts and enumerates only its part of the bitmap
        const int64_t nw = (R1 - R0 + 31) >> 5;
        const int tcnt = (int) min((int64_t) RJ_NT, (nw + RJ_WPT - 1) / RJ_WPT);
        if (tid < tcnt)
            for (int w = 0; w < RJ_WPT; ++w) bm[w * RJ_NT + tid] = 0u;
        if (tid == 0) nrep_s = 0;
        // a pass over part of the partner rows reads only that part of each column (rows ascend within a
        // column: two binary searches per feature), not every incidence of the row once per pass
        const bool whole = !lower && R0 == 0 && R1 >= m;
        if (lower) {
            // lower mode: each bound from the column's start (R0 = 0), the setup's table (a full-span boundary), row
            // i's own position (R1 = i) or a binary search
            for (int e = tid; e < ne; e += RJ_NT) {
                const int64_t a = cst[e], b = a + (zoff[e + 1] - zoff[e]);
                const int32_t f = zcol[e];
                auto first_ge = [&](int64_t Rb) -> int64_t {
                    if (csplit != nullptr && Rb % SPAN_MAX == 0) return csplit[(int64_t) f * nsplit + Rb / SPAN_MAX];
                    int64_t lo = a, hi = b;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (crow[mid] < Rb) lo = mid + 1;
                        else hi = mid;
                    }
                    return lo;
                };
                const int64_t lo = R0 == 0 ? a : first_ge(R0);
                const int64_t lo2 = R1 == i ? cposl[e0 + e] : first_ge(R1);
                pst[e] = lo;
                pzoff[e + 1] = (int32_t) (lo2 - lo);
            }
            __syncthreads();
            if (tid == 0) {
                pzoff[0] = 0;
                for (int e = 0; e < ne; ++e) pzoff[e + 1] += pzoff[e];
            }
        } else if (!whole) {
            // a pass of the full span starts and ends where every row's passes do: the column positions come from the
            // setup's table (one load per feature) instead of two binary searches (a chain of dependent loads)
            const bool tab = csplit != nullptr && R0 % SPAN_MAX == 0 && (R1 >= m || R1 % SPAN_MAX == 0);
            for (int e = tid; e < ne; e += RJ_NT) {
                const int64_t a = cst[e], b = a + (zoff[e + 1] - zoff[e]);
                int64_t lo = a, lo2 = b;
                if (tab) {
                    const int64_t *cs = csplit + (int64_t) zcol[e] * nsplit;
                    lo = cs[R0 / SPAN_MAX];
                    lo2 = R1 >= m ? b : cs[R1 / SPAN_MAX];
                } else {
                    int64_t hi = b;
                    while (lo < hi) {  // first row >= R0
                        const int64_t mid = (lo + hi) >> 1;
                        if (crow[mid] < R0) lo = mid + 1;
                        else hi = mid;
                    }
                    lo2 = lo;
                    int64_t hi2 = b;
                    while (lo2 < hi2) {  // first row >= R1
                        const int64_t mid = (lo2 + hi2) >> 1;
                        if (crow[mid] < R1) lo2 = mid + 1;
                        else hi2 = mid;
                    }
                }
                pst[e] = lo;
                pzoff[e + 1] = (int32_t) (lo2 - lo);
            }
            __syncthreads();
            if (tid == 0) {
                pzoff[0] = 0;
                for (int e = 0; e < ne; ++e) pzoff[e + 1] += pzoff[e];
            }
        }
        __syncthreads();
        const int64_t *S = whole ? cst : pst;
        const int32_t *Z = whole ? zoff : pzoff;
        const int32_t pinc = Z[ne];
        // RJ_U incidences per thread in flight (the walk is bound by the latency of these scattered reads)
        int e = 0;
        for (int32_t t0 = tid; t0 < pinc; t0 += RJ_U * RJ_NT) {
            int64_t jv[RJ_U];
#pragma unroll
            for (int u = 0; u < RJ_U; ++u) {
                const int32_t t = t0 + u * RJ_NT;
                jv[u] = -1;
                if (t < pinc) {
                    while (Z[e + 1] <= t) ++e;
                    jv[u] = crow[S[e] + (t - Z[e])];
                }
            }
#pragma unroll
            for (int u = 0; u < RJ_U; ++u) {
                const int64_t j = jv[u];
                if (j < 0 || j == i || j < R0 || j >= R1) continue;
                const uint32_t bit = 1u << ((j - R0) & 31);
                const uint32_t old = atomicOr(&bm[bm_addr<RJ_WPT, RJ_NT>((j - R0) >> 5)], bit);
                if (old & bit) {
                    const int q = atomicAdd(&nrep_s, 1);
                    if (q < RJ_LCAP) rep[q] = (int32_t) j;
                }
            }
        }
        __syncthreads();
        const int nr = nrep_s;
        if (nr > RJ_LCAP) {  // uniform: this range again in halves
            span = (span + 1) / 2;
            __syncthreads();
            continue;
        }
        if (tid < tcnt)
            for (int w = 0; w < RJ_WPT; ++w) bm[w * RJ_NT + tid] = 0u;
        __syncthreads();
        for (int q = tid; q < nr; q += RJ_NT) {
            const int64_t j = rep[q] - R0;
            atomicOr(&bm[bm_addr<RJ_WPT, RJ_NT>(j >> 5)], 1u << (j & 31));
        }
        __syncthreads();
        int c = 0;
        if (tid < tcnt) {
#pragma unroll 8
            for (int w = 0; w < RJ_WPT; ++w) c += __popc(bm[w * RJ_NT + tid]);
        }
        // exclusive block scan of c (wave scans + wave totals)
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int before = 0, U = 0;
        for (int w = 0; w < RJ_NT / 64; ++w) {
            const int v = wtot[w];
            if (w < wave) before += v;
            U += v;
        }
        if (wr) {
            int pos = before + incl - c;
            for (int w = 0; w < (tid < tcnt ? RJ_WPT : 0); ++w) {
                uint32_t word = bm[w * RJ_NT + tid];
                while (word) {
                    const int b = __ffs(word) - 1;
                    word &= word - 1;
                    rep[pos++] = (int32_t) (R0 + (int64_t) (tid * RJ_WPT + w) * 32 + b);
                }
            }
            __syncthreads();
            if (slots) {
                const int64_t base = r * cap + written;
                for (int q = tid; q < U && written + q < cap; q += RJ_NT) sj[base + q] = rep[q];
            } else {
                const int64_t base = off8[r] + written;
                for (int q = tid; q < U; q += RJ_NT) sj[base + q] = rep[q];
            }
        }
        written += U;
        __syncthreads();  // bm / rep are reused by the next pass
        R0 = R1;
        span = min(span * 2, SPAN_MAX);
    }
    if (!wr || slots) {
        if (tid == 0) {
            cnt[r] = written;
            if (slots) atomicMax(cnt_max, (unsigned long long) written);
        }
        return;
    }
    const int64_t b0 = off8[r], b1 = off8[r + 1];
    for (int64_t k = b0 + written + tid; k < b1; k += RJ_NT) sj[k] = -1;  // pads (exp_rowjoin_h_kernel)
}

// csplit[f][p] = the first position of column f whose row is >= p x (the join's full pass span), p < nsplit
__global__ __launch_bounds__(256) void exp_colsplit_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ crow,
                                                           int64_t d, int nsplit, int64_t span, int64_t *__restrict__ csplit) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= d * nsplit) return;
    const int64_t f = t / nsplit, R = (t % nsplit) * span;
    int64_t lo = colptr[f], hi = colptr[f + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (crow[mid] < R) lo = mid + 1;
        else hi = mid;
    }
    csplit[t] = lo;
}

// H of the row join's partners (sj from exp_rowjoin_kernel's write / slot pass; row r's entries in
// [rbeg[r], rend[r])): one 256-thread workgroup per row i, row i's features in an LDS hash (open addressing,
// <= 1/8 full: one probe per lookup instead of a binary search), one partner per wave at a time: the lanes take
// row j's entries (coalesced, 64 per step), look each up in row i, and the matches — ascending features — are
// summed in that order from a ballot: H_ij = phi(s_ij) - sum_f phi(x_if x_jf) in fp64, rounded to T (the
// sequential sum of the sort join; rbf: a product recurrence without the expm1 of s_ij, in the body). The next
// partner's row bounds are loaded one step ahead. Pads (sj < 0): j = i, H = 0. lower_nz += #(j < i, H != 0 in T).
constexpr int RJH_NT = 256;
// a wave-uniform 64-bit value into scalar registers
__device__ __forceinline__ int64_t rj_uni64(int64_t v) {
    const uint32_t lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) v);
    const uint32_t hi = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) ((uint64_t) v >> 32));
    return (int64_t) (((uint64_t) hi << 32) | lo);
}
constexpr int RJ_HS = 2048;  // hash slots for row i's features (<= RJ_ECAP keys)
__device__ __forceinline__ int rj_hash(int32_t f) { return (int) (((uint32_t) f * 2654435761u) >> (32 - 11)); }
#ifndef RJH_WPE
#define RJH_WPE 8  // waves per SIMD the H kernel is compiled for (<= 64 VGPRs: 8 resident 256-thread workgroups per CU)
#endif
// rbf phi in float (exp_rowjoin_h_kernel<float, true>): expm1(2 g a), a degree-5 Taylor polynomial where |2 g a| < 2^-7
// (truncation < 2^-35 / 720 relative), expm1f otherwise
__device__ __forceinline__ float rj_phi32(float g2, float a) {
    const float u = g2 * a;
    if (fabsf(u) < 0x1p-7f) {
        float p = 1.0f / 120.0f;
        p = fmaf(p, u, 1.0f / 24.0f);
        p = fmaf(p, u, 1.0f / 6.0f);
        p = fmaf(p, u, 0.5f);
        p = fmaf(p, u, 1.0f);
        return p * u;
    }
    return expm1f(u);
}
// F32 (round 5; float contexts, rbf): the shared features' products, their phi and the product recurrence in float.
// The recurrence has no cancellation (two shared features: H = E_a E_b), so H keeps float's relative accuracy, which
// is what the float (or bfloat16) stream stores anyway; the fp64 evaluation cost twice the VALU cycles per partner of
// this VALU-bound kernel. Poly (H = c(s) - sum c(a_f) cancels) and fp64 contexts keep fp64.
template <typename T, bool F32 = false>
__global__ __launch_bounds__(RJH_NT) __attribute__((amdgpu_waves_per_eu(RJH_WPE, RJH_WPE))) void exp_rowjoin_h_kernel(const int64_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ col,
                                                               const T *__restrict__ val, int64_t r0, phi_fn phi,
                                                               double kbase, const int64_t *__restrict__ rbeg,
                                                               const int64_t *__restrict__ rend,
                                                               int32_t *__restrict__ sj, T *__restrict__ sv,
                                                               unsigned long long *__restrict__ lower_nz,
                                                               unsigned long long *__restrict__ ratio_bits) {
    __shared__ int32_t hkey[RJ_HS];
    __shared__ uint8_t hidx[RJ_HS];
    __shared__ T zval[RJ_ECAP];
    __shared__ unsigned long long lnz_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x, i = r0 + r;
    const int64_t e0 = rowptr[i];
    const int ne = (int) (rowptr[i + 1] - e0);  // <= RJ_ECAP (host-checked)
    for (int q = tid; q < RJ_HS; q += RJH_NT) hkey[q] = -1;
    if (tid == 0) lnz_s = 0ull;
    __syncthreads();
    for (int e = tid; e < ne; e += RJH_NT) {
        const int32_t f = col[e0 + e];
        zval[e] = val[e0 + e];
        int h = rj_hash(f);
        while (atomicCAS(&hkey[h], -1, f) != -1) h = (h + 1) & (RJ_HS - 1);  // distinct features: no duplicates
        hidx[h] = (uint8_t) e;
    }
    __syncthreads();
    unsigned long long lnz = 0ull;
    double rmax = 0.0;
    // The partner bookkeeping is wave-uniform and kept in scalar registers (readfirstlane): the partner loop, the step
    // loop and the entry addresses (scalar base + 32-bit lane offset) cost no VALU. The prefetches stay vector loads
    // (an opaque zero offset): a scalar load would share lgkmcnt with the LDS probes and be waited for at once. A
    // partner's row bounds are loaded one partner ahead, its index two ahead.
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int64_t q0 = rj_uni64(rbeg[r]), q1 = rj_uni64(rend[r]);
    constexpr int NW = RJH_NT / 64;
    // buffer loads (always vector memory instructions) through descriptors built in scalar registers: the row's
    // partner list from its start (offsets < 2^31 B), a partner's two row bounds as one 16-byte load
    const __amdgpu_buffer_rsrc_t rs_sj = __builtin_amdgcn_make_buffer_rsrc((void *) (sj + q0), (short) 0, 0x7FFFFFFF, 0x00020000);
    auto load_j = [&](int64_t qq) -> uint32_t {
        return qq < q1 ? __builtin_amdgcn_raw_buffer_load_b32(rs_sj, 0, (int) ((qq - q0) * 4), 0) : 0xFFFFFFFFu;
    };
    using u32x4 = decltype(__builtin_amdgcn_raw_buffer_load_b128(rs_sj, 0, 0, 0));
    auto load_bounds = [&](int64_t jj) -> u32x4 {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *) (rowptr + jj), (short) 0, 16, 0x00020000);
        return __builtin_amdgcn_raw_buffer_load_b128(rs, 0, 0, 0);
    };
    auto uni_lo = [](u32x4 v) {
        return (int64_t) (((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) v[1]) << 32) |
                          (uint32_t) __builtin_amdgcn_readfirstlane((int) v[0]));
    };
    auto uni_hi = [](u32x4 v) {
        return (int64_t) (((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) v[3]) << 32) |
                          (uint32_t) __builtin_amdgcn_readfirstlane((int) v[2]));
    };
    int64_t q = q0 + wv;
    int64_t jn = (int32_t) __builtin_amdgcn_readfirstlane((int) load_j(q));
    u32x4 bn = {};
    if (jn >= 0) bn = load_bounds(jn);
    uint32_t jnn = load_j(q + NW);
    for (; q < q1; q += NW) {
        const int64_t j = jn;
        const int64_t kb = j >= 0 ? uni_lo(bn) : 0, ke = j >= 0 ? uni_hi(bn) : 0;
        jn = (int32_t) __builtin_amdgcn_readfirstlane((int) jnn);  // the next partner: its bounds now, the one after's index
        if (jn >= 0) bn = load_bounds(jn);
        jnn = load_j(q + 2 * NW);
        if (j < 0) {  // pad
            if (lane == 0) {
                sj[q] = (int32_t) i;
                sv[q] = T(0);
            }
            continue;
        }
        // rbf: with E_f = expm1(2 g x_if x_jf), 1 + E(s_ij) = prod_f (1 + E_f), so H = prod (1 + E_f) - 1 - sum E_f
        // accumulates over the shared features (ascending) as Q += P E_f, P += E_f + P E_f (P = prod - 1): no
        // expm1 of s_ij and no cancellation (two shared features: H = E_a E_b exactly). poly: H = c(s) - sum c(a_f).
        using A = typename std::conditional<F32, float, double>::type;
        const bool rbf = F32 || phi.rbf != 0;
        A sd = 0, sphi = 0, P = 0;
        for (int64_t k0 = kb; k0 < ke; k0 += 64) {
            const int32_t *ck = col + k0;
            const T *vkp = val + k0;
            A a = 0, pa = 0;
            bool hit = false;
            if (lane < ke - k0) {
                // the value is loaded with the feature (one latency per partner, not a second one after the probe)
                const int32_t f = ck[lane];
                const T vk = vkp[lane];
                int h = rj_hash(f);
                int32_t key;
                while ((key = hkey[h]) >= 0 && key != f) h = (h + 1) & (RJ_HS - 1);
                if (key == f) {
                    a = (A) zval[hidx[h]] * (A) vk;
                    if constexpr (F32) pa = rj_phi32((float) phi.g2, a);
                    else pa = phi(a);
                    hit = true;
                }
            }
            uint64_t mask = __ballot(hit);
            while (mask) {  // wave-uniform: the shared features in ascending order
                const int b = __ffsll((long long) mask) - 1;
                mask &= mask - 1;
                const A pb = __shfl(pa, b);
                if (rbf) {
                    const A t = P * pb;
                    sphi += t;  // Q
                    P += pb + t;
                } else {
                    sd += __shfl(a, b);
                    sphi += pb;
                }
            }
        }
        const double ps = rbf ? (double) P : phi((double) sd);  // E(s) or c(s)
        const T h = (T) (rbf ? sphi : (A) (ps - (double) sphi));
        // |H| relative to the pair's kernel value without the e_i e_j factor (rbf 1 + E(s), poly kappa + c(s));
        // the division only when it can raise the maximum (wave-uniform values)
        const double kv = fabs(kbase + ps), ah = fabs((double) h);
        if (h != T(0) && ah > rmax * kv) rmax = kv > 0.0 ? ah / kv : 1e300;
        if (lane == 0) {
            sv[q] = h;
            if (j < i && h != T(0)) ++lnz;
        }
    }
    if (lane == 0 && lnz) atomicAdd(&lnz_s, lnz);
    if (lane == 0 && rmax > 0.0) atomicMax(ratio_bits, (unsigned long long) __double_as_longlong(rmax));  // >= 0: bit order
    __syncthreads();
    if (tid == 0 && lnz_s) atomicAdd(lower_nz, lnz_s);
}

// the one-pass join's row ranges: beg[r] = r cap, end[r] = r cap + cnt[r] (every count <= cap, host-checked)
__global__ __launch_bounds__(256) void exp_pool_range_kernel(const int64_t *__restrict__ cnt, int64_t R, int64_t cap,
                                                             int64_t *__restrict__ beg, int64_t *__restrict__ end) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) beg[r] = r * cap, end[r] = r * cap + cnt[r];
}

__global__ __launch_bounds__(256) void exp_pad8_cnt_kernel(const int64_t *__restrict__ cnt, int64_t R,
                                                           int64_t *__restrict__ cnt8) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) cnt8[r] = (cnt[r] + 7) & ~int64_t(7);
}


// ---- remainder stream layout (built from the padded symmetric rows) ---------------------------------------
// count index of (row r, window W): ((I NWV + v) nW + W) RPW + rr,  r = I RB + v RPW + rr
__device__ __forceinline__ int64_t exp_cidx(int64_t r, int64_t W, int64_t nW, int64_t RB) {
    const int64_t RPW = RB / EXP_NWV;
    const int64_t I = r / RB, v = (r % RB) / RPW, rr = r % RPW;
    return ((I * EXP_NWV + v) * nW + W) * RPW + rr;
}

// The cell kernels below walk one row per wave: a row's entries (sorted by j; H == 0 entries — pads, or a
// remainder that rounded to 0 — skipped) are read 64 at a time, coalesced (one row per thread read a row's
// range serially: uncoalesced, 3-4x slower at setup). The valid entries of a step form runs of equal windows
// (j ascending); per run: on_open(prev window, window) when a window starts (wave-uniform), on_entry for each
// of its entries with its rank k among the row's valid entries of that window (lane-parallel), and
// on_close(window, count) when the window's last entry has been seen (wave-uniform). Same order, same values
// as the sequential walk.
template <typename T, typename FO, typename FE, typename FC>
__device__ __forceinline__ void exp_row_windows(const int32_t *__restrict__ sj, const T *__restrict__ sv, int64_t b,
                                                int64_t e, int64_t CW, FO on_open, FE on_entry, FC on_close) {
    const int lane = threadIdx.x & 63;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int curW = -1;
    int64_t kcur = 0;
    for (int64_t s0 = b; s0 < e; s0 += 64) {
        const int64_t s = s0 + lane;
        bool valid = false;
        int W = 0;
        int32_t jj = 0;
        T h = T(0);
        if (s < e) {
            h = sv[s];
            jj = sj[s];
            valid = h != T(0);
            W = valid ? (int) (jj / CW) : 0;
        }
        uint64_t rem = __ballot(valid);
        while (rem) {  // wave-uniform: one run of equal windows at a time
            const int W0 = __shfl(W, __ffsll((long long) rem) - 1);
            const uint64_t m0 = __ballot(valid && W == W0) & rem;
            if (W0 != curW) {
                if (curW >= 0) on_close(curW, kcur);
                on_open(curW, W0);
                curW = W0;
                kcur = 0;
            }
            if ((m0 >> lane) & 1ull) on_entry(jj, h, W0, kcur + __popcll(m0 & below));
            kcur += __popcll(m0);
            rem &= ~m0;
        }
    }
    if (curW >= 0) on_close(curW, kcur);
}

// per row r (rank-local), window W: count of its non-zero entries with j in W, rounded up to gran (4: chunks, 2: pair
// flags) slots; the cells without entries are left as they are (0, or a dummy written before)
template <typename T>
__global__ __launch_bounds__(256) void exp_cell_count_kernel(const int64_t *__restrict__ rbeg, const int64_t *__restrict__ rend,
                                                             const int32_t *__restrict__ sj, const T *__restrict__ sv,
                                                             int64_t R, int64_t nW, int64_t CW, int64_t RB, int64_t gran,
                                                             int64_t *__restrict__ cnt) {
    const int64_t r = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    exp_row_windows<T>(sj, sv, rbeg[r], rend[r], CW, [](int, int) {}, [](int32_t, T, int, int64_t) {},
                       [&](int W, int64_t k) {
                           if (lane == 0) cnt[exp_cidx(r, W, nW, RB)] = (k + gran - 1) & ~(gran - 1);
                       });
}

// pair flags: a wave's stream of a window (RPW consecutive cells, exp_cidx) padded to a multiple of 4 slots, the
// 2 padding slots (H = 0, no flag: they add 0 to the row open at the end) given to the group's last cell — so every
// (block, wave, window) range starts on a chunk (woff = coff / 4)
__global__ __launch_bounds__(256) void exp_cell_pad_groups_kernel(int64_t ngroups, int64_t RPW, int64_t *__restrict__ cnt) {
    const int64_t gi = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= ngroups) return;
    int64_t *c = cnt + gi * RPW;
    int64_t s = 0;
    for (int64_t k = 0; k < RPW; ++k) s += c[k];
    if (s & 2) c[RPW - 1] += 2;
}

template <typename T>
__global__ __launch_bounds__(256) void exp_cell_scatter_kernel(const int64_t *__restrict__ rbeg, const int64_t *__restrict__ rend,
                                                               const int32_t *__restrict__ sj, const T *__restrict__ sv,
                                                               int64_t R, int64_t nW, int64_t CW, int64_t RB,
                                                               const int64_t *__restrict__ coff,
                                                               uint16_t *__restrict__ hjl, T *__restrict__ hv,
                                                               uint16_t *__restrict__ hv16, uint16_t *__restrict__ hrow) {
    const int64_t r = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    const uint16_t rl = (uint16_t) (r % RB);
    int64_t base = 0;
    exp_row_windows<T>(sj, sv, rbeg[r], rend[r], CW, [&](int, int W) { base = coff[exp_cidx(r, W, nW, RB)]; },
                       [&](int32_t j, T h, int W, int64_t k) {
                           hjl[base + k] = (uint16_t) (j - (int64_t) W * CW);
                           if (hv16 != nullptr) hv16[base + k] = bf16_rne((float) h);
                           else hv[base + k] = h;
                       },
                       [&](int, int64_t k) {
                           for (int64_t q = lane; q < ((k + 3) >> 2); q += 64) hrow[(base >> 2) + q] = rl;
                       });
}

// ---- flagged chunks (hbf16 layouts): no per-chunk row index ------------------------------------------------
// A stored bfloat16 H with |H| < 2 has bit 14 (the exponent's top bit) clear, so the first H of a chunk can
// carry a flag instead: set on the first chunk of each (row, window) cell. Every row of the rank gets at least
// one chunk per window (a dummy: j = 0, H = 0, when it has no partners there), so inside a wave's stream of a
// window the rows follow each other without gaps and a chunk's row is the wave's first row + (the number of
// flags up to it) - 1: a ballot and a lane count per 64 chunks instead of 2 bytes per chunk.

// stats[0] += windows without entries (the dummies the layout would add), stats[1] |= 1 when a stored H's
// bfloat16 has bit 14 set (|H| >= 2: the bit is not free)
template <typename T>
__global__ __launch_bounds__(256) void exp_cell_stats_kernel(const int64_t *__restrict__ rbeg, const int64_t *__restrict__ rend,
                                                             const int32_t *__restrict__ sj, const T *__restrict__ sv,
                                                             int64_t R, int64_t nW, int64_t CW,
                                                             unsigned long long *__restrict__ stats) {
    const int64_t r = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    int64_t nwin = 0;
    unsigned long long big = 0;
    exp_row_windows<T>(sj, sv, rbeg[r], rend[r], CW, [&](int, int) { ++nwin; },
                       [&](int32_t, T h, int, int64_t) {
                           if (bf16_rne((float) h) & 0x4000u) big = 1;
                       },
                       [](int, int64_t) {});
    big = __ballot(big != 0) ? 1ull : 0ull;
    if ((threadIdx.x & 63) == 0) {
        if (nW - nwin) atomicAdd(stats, (unsigned long long) (nW - nwin));
        if (big) atomicOr(stats + 1, big);
    }
}

// the dummies: a (row, window) cell without entries takes one 4-slot chunk (pair flags: one 2-slot pair)
__global__ __launch_bounds__(256) void exp_cell_fill_empty_kernel(int64_t R, int64_t nW, int64_t RB, int64_t dsz,
                                                                  int64_t *__restrict__ cnt) {
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * nW) return;
    const int64_t idx = exp_cidx(t / nW, t % nW, nW, RB);
    if (cnt[idx] == 0) cnt[idx] = dsz;
}

// flagged layout, EXP_JH: slot t of chunk c = t / 4 keeps its index at 8 c + t % 4 and its H at 8 c + 4 + t % 4
// of the one array (0: two arrays, index and H at t)
__device__ __forceinline__ int64_t exp_jh_j(int64_t t) { return EXP_JH ? ((t & ~int64_t(3)) << 1) + (t & 3) : t; }
__device__ __forceinline__ int64_t exp_jh_h(int64_t t) { return EXP_JH ? ((t & ~int64_t(3)) << 1) + 4 + (t & 3) : t; }

// exp_cell_scatter_kernel for the flagged layout (bfloat16 H, buffers zeroed): every window of the row in
// order, its entries with bit 14 set on the cell's first H, or a dummy (j = 0, H = 0 with the bit) for a window
// without entries
template <typename T>
__global__ __launch_bounds__(256) void exp_cell_scatter_flag_kernel(const int64_t *__restrict__ rbeg, const int64_t *__restrict__ rend,
                                                                    const int32_t *__restrict__ sj, const T *__restrict__ sv,
                                                                    int64_t R, int64_t nW, int64_t CW, int64_t RB,
                                                                    const int64_t *__restrict__ coff,
                                                                    uint16_t *__restrict__ hjl, uint16_t *__restrict__ hv16) {
    const int64_t r = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    auto dummies = [&](int64_t w0, int64_t w1) {  // windows [w0, w1) without entries
        for (int64_t w = w0 + lane; w < w1; w += 64) hv16[exp_jh_h(coff[exp_cidx(r, w, nW, RB)])] = (uint16_t) 0x4000u;
    };
    int64_t base = 0, last = -1;
    exp_row_windows<T>(sj, sv, rbeg[r], rend[r], CW,
                       [&](int prev, int W) {
                           dummies(prev + 1, W);
                           base = coff[exp_cidx(r, W, nW, RB)];
                           last = W;
                       },
                       [&](int32_t j, T h, int W, int64_t k) {
                           hjl[exp_jh_j(base + k)] = (uint16_t) (j - (int64_t) W * CW);
                           hv16[exp_jh_h(base + k)] = (uint16_t) (bf16_rne((float) h) | (k == 0 ? 0x4000u : 0u));
                       },
                       [](int, int64_t) {});
    dummies(last + 1, nW);
}

// first chunk of (block I, wave v, window W), W = 0..nW (W = nW: the end of the wave's stream)
__global__ __launch_bounds__(256) void exp_cell_woff_kernel(const int64_t *__restrict__ coff, int64_t nbv, int64_t nW,
                                                            int64_t RB, int64_t *__restrict__ woff) {
    const int64_t RPW = RB / EXP_NWV;
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nbv * (nW + 1)) return;
    const int64_t bv = t / (nW + 1), W = t % (nW + 1);
    woff[t] = coff[(bv * nW + W) * RPW] >> 2;
}

}  // namespace

// Can the expansion represent this kernel to rounding? rbf (factored form): the Taylor degree K of
// E(a) = expm1(2 g a) whose remainder |u|^K e^{2|u|} / (K+1)! is below 2^-27 (fp32) / 2^-56 (fp64)
// relative for every |u| = |2 g x_if x_jf| <= umax; poly: K = degree (exact). K <= EXP_KMAX.
template <typename T>
bool engine<T>::expansion_eligible() {
    auto &ex = csr.ex;
    std::fill(std::begin(ex.coef), std::end(ex.coef), 0.0);
    if (kernel == 1) {
        if (degree < 0 || degree > EXP_KMAX) return false;
        const phi_fn phi = make_phi<T>(kernel, degree, gamma, coef0);
        ex.K = degree;
        for (int k = 1; k <= degree; ++k) ex.coef[k] = phi.bin[k];
    } else if (kernel == 2) {
        if (rbf_form == 1) return false;
        const double umax = ex.umax;
        const double tol = sizeof(T) == 4 ? std::ldexp(1.0, -27) : std::ldexp(1.0, -56);
        int K = 1;
        double fact = 2.0;  // (K + 1)!
        while (K <= EXP_KMAX && std::pow(umax, K) * std::exp(2.0 * umax) / fact > tol) {
            ++K;
            fact *= (double) (K + 1);
        }
        if (K > EXP_KMAX) return false;
        ex.K = K;
        double c = 1.0;  // (2 g)^k / k!
        for (int k = 1; k <= K; ++k) {
            c = c * 2.0 * (double) gamma / (double) k;
            ex.coef[k] = c;
        }
    } else {
        return false;
    }
    ex.KM = ex.K <= 2 ? 2 : (ex.K <= 4 ? 4 : (ex.K <= 8 ? 8 : 16));
    return true;
}

// ---- the setup's stages (DESIGN.md §5.1 "setup stages"): build_expansion below is their chain -------------------
namespace {

// kern over blocks x threads on the stream, checked
template <typename K, typename... A>
void launch(K kern, int64_t blocks, int threads, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(kern, dim3((unsigned) blocks), dim3((unsigned) threads), 0, stream, args...);
    MI_LAUNCH_CHECK();
}

// out[k] = in[0] + ... + in[k - 1] for k < n, with a temporary of its own
template <typename In, typename Out>
void exclusive_sum(In *in, Out *out, int64_t n, hipStream_t stream) {
    size_t tb = 0;
    MI_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int) n, stream));
    dev_buf<unsigned char> t;
    t.alloc((int64_t) std::max<size_t>(tb, 16), stream, false);
    MI_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(t.get(), tb, in, out, (int) n, stream));
}

// every PLSSVM_MI_EXP_* variable the setup reads, read once per setup
struct exp_knobs {
    static int as_int(const char *name) { return (int) std::clamp<long long>(env_long(name), INT_MIN, INT_MAX); }
    bool join_sort = env_is("PLSSVM_MI_EXP_JOIN", "sort");    // the column-join sort instead of the row joins
    bool twopass = env_is("PLSSVM_MI_EXP_RJ", "twopass");     // row join: count pass + write pass, no slot pool
    int64_t rj_cap = env_long("PLSSVM_MI_EXP_RJ_CAP");        // > 0: the slot pools' partners per row (tests)
    int rj_pmax = as_int("PLSSVM_MI_EXP_RJ_PMAX") >= 1 ? as_int("PLSSVM_MI_EXP_RJ_PMAX") : RJ_PMAX;  // passes per row
    bool lt = !env_is("PLSSVM_MI_EXP_LT", "0");               // 0: no lower-triangle join
    bool colsplit = !env_is("PLSSVM_MI_EXP_COLSPLIT", "0");   // 0: binary searches only (tests)
    bool h64 = env_long("PLSSVM_MI_EXP_H64") != 0;            // the H kernel in fp64 also for rbf in a float context
    bool hfmt_full = env_is("PLSSVM_MI_EXP_HFMT", "full");    // H stays in the real type
    int rows = env_is("PLSSVM_MI_EXP_ROWS", "index")   ? EXP_ROWS_INDEX
               : env_is("PLSSVM_MI_EXP_ROWS", "flags") ? EXP_ROWS_FLAGS
               : env_is("PLSSVM_MI_EXP_ROWS", "pairs") ? EXP_ROWS_PAIRS
                                                       : EXP_ROWS_AUTO;
    int rbb = as_int("PLSSVM_MI_EXP_RBB");                    // an accumulator class (4096 .. 32768) forces it
    int g = as_int("PLSSVM_MI_EXP_G");                        // >= 1: window groups (tests)
    bool dot2 = !env_is("PLSSVM_MI_EXP_DOT2", "0");           // 0: the FMA chain instead of the dot instructions
};

// The remainder's symmetric rows [r0, r1), the product of every join: row r's partners j != r with H_rj != 0 possible
// (ascending, both triangles) and their H at (sj, sv)[rbeg[r] .. rend[r]). A join fills it and reports so; a join
// that gives up leaves it reset.
template <typename T>
struct sym_rows {
    dev_buf<int64_t> off8;         // [R + 1] row offsets (rows padded to 8 slots): rbeg = off8, rend = off8 + 1 ...
    dev_buf<int32_t> sj;
    dev_buf<T> sv;
    int64_t nslot8 = 0;            // off8[R]
    dev_buf<int64_t> pbeg, pend;   // ... or [R] each: the one-pass join's ranges inside its fixed slots
    const int64_t *rbeg = nullptr, *rend = nullptr;
    int64_t pairs = 0;             // unordered pairs with H != 0 (in the real type)
    double hratio = -1.0;          // max |H_ij| / |kernel value of the pair| (< 0: unknown, the sort join)
    void rows_from_off8() { rbeg = off8.get(), rend = off8.get() + 1; }
    void reset() {
        sj.reset(), sv.reset(), off8.reset(), pbeg.reset(), pend.reset();
        rbeg = rend = nullptr;
        nslot8 = 0;
        pairs = 0;
        hratio = -1.0;
    }
};

// what the joins read, and the device scalars and counts one join may leave to the next; lives as long as phase 1
template <typename T>
struct join_state {
    engine<T> &en;
    const exp_knobs &kn;
    phase_timer &pt;
    const int64_t *cpos;  // per CSR entry: its position in the CSC
    phi_fn phi;
    int64_t R;            // the rank's rows
    double kbase = 1.0;   // rbf: 1 + E(s); poly: kappa + c(s)
    // the row join's pass boundaries in every column (more rows than one bitmap pass: each row's full passes start at
    // the same partner rows, p x RJ_BMW x 32, so each column's positions there are found once)
    dev_buf<int64_t> csplit;
    int nsplit = 0;
    dev_buf<int64_t> cnt;   // [R] partners per row ...
    bool have_cnt = false;  // ... exact for every row (a one-pass join whose slots were too few)
    dev_buf<unsigned long long> lnz;  // [0] lower pairs with H != 0, [1] max |H| / kernel value (double bits), [2] max cnt
};

// what a join strategy reports: the rows are built | not by this strategy, try the next | a row needs more passes than
// the row join allows (or the row join cannot hold it): only the sort join builds these rows
enum class join_out { filled, next, sort };

// H_ii, phi(|x_i|^2) and the buffers of the moments and the row sums
template <typename T>
void alloc_moments_and_diag(engine<T> &en, const phi_fn &phi) {
    auto &csr = en.csr;
    auto &ex = csr.ex;
    hipStream_t stream = en.stream;
    ex.M.alloc(std::max<int64_t>(en.d, 1) * ex.KM, stream);
    ex.mom.alloc(std::max<int64_t>(en.d, 1) * ex.KM, stream);
    csr.ssc.alloc(2, stream);  // device scalar S = sum_j w_j
    ex.hdiag.alloc(en.n_pad, stream);
    ex.hs.alloc(en.n_pad, stream);
    ex.wv.alloc(en.kernel == 2 ? en.n_pad : 1, stream);
    ex.phin.alloc(en.n_pad, stream);
    if (en.m > 0)
        launch(exp_diag_kernel<T>, ceil_div(en.m, 256), 256, stream, csr.rowptr.get(), csr.val.get(), en.m, phi,
               ex.hdiag.get(), ex.phin.get());
}

// Can the row join build this rank's rows (every row within its LDS copy, incidences within int32;
// PLSSVM_MI_EXP_JOIN=sort: no)? Then also the column split table of its passes.
template <typename T>
bool prepare_row_join(join_state<T> &js) {
    auto &en = js.en;
    auto &csr = en.csr;
    const int64_t R = js.R, m = en.m, d = en.d;
    bool row_join = !js.kn.join_sort;
    if (row_join && R > 0) {
        std::vector<int64_t> rp((size_t) (R + 1));
        read_back(rp.data(), csr.rowptr.get() + en.r0, R + 1, en.stream);
        for (int64_t r = 0; r < R && row_join; ++r) row_join = rp[(size_t) r + 1] - rp[(size_t) r] <= RJ_ECAP;
        if (row_join && csr.nnz >= (int64_t) INT32_MAX) row_join = false;  // a row's incidences <= nnz
    }
    if (row_join && R > 0 && d > 0 && m > (int64_t) RJ_BMW * 32 && js.kn.colsplit) {
        js.nsplit = (int) ceil_div(m, (int64_t) RJ_BMW * 32);
        js.csplit.alloc(d * js.nsplit, en.stream, false);
        launch(exp_colsplit_kernel, ceil_div(d * js.nsplit, 256), 256, en.stream, csr.colptr.get(), csr.crow.get(), d,
               js.nsplit, (int64_t) RJ_BMW * 32, js.csplit.get());
    }
    return row_join;
}

// exp_rowjoin_kernel over the rank's rows, one workgroup each (its modes: see the kernel; cposl: the lower triangle)
template <typename T>
void launch_rowjoin(join_state<T> &js, int64_t *cnt, const int64_t *off8, int32_t *sj, unsigned int *ovf, int64_t cap,
                    unsigned long long *cnt_max, const int64_t *cposl = nullptr) {
    auto &en = js.en;
    auto &csr = en.csr;
    launch(exp_rowjoin_kernel, js.R, RJ_NT, en.stream, csr.rowptr.get(), csr.col.get(), csr.colptr.get(), csr.crow.get(), en.m,
           en.r0, cnt, off8, sj, ovf, js.kn.rj_pmax, cap, cnt_max, js.csplit.get(), js.nsplit, cposl);
}

// the H kernel over the partners listed at hj[hb[r] .. he[r]): float evaluation for rbf in a float context
// (exp_rowjoin_h_kernel's F32; PLSSVM_MI_EXP_H64=1: fp64)
template <typename T>
void launch_h(join_state<T> &js, const int64_t *hb, const int64_t *he, int32_t *hj, T *hv) {
    auto &en = js.en;
    auto &csr = en.csr;
    const bool f32 = sizeof(T) == 4 && js.phi.rbf != 0 && !js.kn.h64;
    launch(f32 ? exp_rowjoin_h_kernel<T, true> : exp_rowjoin_h_kernel<T, false>, js.R, RJH_NT, en.stream, csr.rowptr.get(),
           csr.col.get(), csr.val.get(), en.r0, js.phi, js.kbase, hb, he, hj, hv, js.lnz.get(), js.lnz.get() + 1);
}

// the pairs count and the H bound the H kernel left
template <typename T>
void read_lnz(join_state<T> &js, sym_rows<T> &sym) {
    unsigned long long np[2] = { 0ull, 0ull };
    read_back(np, js.lnz.get(), 2, js.en.stream);
    sym.pairs = (int64_t) np[0];
    std::memcpy(&sym.hratio, &np[1], sizeof(double));
}

// H of every listed partner of the rows, then the pairs count and the H bound
template <typename T>
void h_pass(join_state<T> &js, sym_rows<T> &sym) {
    if (js.R > 0) launch_h(js, sym.rbeg, sym.rend, sym.sj.get(), sym.sv.get());
    read_lnz(js, sym);
}

// Lower-triangle join (one rank holding every row): each row joins only its partners j < i (half the incidences), H
// is formed once per unordered pair, and the upper lists are the transpose — a stable radix sort of the lower pairs
// by partner (rows stay ascending within a partner). The symmetric rows, their partners and their H are bit for bit
// those of the full join (H_ij = H_ji: commutative products, features in ascending order). PLSSVM_MI_EXP_LT=0 keeps
// the full join. Anything unusual (a row beyond its slots, a dense cluster, out of memory) gives up: the full join
// recounts the pairs and the H bound, so nothing this join read survives it.
template <typename T>
join_out join_lower_triangle(join_state<T> &js, sym_rows<T> &sym) {
    auto &en = js.en;
    auto &csr = en.csr;
    auto &ex = csr.ex;
    hipStream_t stream = en.stream;
    const int64_t R = js.R, m = en.m;
    if (!js.kn.lt || js.kn.twopass) return join_out::next;
    if (!(R > 0 && R == m && en.r0 == 0 && !en.shard && en.world == 1 && en.sim_world == 0 && js.cpos != nullptr &&
          ex.rj_mean > 0.0 && m < (int64_t) INT32_MAX))
        return join_out::next;
    const int64_t cap = exp_slot_cap(ex.rj_mean, ex.rj_max, js.kn.rj_cap);
    // the slot pool beside the structures the estimate counts; an unknown budget is no room
    const double room = csr.budget_b > 0 ? (double) (csr.budget_b - csr.est_bytes) : 0.0;
    if ((double) R * (double) cap * (double) (4 + sizeof(T)) > room) return join_out::next;
    const auto give_up = [&] {
        sym.reset();
        return join_out::next;
    };
    try {
        dev_buf<int32_t> ls;
        dev_buf<T> lv;
        dev_buf<int64_t> lcnt, lb, le;
        ls.alloc(R * cap, stream, false);
        lcnt.alloc(R + 1, stream);
        js.lnz.alloc(3, stream);
        dev_buf<unsigned int> ovf;
        ovf.alloc(1, stream);
        launch_rowjoin(js, lcnt.get(), nullptr, ls.get(), ovf.get(), cap, js.lnz.get() + 2, js.cpos);
        // the H buffers are mapped while the join runs (a multi-GB hipMalloc is tens of ms of host time)
        lv.alloc(R * cap, stream, false);
        lb.alloc(R, stream, false);
        le.alloc(R, stream, false);
        unsigned int ov = 0u;
        MI_HIP_CHECK(hipMemcpyAsync(&ov, ovf.get(), sizeof(ov), hipMemcpyDeviceToHost, stream));
        const unsigned long long cmax = read_back(js.lnz.get() + 2, stream);
        if (ov != 0u || (int64_t) cmax > cap) return give_up();
        js.pt.mark("expansion: row join, lower triangle");
        launch(exp_pool_range_kernel, ceil_div(R, 256), 256, stream, lcnt.get(), R, cap, lb.get(), le.get());
        launch_h(js, lb.get(), le.get(), ls.get(), lv.get());
        read_lnz(js, sym);  // pairs with H != 0 and the H bound: the lower pairs are every unordered pair
        js.pt.mark("expansion: row join, lower triangle (H)");
        // compact lower pairs, in row order (rows ascending, partners ascending)
        dev_buf<int64_t> loff;
        loff.alloc(R + 1, stream, false);
        exclusive_sum(lcnt.get(), loff.get(), R + 1, stream);  // lcnt[R] = 0 (allocated zeroed)
        const int64_t NL = read_back(loff.get() + R, stream);
        if (NL >= (int64_t) INT32_MAX) return give_up();
        // the transpose's peak: the packed pairs, their sorted copy and the symmetric rows (both triangles) live
        // together once the slot pool is freed — gated on the same room as the pool
        const double tr_b = (double) NL * (double) (2 * (sizeof(uint32_t) + sizeof(lt_val<T>)) + 2 * (4 + sizeof(T))) +
                            4.0 * 8.0 * (double) (R + 1);
        if (tr_b > room) return give_up();
        const int64_t NLa = std::max<int64_t>(NL, 1);
        dev_buf<uint32_t> lk, ks;
        dev_buf<lt_val<T>> lvv, vs;
        lk.alloc(NLa, stream, false);
        lvv.alloc(NLa, stream, false);
        launch(exp_lt_compact_kernel<T>, ceil_div(R, 4), 256, stream, ls.get(), lv.get(), lcnt.get(), loff.get(), R, cap,
               lk.get(), lvv.get());
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        ls.reset(), lv.reset(), lb.reset(), le.reset();
        // the transpose: a stable sort of the pairs by partner (their row order kept within a partner)
        ks.alloc(NLa, stream, false);
        vs.alloc(NLa, stream, false);
        if (NL > 0) {
            int end_bit = 1;
            while (end_bit < 32 && (int64_t(1) << end_bit) < m) ++end_bit;
            size_t tb = 0;
            MI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, lk.get(), ks.get(), lvv.get(), vs.get(), (int) NL,
                                                            0, end_bit, stream));
            dev_buf<unsigned char> t;
            t.alloc((int64_t) std::max<size_t>(tb, 16), stream, false);
            MI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(t.get(), tb, lk.get(), ks.get(), lvv.get(), vs.get(), (int) NL,
                                                            0, end_bit, stream));
        }
        // the symmetric rows: row r = its lower list, then its upper list (ascending partners throughout)
        dev_buf<int64_t> tot, ustart;
        tot.alloc(R + 1, stream, false);
        ustart.alloc(R + 1, stream, false);
        launch(exp_lt_runs_kernel, ceil_div(R + 1, 256), 256, stream, ks.get(), NL, lcnt.get(), R, ustart.get(), tot.get());
        sym.off8.alloc(R + 1, stream, false);
        exclusive_sum(tot.get(), sym.off8.get(), R + 1, stream);
        sym.nslot8 = read_back(sym.off8.get() + R, stream);
        sym.sj.alloc(std::max<int64_t>(sym.nslot8, 8), stream, false);
        sym.sv.alloc(std::max<int64_t>(sym.nslot8, 8), stream, false);
        if (NL > 0)
            launch(exp_lt_place_kernel<T>, ceil_div(NL, 256), 256, stream, lk.get(), lvv.get(), ks.get(), vs.get(), NL,
                   loff.get(), lcnt.get(), ustart.get(), sym.off8.get(), sym.sj.get(), sym.sv.get());
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        sym.rows_from_off8();
        js.pt.mark("expansion: row join, transpose");
        return join_out::filled;
    } catch (const std::exception &e) {
        if (exception_code(e) != -4) throw;
        (void) hipGetLastError();
        return give_up();
    }
}

// One pass of the full join into fixed per-row slot ranges of cap partners (exp_rowjoin_kernel's slot mode, no count
// pass), cap from the setup's sample of the rank's rows (estimate_expansion_bytes). A row beyond its slots: the two
// passes, with the counts this pass took. PLSSVM_MI_EXP_RJ=twopass: not tried.
template <typename T>
join_out join_one_pass(join_state<T> &js, sym_rows<T> &sym) {
    auto &en = js.en;
    auto &csr = en.csr;
    auto &ex = csr.ex;
    hipStream_t stream = en.stream;
    const int64_t R = js.R;
    if (R <= 0) return join_out::next;
    const int64_t cap = exp_slot_cap(ex.rj_mean, ex.rj_max, js.kn.rj_cap);
    // the slot pool beside the structures the estimate counts: gated on the budget left over by the estimate, both
    // taken before the SELL plans' host thread allocates — the same choice on every run; an unknown budget: 40 % of
    // the free memory
    double room = (double) (csr.budget_b - csr.est_bytes);
    if (csr.budget_b <= 0) {
        size_t free_b = 0, total_b = 0;
        MI_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        room = 0.4 * (double) free_b;
    }
    const double pool_b = (double) R * (double) cap * (double) (4 + sizeof(T));
    if (js.kn.twopass || !(ex.rj_mean > 0.0) || pool_b > room) return join_out::next;
    sym.sj.alloc(R * cap, stream, false);
    js.cnt.alloc(R, stream);
    js.lnz.alloc(3, stream);
    dev_buf<unsigned int> ovf;
    ovf.alloc(1, stream);
    launch_rowjoin(js, js.cnt.get(), nullptr, sym.sj.get(), ovf.get(), cap, js.lnz.get() + 2);
    unsigned int ov = 0u;
    MI_HIP_CHECK(hipMemcpyAsync(&ov, ovf.get(), sizeof(ov), hipMemcpyDeviceToHost, stream));
    const unsigned long long cmax = read_back(js.lnz.get() + 2, stream);
    js.pt.mark("expansion: row join (one pass)");
    if (ov != 0u) {  // a row whose partner clusters need more than RJ_PMAX passes
        sym.reset();
        js.cnt.reset();
        return join_out::sort;
    }
    if ((int64_t) cmax > cap) {  // a row beyond its slots: the two-pass join with these exact counts
        sym.reset();
        js.have_cnt = true;
        return join_out::next;
    }
    sym.sv.alloc(R * cap, stream, false);
    sym.pbeg.alloc(R, stream, false);
    sym.pend.alloc(R, stream, false);
    launch(exp_pool_range_kernel, ceil_div(R, 256), 256, stream, js.cnt.get(), R, cap, sym.pbeg.get(), sym.pend.get());
    sym.rbeg = sym.pbeg.get();
    sym.rend = sym.pend.get();
    h_pass(js, sym);
    js.pt.mark("expansion: row join (H)");
    return join_out::filled;
}

// Two passes of the full join: count (unless the one-pass join counted), padded offsets, then the write pass and H
template <typename T>
join_out join_two_pass(join_state<T> &js, sym_rows<T> &sym) {
    hipStream_t stream = js.en.stream;
    const int64_t R = js.R;
    sym.off8.alloc(R + 1, stream);
    if (!js.have_cnt) js.cnt.alloc(std::max<int64_t>(R, 1), stream);
    dev_buf<int64_t> cnt8;
    cnt8.alloc(R + 1, stream);
    js.lnz.alloc(3, stream);
    dev_buf<unsigned int> ovf;
    ovf.alloc(1, stream);
    if (R > 0 && !js.have_cnt) launch_rowjoin(js, js.cnt.get(), nullptr, nullptr, ovf.get(), 0, nullptr);  // count mode
    if (R > 0) launch(exp_pad8_cnt_kernel, ceil_div(R, 256), 256, stream, js.cnt.get(), R, cnt8.get());
    exclusive_sum(cnt8.get(), sym.off8.get(), R + 1, stream);
    MI_HIP_CHECK(hipMemcpyAsync(&sym.nslot8, sym.off8.get() + R, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    const unsigned int ov = read_back(ovf.get(), stream);
    js.pt.mark("expansion: row join (count)");
    if (ov != 0u) {  // a row whose partner clusters need more than RJ_PMAX passes
        sym.reset();
        return join_out::sort;
    }
    sym.sj.alloc(std::max<int64_t>(sym.nslot8, 8), stream, false);
    sym.sv.alloc(std::max<int64_t>(sym.nslot8, 8), stream, false);
    if (R > 0) launch_rowjoin(js, js.cnt.get(), sym.off8.get(), sym.sj.get(), nullptr, 0, nullptr);  // write mode
    sym.rows_from_off8();
    h_pass(js, sym);
    js.pt.mark("expansion: row join (rows)");
    return join_out::filled;
}

// The column-join sort (PLSSVM_MI_EXP_JOIN=sort, rows longer than the row join's LDS copy, rows beyond its pass cap):
// every incidence (i, j < i, a, phi(a)) generated, radix-sorted and reduced by key, block of rows by block of rows;
// the kept lower pairs then placed into both triangles. Always builds the rows (or throws).
template <typename T>
void join_sort(join_state<T> &js, sym_rows<T> &sym) {
    auto &en = js.en;
    auto &csr = en.csr;
    auto &pt = js.pt;
    hipStream_t stream = en.stream;
    const int64_t R = js.R, m = en.m, r0 = en.r0, r1 = en.r1;
    const int64_t *cpos = js.cpos;
    const phi_fn &phi = js.phi;
    // ---- incidences per row (host) -> row sub-blocks of at most CAP incidences ----
    std::vector<int64_t> inc(std::max<int64_t>(m, 1), 0);
    {
        dev_buf<int64_t> cnt;
        cnt.alloc(std::max<int64_t>(m, 1), stream);
        if (m > 0)
            launch(exp_count_kernel, ceil_div(m, 256), 256, stream, csr.rowptr.get(), csr.col.get(), cpos, csr.colptr.get(),
                   (int64_t) 0, m, cnt.get());
        read_back(inc.data(), cnt.get(), m, stream);
    }
    constexpr int64_t CAP = int64_t(1) << 27;  // incidences per sub-block (≈ 80 B each in flight)
    constexpr int64_t ROWS_MAX = 65536;        // rows per sub-block (one workgroup per row)
    std::vector<std::pair<int64_t, int64_t>> blocks;
    {
        int64_t a = r0, acc = 0;  // pairs (i, j < i) touch rows [r0, r1) only if i >= r0
        for (int64_t i = r0; i < m; ++i) {
            if (inc[i] > CAP) throw mi_error(-4, "a data point shares features with more than 2^27 others (dense row)");
            if (i > a && (acc + inc[i] > CAP || i - a >= ROWS_MAX)) {
                blocks.emplace_back(a, i);
                a = i;
                acc = 0;
            }
            acc += inc[i];
        }
        if (a < m) blocks.emplace_back(a, m);
    }
    int64_t max_blk = 1;
    for (auto &b : blocks) {
        int64_t s = 0;
        for (int64_t i = b.first; i < b.second; ++i) s += inc[i];
        max_blk = std::max(max_blk, s);
    }

    // ---- temporaries: sized once here, so the loop over the blocks allocates nothing ----
    dev_buf<uint64_t> keys, keys_s;
    dev_buf<double2> vals, vals_s;
    dev_buf<hpair> hp, hsel;
    dev_buf<int64_t> cntb, off, nruns, nsel;
    keys.alloc(max_blk, stream, false);
    keys_s.alloc(max_blk, stream, false);
    vals.alloc(max_blk, stream, false);
    vals_s.alloc(max_blk, stream, false);
    cntb.alloc(ROWS_MAX + 1, stream);
    off.alloc(ROWS_MAX + 1, stream);
    nruns.alloc(1, stream);
    nsel.alloc(1, stream);
    size_t tmp_sort = 0, tmp_scan = 0, tmp_red = 0, tmp_sel = 0;
    const int nmax = (int) max_blk;
    MI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, keys.get(), keys_s.get(), vals.get(), vals_s.get(),
                                                    nmax, 0, 64, stream));
    MI_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_scan, cntb.get(), off.get(), (int) (ROWS_MAX + 1), stream));
    MI_HIP_CHECK(hipcub::DeviceReduce::ReduceByKey(nullptr, tmp_red, keys_s.get(), keys.get(), vals_s.get(), vals.get(),
                                                   nruns.get(), d2sum(), nmax, stream));
    hp.alloc(max_blk, stream, false);
    hsel.alloc(max_blk, stream, false);
    MI_HIP_CHECK(hipcub::DeviceSelect::If(nullptr, tmp_sel, hp.get(), hsel.get(), nsel.get(), nmax,
                                          h_keep{ 0, r0, r1, sizeof(T) == 4 }, stream));
    dev_buf<unsigned char> tmp;
    tmp.alloc((int64_t) std::max({ tmp_sort, tmp_scan, tmp_red, tmp_sel, (size_t) 16 }), stream, false);

    // growable list of kept lower pairs (li > lj), in (li, lj) order
    dev_buf<int32_t> Li, Lj;
    dev_buf<T> Lh;
    int64_t P = 0, cap = 0;
    auto grow = [&](int64_t need) {
        if (need <= cap) return;
        const int64_t nc = std::max<int64_t>(need, cap + cap / 2 + 1024);
        dev_buf<int32_t> ni, nj;
        dev_buf<T> nh;
        ni.alloc(nc, stream, false);
        nj.alloc(nc, stream, false);
        nh.alloc(nc, stream, false);
        if (P > 0) {
            MI_HIP_CHECK(hipMemcpyAsync(ni.get(), Li.get(), sizeof(int32_t) * (size_t) P, hipMemcpyDeviceToDevice, stream));
            MI_HIP_CHECK(hipMemcpyAsync(nj.get(), Lj.get(), sizeof(int32_t) * (size_t) P, hipMemcpyDeviceToDevice, stream));
            MI_HIP_CHECK(hipMemcpyAsync(nh.get(), Lh.get(), sizeof(T) * (size_t) P, hipMemcpyDeviceToDevice, stream));
        }
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        Li = std::move(ni);
        Lj = std::move(nj);
        Lh = std::move(nh);
        cap = nc;
    };
    double st_gen = 0, st_sort = 0, st_red = 0, st_sel = 0;  // PLSSVM_MI_TIMING: stage seconds
    auto stage = [&](double &acc) {
        if (!pt.on) return;
        MI_HIP_CHECK(hipStreamSynchronize(stream));
        const auto now = std::chrono::steady_clock::now();
        acc += std::chrono::duration<double>(now - pt.t).count();
        pt.t = now;
    };
    for (auto &b : blocks) {
        const int64_t i0 = b.first, rows = b.second - b.first;
        int64_t total = 0;
        for (int64_t i = b.first; i < b.second; ++i) total += inc[i];
        if (total == 0) continue;
        launch(exp_count_kernel, ceil_div(rows, 256), 256, stream, csr.rowptr.get(), csr.col.get(), cpos, csr.colptr.get(),
               i0, b.second, cntb.get());
        size_t ts = tmp_scan;
        MI_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.get(), ts, cntb.get(), off.get(), (int) (rows + 1), stream));
        launch(exp_gen_kernel<T>, rows, 256, stream, csr.rowptr.get(), csr.col.get(), csr.val.get(), cpos, csr.colptr.get(),
               csr.crow.get(), csr.cval.get(), i0, off.get(), keys.get(), vals.get(), phi);
        stage(st_gen);
        const int end_bit = 32 + std::max(1, (int) std::ceil(std::log2((double) rows + 1.0)));
        size_t t1s = tmp_sort;
        MI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.get(), t1s, keys.get(), keys_s.get(), vals.get(), vals_s.get(),
                                                        (int) total, 0, end_bit, stream));
        stage(st_sort);
        size_t t2s = tmp_red;
        MI_HIP_CHECK(hipcub::DeviceReduce::ReduceByKey(tmp.get(), t2s, keys_s.get(), keys.get(), vals_s.get(), vals.get(),
                                                       nruns.get(), d2sum(), (int) total, stream));
        launch(exp_h_kernel, ceil_div(total, 256), 256, stream, keys.get(), vals.get(), nruns.get(), phi, hp.get());
        stage(st_red);
        const int64_t nu = read_back(nruns.get(), stream);
        size_t t3s = tmp_sel;
        MI_HIP_CHECK(hipcub::DeviceSelect::If(tmp.get(), t3s, hp.get(), hsel.get(), nsel.get(), (int) nu,
                                              h_keep{ i0, r0, r1, sizeof(T) == 4 }, stream));
        const int64_t ns = read_back(nsel.get(), stream);
        if (ns == 0) continue;
        grow(P + ns);
        launch(exp_append_kernel<T>, ceil_div(ns, 256), 256, stream, hsel.get(), nsel.get(), i0, Li.get() + P, Lj.get() + P,
               Lh.get() + P);
        P += ns;
        stage(st_sel);
    }
    if (pt.on)
        std::fprintf(stderr, "[plssvm_mi] column join: %zu blocks, gen %.3f sort %.3f reduce %.3f select+append %.3f\n",
                     blocks.size(), st_gen, st_sort, st_red, st_sel);
    keys.reset(), keys_s.reset(), vals.reset(), vals_s.reset(), hp.reset(), hsel.reset(), tmp.reset();
    pt.mark("expansion: column join (blocks)");
    if (P > INT32_MAX) throw mi_error(-5, "more than 2^31 multi-feature pairs on one rank: use more GPUs");

    // ---- symmetric rows [r0, r1), padded to 8 slots ----
    dev_buf<unsigned long long> clo, cup;
    dev_buf<int64_t> cnt8, lo_start, up_start;
    dev_buf<uint32_t> ukey, ukey_s, uidx, uidx_s;
    clo.alloc(std::max<int64_t>(R, 1), stream);
    cup.alloc(std::max<int64_t>(R, 1), stream);
    cnt8.alloc(R + 1, stream);
    sym.off8.alloc(R + 1, stream);
    lo_start.alloc(R + 1, stream);
    up_start.alloc(R + 1, stream);
    ukey.alloc(std::max<int64_t>(P, 1), stream, false);
    if (P > 0)
        launch(exp_hist_kernel, ceil_div(P, 256), 256, stream, Li.get(), Lj.get(), P, r0, r1, clo.get(), cup.get(),
               ukey.get());
    if (R > 0)
        launch(exp_pad8_kernel, ceil_div(R, 256), 256, stream, clo.get(), cup.get(), R, cnt8.get());
    exclusive_sum(cnt8.get(), sym.off8.get(), R + 1, stream);
    exclusive_sum(clo.get(), lo_start.get(), R, stream);
    exclusive_sum(cup.get(), up_start.get(), R, stream);
    MI_HIP_CHECK(hipStreamSynchronize(stream));
    {
        // rows' lower pairs are the list's prefix (sorted by li); count them
        std::vector<unsigned long long> hlo(std::max<int64_t>(R, 1), 0);
        read_back(hlo.data(), clo.get(), R, stream);
        for (int64_t r = 0; r < R; ++r) sym.pairs += (int64_t) hlo[r];
    }
    // padded symmetric rows (temporary): row r's entries in [off8[r], off8[r + 1]), sorted by j
    sym.nslot8 = read_back(sym.off8.get() + R, stream);
    dev_buf<int32_t> scrow;
    sym.sj.alloc(std::max<int64_t>(sym.nslot8, 8), stream, false);
    sym.sv.alloc(std::max<int64_t>(sym.nslot8, 8), stream);
    scrow.alloc(std::max<int64_t>(sym.nslot8 / 8, 1), stream, false);
    if (R > 0)
        launch(exp_init_rows_kernel<T>, ceil_div(R, 4), 256, stream, sym.off8.get(), R, r0, sym.sj.get(), sym.sv.get(),
               scrow.get());
    scrow.reset();
    if (P > 0) {
        launch(exp_place_lower_kernel<T>, ceil_div(P, 256), 256, stream, Li.get(), Lj.get(), Lh.get(), P, r0, r1,
               lo_start.get(), sym.off8.get(), sym.sj.get(), sym.sv.get());
        // upper part: entries with j in [r0, r1), stably sorted by j (their li order is kept)
        uidx.alloc(P, stream, false);
        ukey_s.alloc(P, stream, false);
        uidx_s.alloc(P, stream, false);
        {
            launch(exp_iota_kernel, ceil_div(P, 256), 256, stream, uidx.get(), P);
            size_t tb = 0;
            MI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ukey.get(), ukey_s.get(), uidx.get(), uidx_s.get(),
                                                            (int) P, 0, 32, stream));
            dev_buf<unsigned char> t;
            t.alloc((int64_t) std::max<size_t>(tb, 16), stream, false);
            MI_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(t.get(), tb, ukey.get(), ukey_s.get(), uidx.get(), uidx_s.get(),
                                                            (int) P, 0, 32, stream));
            MI_HIP_CHECK(hipStreamSynchronize(stream));
        }
        int64_t nup = 0;
        {
            std::vector<unsigned long long> hup(std::max<int64_t>(R, 1), 0);
            read_back(hup.data(), cup.get(), R, stream);
            for (int64_t r = 0; r < R; ++r) nup += (int64_t) hup[r];
        }
        if (nup > 0)
            launch(exp_place_upper_kernel<T>, ceil_div(nup, 256), 256, stream, ukey_s.get(), uidx_s.get(), nup, Li.get(),
                   Lh.get(), clo.get(), up_start.get(), sym.off8.get(), sym.sj.get(), sym.sv.get());
    }
    Li.reset(), Lj.reset(), Lh.reset(), uidx.reset(), ukey.reset(), ukey_s.reset(), uidx_s.reset();
    sym.rows_from_off8();
}

// H storage (float contexts): bfloat16 when every stored |H_ij| is at most 2^-16 of its pair's kernel value (the row
// join's hratio; see "H storage" in build_cells). A sharded group gathers bfloat16 w or real w by this flag
// (expansion_kp_raw), so a real group takes it once: the AND over the ranks, after every rank's join. Phase 1 may have
// failed on this rank only (fail1; memory, a dense row): before_agree — the caller's concurrent step (the SELL plans),
// joined here, its failure counts as ours — and the agreement are still reached, and the agreement raises the same
// error on every rank.
template <typename T>
bool agree_h_storage(engine<T> &en, const exp_knobs &kn, std::exception_ptr fail1,
                     const std::function<std::exception_ptr()> &before_agree, double hratio) {
    if (before_agree) {
        std::exception_ptr e = before_agree();
        if (e && !fail1) fail1 = e;
    }
    bool hb_ok = !fail1 && sizeof(T) == 4 && hratio >= 0.0 && hratio <= std::ldexp(1.0, -16) && !kn.hfmt_full;
    if (en.in_group()) {
        int code = 0;
        std::string why;
        if (fail1) {
            try {
                std::rethrow_exception(fail1);
            } catch (const std::exception &e) {
                code = exception_code(e);
                why = e.what();
            } catch (...) {
                code = -1;
                why = "unknown exception in the expansion setup";
            }
        }
        const auto g = en.group_step(code, why, { hb_ok ? 1.0 : 0.0 });  // throws on every rank if any failed
        for (double v : g) hb_ok = hb_ok && v != 0.0;
    } else if (fail1) {
        std::rethrow_exception(fail1);
    }
    return hb_ok;
}

// the remainder stream's geometry (exp_geometry.hpp): blocks of RB rows x windows of CW partners, G window groups
template <typename T>
void choose_geometry(engine<T> &en, const exp_knobs &kn, bool hb_ok) {
    auto &ex = en.csr.ex;
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, en.device) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    const int64_t R = en.r1 - en.r0;
    exp_geometry g = exp_choose_geometry(R, cus, (int) sizeof(T), kn.rbb, kn.g);
    ex.hbf16 = hb_ok;
    exp_set_windows(g, (int) sizeof(T), ex.hbf16, en.m);
    ex.RBB = g.RBB, ex.RB = g.RB, ex.G = g.G, ex.CW = g.CW, ex.nW = g.nW;
    ex.nblk = ceil_div(R, (int64_t) ex.RB);
}

// The cells of the remainder stream from the symmetric rows: per (row, window) cell its slots counted, the layout
// chosen (a row index per chunk, chunk flags or pair flags), the entries scattered and the (block, wave, window)
// offsets written.
//
// H storage (float contexts): bfloat16 H and bfloat16 windows of w when every stored |H_ij| is at most 2^-16 of its
// pair's kernel value (row join's hratio). H_ij w_j is then formed from two values with relative error <= 2^-9 each,
// so each pair's term moves by at most ~2^-8 |H_ij w_j| <= 2^-24 of the pair's k_ij w_j — the float rounding of that
// term itself. PLSSVM_MI_EXP_HFMT=full keeps the real type. The bfloat16 window holds twice the partners (fewer
// windows, fewer padded cells). ex.hbf16: agreed by the whole group (agree_h_storage).
template <typename T>
void build_cells(engine<T> &en, const exp_knobs &kn, const sym_rows<T> &sym) {
    auto &ex = en.csr.ex;
    hipStream_t stream = en.stream;
    const int64_t R = en.r1 - en.r0, m = en.m, RB = ex.RB, CW = ex.CW, nbv = ex.nblk * EXP_NWV;
    {
        const int64_t ncnt = ex.nblk * RB * ex.nW;
        dev_buf<int64_t> cnt, coff;
        cnt.alloc(ncnt + 1, stream);
        coff.alloc(ncnt + 1, stream, false);
        auto scan = [&] {  // coff = the cells' first slots, ex.slots = their total; synchronises
            exclusive_sum(cnt.get(), coff.get(), ncnt + 1, stream);
            ex.slots = read_back(coff.get() + ncnt, stream);
        };
        auto count_cells = [&](int64_t gran) {  // a cell with entries: their count rounded up to gran slots
            if (R <= 0) return;
            launch(exp_cell_count_kernel<T>, ceil_div(R, 4), 256, stream, sym.rbeg, sym.rend, sym.sj.get(), sym.sv.get(), R,
                   ex.nW, CW, RB, gran, cnt.get());
        };
        auto fill_empty = [&](int64_t gran) {  // a cell without entries: one dummy of gran slots
            launch(exp_cell_fill_empty_kernel, ceil_div(R * ex.nW, 256), 256, stream, R, ex.nW, RB, gran, cnt.get());
        };
        auto recount = [&](int64_t gran) {  // the flagged layouts' counts from scratch
            MI_HIP_CHECK(hipMemsetAsync(cnt.get(), 0, sizeof(int64_t) * (size_t) (ncnt + 1), stream));
            count_cells(gran);
            fill_empty(gran);
        };
        count_cells(4);
        // flagged chunks (bfloat16 H only; the rule: exp_take_chunk_flags). PLSSVM_MI_EXP_ROWS=index keeps the row
        // index, =flags forces the flags (when the bit is free)
        ex.rflags = false;
        ex.rpairs = false;
        if (ex.hbf16 && R > 0 && kn.rows >= 0) {
            dev_buf<unsigned long long> st;
            st.alloc(2, stream);
            launch(exp_cell_stats_kernel<T>, ceil_div(R, 4), 256, stream, sym.rbeg, sym.rend, sym.sj.get(), sym.sv.get(), R,
                   ex.nW, CW, st.get());
            unsigned long long hs2[2] = { 0ull, 0ull };  // the cells without entries; any |H| >= 2
            MI_HIP_CHECK(hipMemcpyAsync(hs2, st.get(), sizeof(hs2), hipMemcpyDeviceToHost, stream));
            scan();  // ex.slots = the indexed layout's slots
            ex.rflags = exp_take_chunk_flags((int64_t) hs2[0], hs2[1] != 0, ex.slots, kn.rows);
            if (ex.rflags) fill_empty(4);
            // pair flags: the flags on slot pairs, cells padded to 2 slots instead of 4 (the 4-slot padding is ~15 % of
            // the stream on config 5's 2M geometry; the rule: exp_take_pair_flags). PLSSVM_MI_EXP_ROWS=pairs forces
            // it, =flags keeps the chunk flags
            if (ex.rflags && kn.rows != EXP_ROWS_FLAGS) {
                scan();
                const int64_t slots4 = ex.slots;
                recount(2);
                const int64_t ngroups = nbv * ex.nW, RPW = RB / EXP_NWV;
                launch(exp_cell_pad_groups_kernel, ceil_div(ngroups, 256), 256, stream, ngroups, RPW, cnt.get());
                scan();
                ex.rpairs = exp_take_pair_flags(ex.slots, slots4, kn.rows);
                if (!ex.rpairs) recount(4);  // back to the chunk-flag counts
            }
        }
        scan();
        ex.nchunks = ex.slots / 4;
        // EXP_NH x 64 chunks of zeroed padding past the stream's end: the remainder stream's loads of a step
        // past the end read padding (masked) instead of clamping each lane's 64-bit address
        const int64_t spad = std::max<int64_t>(ex.slots, 4) + (int64_t) EXP_NH * 64 * 4;
        ex.hjl.alloc(spad * (ex.rflags && EXP_JH ? 2 : 1), stream);
        if (ex.hbf16) {
            if (ex.rflags && EXP_JH) ex.hv16.reset();
            else ex.hv16.alloc(spad, stream);
            ex.wv16.alloc(round_up(std::max<int64_t>({ m, en.chunk * en.G, 8 }), (int64_t) 8), stream);
        } else {
            ex.hv.alloc(spad, stream);
        }
        if (ex.rflags) {
            ex.hrow.reset();
            launch(exp_cell_scatter_flag_kernel<T>, ceil_div(R, 4), 256, stream, sym.rbeg, sym.rend, sym.sj.get(),
                   sym.sv.get(), R, ex.nW, CW, RB, coff.get(), ex.hjl.get(), EXP_JH ? ex.hjl.get() : ex.hv16.get());
        } else {
            ex.hrow.alloc(std::max<int64_t>(ex.nchunks, 1) + (int64_t) EXP_NH * 64, stream);
            if (R > 0)
                launch(exp_cell_scatter_kernel<T>, ceil_div(R, 4), 256, stream, sym.rbeg, sym.rend, sym.sj.get(),
                       sym.sv.get(), R, ex.nW, CW, RB, coff.get(), ex.hjl.get(), ex.hv.get(), ex.hv16.get(), ex.hrow.get());
        }
        ex.woff.alloc(std::max<int64_t>(nbv * (ex.nW + 1), 1), stream);
        if (nbv > 0)
            launch(exp_cell_woff_kernel, ceil_div(nbv * (ex.nW + 1), 256), 256, stream, coff.get(), nbv, ex.nW, RB,
                   ex.woff.get());
        MI_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (ex.G > 1) ex.hslab.alloc((int64_t) ex.G * R, stream, false);
    MI_HIP_CHECK(hipStreamSynchronize(stream));
}

}  // namespace

// Setup: H_ii and the moment buffers; the remainder H of the pairs sharing >= 2 features as symmetric rows [r0, r1),
// by the first join strategy that can build them — lower triangle + transpose, one pass into slots, two passes, and
// the column-join sort, which always can; the group's agreement on failure and on H's storage format; the remainder
// stream's geometry and its cells.
template <typename T>
void engine<T>::build_expansion(const int64_t *cpos, int64_t /*max_inc*/,
                                const std::function<std::exception_ptr()> &before_agree) {
    auto &ex = csr.ex;
    phase_timer pt;
    const exp_knobs kn{};
    ex.dot2 = kn.dot2;
    sym_rows<T> sym;
    bool lt = false;
    // phase 1 (the symmetric rows) may fail on one rank only (memory, a dense row): in a real group every rank
    // still reaches the agreement after it, which raises the same error everywhere
    std::exception_ptr fail1;
    try {
        join_state<T> js{ *this, kn, pt, cpos, make_phi<T>(kernel, degree, gamma, coef0), r1 - r0 };
        if (kernel == 1)
            for (int q2 = 0; q2 < degree; ++q2) js.kbase *= (double) coef0;
        alloc_moments_and_diag(*this, js.phi);
        join_out o = prepare_row_join(js) ? join_out::next : join_out::sort;
        if (o == join_out::next) o = join_lower_triangle(js, sym);
        lt = o == join_out::filled;
        if (o == join_out::next) o = join_one_pass(js, sym);
        if (o == join_out::next) o = join_two_pass(js, sym);
        if (o != join_out::filled) join_sort(js, sym);
        pt.mark("expansion: symmetric rows");
    } catch (...) {
        fail1 = std::current_exception();
    }
    ex.pairs = sym.pairs;
    ex.hratio = sym.hratio;
    ex.lt = lt;
    const bool hb_ok = agree_h_storage(*this, kn, fail1, before_agree, sym.hratio);
    choose_geometry(*this, kn, hb_ok);
    build_cells(*this, kn, sym);
    pt.mark("expansion: cells");
    csr.pairs = ex.pairs;
    csr.slots = ex.slots;
    csr.rbf_factored = kernel == 2;
    ex.on = true;
}

void exp_setup_load_code_object() {
    hipFuncAttributes a;
    (void) hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&exp_rowjoin_kernel));
}

#define INST(T)                                    \
    template bool engine<T>::expansion_eligible(); \
    template void engine<T>::build_expansion(const int64_t *, int64_t, const std::function<std::exception_ptr()> &);
INST(float)
INST(double)
#undef INST

}  // namespace plssvm_mi
