// What the kernel expansion's two files share: expand.hip runs per K·p and per predict,
// expand_setup.hip builds the stored remainder once per setup.
#pragma once

#include <cmath>

#include "cg_common.hpp"
#include "engine.hpp"

namespace plssvm_mi {

int exp_ablate();                   // expand.hip: PLSSVM_MI_EXP_ABLATE (timing/test-only ablations)
void exp_setup_load_code_object();  // expand_setup.hip: its code object loaded (exp_load_code_object calls it)

namespace {

using cgk::bf16_rne;

// phi in double: the exact per-pair function (rbf: expm1(2 g a); poly: sum_k bin_k a^k, no cancellation).
// rbf with |u| = |2 g a| < 2^-7 (every pair of the BASELINE sets: u <= 2 g max x^2 ~ 1e-4): the Taylor
// polynomial of degree 7, whose remainder u^8 / 8! is below 2^-54 |u| there — fp64 accuracy in 8 fma instead of
// the library expm1's range reduction (the setup's remainder kernels evaluate phi once per wave step)
struct phi_fn {
    int rbf = 0, deg = 0;
    double g2 = 0.0;                   // rbf: 2 g
    double bin[EXP_KMAX + 1] = {};     // poly: C(deg, k) c0^(deg - k) g^k
    __host__ __device__ double operator()(double a) const {
        if (rbf) {
            const double u = g2 * a;
            if (fabs(u) < 0x1p-7) {
                double p = 1.0 / 5040.0;
                p = fma(p, u, 1.0 / 720.0);
                p = fma(p, u, 1.0 / 120.0);
                p = fma(p, u, 1.0 / 24.0);
                p = fma(p, u, 1.0 / 6.0);
                p = fma(p, u, 0.5);
                p = fma(p, u, 1.0);
                return p * u;
            }
            return expm1(u);
        }
        double h = 0.0;
        for (int k = deg; k >= 1; --k) h = (h + bin[k]) * a;
        return h;
    }
};

// bitmap word L of the join (partner rows 32 L .. 32 L + 31 of the pass) lives at LDS word (L % WPT) NT + L / WPT:
// thread t owns the contiguous words t WPT .. t WPT + WPT - 1 (its count and its ascending enumeration), and at
// each step of those loops the 64 lanes read consecutive LDS words — one bank each (word t WPT + w of a plain
// layout put every lane of a wave on the same bank: 64-way conflicts)
template <int WPT, int NT>
__device__ __forceinline__ int bm_addr(int64_t L) {
    return (int) (L % WPT) * NT + (int) (L / WPT);
}

#ifndef EXP_JH
#define EXP_JH 1  // flagged layout: a chunk's 4 indices and 4 bfloat16 H side by side (one 16-byte load per lane)
#endif
#ifndef EXP_NH
#define EXP_NH 2  // remainder stream: groups of 64 chunks per lane step (bytes in flight per wave)
#endif

template <typename T>
phi_fn make_phi(int kernel, int degree, T gamma, T coef0) {
    phi_fn phi;
    if (kernel == 2) {
        phi.rbf = 1;
        phi.g2 = 2.0 * (double) gamma;
    } else {
        phi.deg = degree;
        double binom = 1.0;
        for (int k = 1; k <= degree && k <= EXP_KMAX; ++k) {
            binom = binom * (double) (degree - k + 1) / (double) k;
            phi.bin[k] = binom * std::pow((double) coef0, (double) (degree - k)) * std::pow((double) gamma, (double) k);
        }
    }
    return phi;
}

}  // namespace

}  // namespace plssvm_mi
