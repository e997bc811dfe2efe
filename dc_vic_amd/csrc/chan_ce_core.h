// chan_ce_core.h -- the one-pass cross entropy over the channel axis of logits [N][C][HW] that csrc/chan_ce.hip (dcvic_oasis_ce_f32,
// dcvic_focal_ce_f32) and csrc/sample_loss.hip (dcvic_focal_ce_sample_f32) launch.  The layout of the work and the three places
// where OASIS and focal differ are described at the head of chan_ce.hip; WEIGHTED replaces the one factor `scale` on the gradient by
// image n's own weight wgt[n] and changes nothing else: the per-workgroup partials stay the unweighted sums of f.
#pragma once
#include "common.h"

namespace chan_ce {

constexpr int WAVES = 16, KREG = 17, POS = 64;

__device__ __forceinline__ double wsum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// is_real is read by the OASIS instantiation only, gamma by the focal one only, wgt by the WEIGHTED one only (which does not read scale)
template <bool CACHED, bool OASIS, bool WEIGHTED = false>
__global__ __launch_bounds__(WAVES * 64) void chan_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                             float* __restrict__ dlogits, double* __restrict__ part, int C, int HW, int tiles,
                                                             int is_real, double gamma, float scale, const float* __restrict__ wgt) {
    __shared__ float s_m[WAVES][POS], s_s[WAVES][POS];
    __shared__ float s_t[POS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x / tiles, p = (blockIdx.x % tiles) * POS + lane;
    const bool active = p < HW;
    const float* lp = logits + (long long)n * C * HW + p;
    // effective class; -1 marks one outside the valid range (the loss becomes NaN, nothing is indexed by it)
    constexpr int SHIFT = OASIS ? 1 : 0;
    int t = 0;
    if (active && (!OASIS || is_real)) {
        const long long tt = (long long)target[(long long)n * HW + p] + SHIFT;
        t = (tt >= SHIFT && tt < C) ? (int)tt : -1;
    }
    if (w == 0 && t < 0) s_t[lane] = __builtin_nanf("");

    float v[KREG];
    float m = -INFINITY, s = 0.f;
    double sc = 0.0;                                   // OASIS: sum of this thread's logits of class >= 1
    if (CACHED) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int c = w + WAVES * k;
            v[k] = (active && c < C) ? lp[(long long)c * HW] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < KREG; ++k) m = fmaxf(m, v[k]);
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int c = w + WAVES * k;
            if (active && c < C) {
                s += expf(v[k] - m);
                if (OASIS && c >= 1) sc += (double)v[k];
                if (c == t) s_t[lane] = v[k];
            }
        }
    } else if (active) {
        for (int c0 = w; c0 < C; c0 += 4 * WAVES) {
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + WAVES * j;
                x[j] = c < C ? lp[(long long)c * HW] : -INFINITY;
            }
            const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
            if (mx > m) {
                s *= expf(m - mx);                     // (first round: s = 0 and expf(-inf) = 0)
                m = mx;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + WAVES * j;
                if (c < C) {
                    s += expf(x[j] - m);
                    if (OASIS && c >= 1) sc += (double)x[j];
                    if (c == t) s_t[lane] = x[j];
                }
            }
        }
    }
    s_m[w][lane] = m;
    s_s[w][lane] = s;
    __syncthreads();

    double f_p = 0.0;
    if (active) {
        float M = -INFINITY, S = 0.f;
#pragma unroll
        for (int i = 0; i < WAVES; ++i) M = fmaxf(M, s_m[i][lane]);
#pragma unroll
        for (int i = 0; i < WAVES; ++i) S += s_s[i][lane] * expf(s_m[i][lane] - M);     // a wave without channels: 0 * expf(-inf) = 0
        // S >= 1 and M >= z_t, so ce >= 0 and q stays in [0, 1]
        const double ce = (double)logf(S) + ((double)M - (double)s_t[lane]);
        double A = 1.0;                                // d f / d ce, the factor on (p_j - [j == t])
        f_p = ce;
        if constexpr (!OASIS) {
            if (gamma != 0.0) {
                const double pt = exp(-ce), q = -expm1(-ce);
                const double qg1 = pow(q, gamma - 1.0);    // gamma >= 1: pow(0, 0) = 1, pow(0, > 0) = 0, never Inf
                const double qg = qg1 * q;
                f_p = qg * ce;
                A = qg + gamma * qg1 * pt * ce;
            }
        }
        if (dlogits) {
            float* dp = dlogits + (long long)n * C * HW + p;
            float image_scale = scale;
            if constexpr (WEIGHTED) image_scale = wgt[n];
            const float inv = 1.f / S, coef = image_scale * (float)A;     // OASIS: scale * 1.f is scale
            if (CACHED) {
#pragma unroll
                for (int k = 0; k < KREG; ++k) {
                    const int c = w + WAVES * k;
                    if (c < C) dp[(long long)c * HW] = coef * (expf(v[k] - M) * inv - (c == t ? 1.f : 0.f));
                }
            } else {
                for (int c = w; c < C; c += WAVES)
                    dp[(long long)c * HW] = coef * (expf(lp[(long long)c * HW] - M) * inv - (c == t ? 1.f : 0.f));
            }
        }
    }
    // workgroup partials: the value from wave 0 (every wave holds the same values); OASIS: the class >= 1 sum over the waves in order
    constexpr int STRIDE = OASIS ? 2 : 1;
    if (w == 0) {
        const double L = wsum_d(f_p);
        if (lane == 0) part[STRIDE * (long long)blockIdx.x] = L;
    }
    if constexpr (OASIS) {
        __shared__ double s_red[WAVES];
        const double Q = wsum_d(sc);
        if (lane == 0) s_red[w] = Q;
        __syncthreads();
        if (threadIdx.x == 0) {
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < WAVES; ++i) q += s_red[i];
            part[2 * (long long)blockIdx.x + 1] = q;
        }
    }
}

// workgroups of one launch: dcvic_cdiv(HW, POS) per image, image after image
inline long long blocks(int N, int HW) {
    if (N <= 0 || HW <= 0) return 0;
    return (long long)N * dcvic_cdiv(HW, POS);
}

// the sizes one launch can index, after the entry point's own argument checks
inline bool fits(int N, int C, int HW) { return blocks(N, HW) <= 0x3fffffff && (long long)C * HW <= 0x7fffffffLL; }

}  // namespace chan_ce
