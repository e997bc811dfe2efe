// focal.hip -- focal cross entropy over the channel axis (reference: src/losses/cross_entropy_loss.py:33-53
// `FocalCrossEntropyLoss.forward`) as ONE pass over the logits [N][C][HW]: per position ce = logsumexp_c(z) - z[t], p_t = exp(-ce),
// f = (1 - p_t)^gamma * ce, the scaled sum of f, and d/dz_j = (p_j - [j == t]) * (q^gamma + gamma * q^(gamma-1) * p_t * ce).
//
// Layout of the work (csrc/oasis.hip solves the same shape and is the model).  A workgroup of 16 waves owns 64 consecutive
// positions of one image: lane = position, so every channel row a wave touches is one contiguous 256-byte segment.  The waves
// split the channel axis interleaved (wave w owns c = w, w + 16, ...); up to FOCAL_KREG * 16 = 272 channels (the trainer has 256)
// a lane keeps its slice of the logits in registers, so the logits are read exactly once and the gradient is written from
// registers.  Wider tensors stream: an online (max, sum) pass, then -- only when the gradient is asked for -- a second read.
// Per-wave (max, sum) pairs meet in LDS and every wave merges them in wave order, so all 16 waves hold the same bits.  The
// per-position focal factor is formed in fp64 from ce: q = -expm1(-ce) keeps its digits as p_t -> 1, where 1 - exp(-ce) has none.
// Per-workgroup fp64 partials go to the workspace; a one-workgroup pass adds them in a fixed order.  No atomics.
#include "common.h"
#include "dcvic_loss.h"

#define FOCAL_WAVES 16
#define FOCAL_KREG 17
#define FOCAL_POS 64

namespace {

__device__ __forceinline__ double focal_wsum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool CACHED>
__global__ __launch_bounds__(FOCAL_WAVES * 64) void focal_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                    float* __restrict__ dlogits, double* __restrict__ part, int C, int HW,
                                                                    int tiles, double gamma, float scale) {
    __shared__ float s_m[FOCAL_WAVES][FOCAL_POS], s_s[FOCAL_WAVES][FOCAL_POS];
    __shared__ float s_t[FOCAL_POS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x / tiles, p = (blockIdx.x % tiles) * FOCAL_POS + lane;
    const bool active = p < HW;
    const float* lp = logits + (long long)n * C * HW + p;
    // -1 marks a class outside [0, C): the loss becomes NaN, nothing is indexed by it
    int t = 0;
    if (active) {
        const long long tt = (long long)target[(long long)n * HW + p];
        t = (tt >= 0 && tt < C) ? (int)tt : -1;
    }
    if (w == 0 && t < 0) s_t[lane] = __builtin_nanf("");

    float v[FOCAL_KREG];
    float m = -INFINITY, s = 0.f;
    if (CACHED) {
#pragma unroll
        for (int k = 0; k < FOCAL_KREG; ++k) {
            const int c = w + FOCAL_WAVES * k;
            v[k] = (active && c < C) ? lp[(long long)c * HW] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < FOCAL_KREG; ++k) m = fmaxf(m, v[k]);
#pragma unroll
        for (int k = 0; k < FOCAL_KREG; ++k) {
            const int c = w + FOCAL_WAVES * k;
            if (active && c < C) {
                s += expf(v[k] - m);
                if (c == t) s_t[lane] = v[k];
            }
        }
    } else if (active) {
        for (int c0 = w; c0 < C; c0 += 4 * FOCAL_WAVES) {
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + FOCAL_WAVES * j;
                x[j] = c < C ? lp[(long long)c * HW] : -INFINITY;
            }
            const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
            if (mx > m) {
                s *= expf(m - mx);                     // (first round: s = 0 and expf(-inf) = 0)
                m = mx;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + FOCAL_WAVES * j;
                if (c < C) {
                    s += expf(x[j] - m);
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
        for (int i = 0; i < FOCAL_WAVES; ++i) M = fmaxf(M, s_m[i][lane]);
#pragma unroll
        for (int i = 0; i < FOCAL_WAVES; ++i) S += s_s[i][lane] * expf(s_m[i][lane] - M);     // a wave without channels: 0 * expf(-inf) = 0
        // S >= 1 and M >= z_t, so ce >= 0 and q stays in [0, 1]
        const double ce = (double)logf(S) + ((double)M - (double)s_t[lane]);
        double A = 1.0;                                // d f / d ce, the factor on (p_j - [j == t])
        f_p = ce;
        if (gamma != 0.0) {
            const double pt = exp(-ce), q = -expm1(-ce);
            const double qg1 = pow(q, gamma - 1.0);    // gamma >= 1: pow(0, 0) = 1, pow(0, > 0) = 0, never Inf
            const double qg = qg1 * q;
            f_p = qg * ce;
            A = qg + gamma * qg1 * pt * ce;
        }
        if (dlogits) {
            float* dp = dlogits + (long long)n * C * HW + p;
            const float inv = 1.f / S, coef = scale * (float)A;
            if (CACHED) {
#pragma unroll
                for (int k = 0; k < FOCAL_KREG; ++k) {
                    const int c = w + FOCAL_WAVES * k;
                    if (c < C) dp[(long long)c * HW] = coef * (expf(v[k] - M) * inv - (c == t ? 1.f : 0.f));
                }
            } else {
                for (int c = w; c < C; c += FOCAL_WAVES)
                    dp[(long long)c * HW] = coef * (expf(lp[(long long)c * HW] - M) * inv - (c == t ? 1.f : 0.f));
            }
        }
    }
    // workgroup partial from wave 0: every wave holds the same values
    if (w == 0) {
        const double L = focal_wsum_d(f_p);
        if (lane == 0) part[blockIdx.x] = L;
    }
}

// one workgroup: thread i adds the partials i, i + 256, ... in ascending order, then the 256 sums are added lane-tree by wave
__global__ __launch_bounds__(256) void focal_ce_final_kernel(const double* __restrict__ part, int blocks, double scale, float* __restrict__ loss) {
    __shared__ double red[4];
    double l = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) l += part[i];
    l = focal_wsum_d(l);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) * scale);
}

long long focal_blocks(int N, int HW) {
    if (N <= 0 || HW <= 0) return 0;
    return (long long)N * dcvic_cdiv(HW, FOCAL_POS);
}

}  // namespace

extern "C" long long dcvic_focal_ce_workspace_doubles(int N, int HW) { return focal_blocks(N, HW); }

extern "C" int dcvic_focal_ce_f32(const float* logits, const int64_t* target, double gamma, double scale, float* loss, float* dlogits,
                                  double* workspace, int N, int C, int HW, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && C > 0 && HW > 0, "focal_ce: empty tensor N=%d C=%d HW=%d", N, C, HW);
    DCVIC_CHECK_ARG(C >= 2, "focal_ce: C=%d, a cross entropy needs at least two classes (C >= 2)", C);
    DCVIC_CHECK_ARG(gamma == 0.0 || gamma >= 1.0,
                    "focal_ce: gamma=%g, needs 0 (plain cross entropy) or >= 1 (the derivative is unbounded at p_t = 1 for 0 < gamma < 1)", gamma);
    DCVIC_CHECK_ARG(logits && target && loss && workspace, "focal_ce: null pointer (logits %p, target %p, loss %p, workspace %p)",
                    (const void*)logits, (const void*)target, (void*)loss, (void*)workspace);
    const long long blocks = focal_blocks(N, HW);
    DCVIC_CHECK_ARG(blocks <= 0x3fffffff && (long long)C * HW <= 0x7fffffffLL, "focal_ce: N=%d C=%d HW=%d too large", N, C, HW);
    const int tiles = dcvic_cdiv(HW, FOCAL_POS);
    if (C <= FOCAL_KREG * FOCAL_WAVES)
        focal_ce_kernel<true><<<(unsigned)blocks, FOCAL_WAVES * 64, 0, (hipStream_t)stream>>>(logits, target, dlogits, workspace, C, HW, tiles, gamma,
                                                                                                  (float)scale);
    else
        focal_ce_kernel<false><<<(unsigned)blocks, FOCAL_WAVES * 64, 0, (hipStream_t)stream>>>(logits, target, dlogits, workspace, C, HW, tiles, gamma,
                                                                                                   (float)scale);
    DCVIC_CHECK_LAUNCH("focal_ce");
    focal_ce_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(workspace, (int)blocks, scale, loss);
    DCVIC_CHECK_LAUNCH("focal_ce_final");
    return DCVIC_OK;
}
