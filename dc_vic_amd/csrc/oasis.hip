// oasis.hip -- the OASIS GAN loss (reference: src/losses/oasis_gan_loss.py `OasisGANLoss.forward`, and
// src/trainer/dual_cond_oasis_gan_distortion_vq_code_trainer.py `calc_avg_d_score_for_log`) as ONE pass over the discriminator's
// logits [N][C][HW]: the (C = n_embed + 1)-way cross entropy per VQ token position against `index + 1` (real) or 0 (fake), its
// gradient, and the mean of the channels 1.. that the trainer logs.
//
// Layout of the work.  A workgroup of 16 waves owns 64 consecutive positions of one image: lane = position, so every channel row
// a wave touches is one contiguous 256-byte segment.  The waves split the channel axis interleaved (wave w owns c = w, w + 16, ...);
// up to OASIS_KREG * 16 = 272 channels (the trainer has 257) a lane keeps its slice of the logits in registers, so the logits are
// read exactly once and the gradient is written from registers.  Wider tensors stream: an online (max, sum) pass, then -- only
// when the gradient is asked for -- a second read of the logits.  Per-wave (max, sum) pairs meet in LDS and every wave merges
// them in wave order, so all 16 waves hold the same bits.  Per-workgroup fp64 partials of the loss and of the class >= 1 sum go
// to the workspace; a one-workgroup pass adds them in a fixed order.  No atomics: the same inputs give the same bits on every run.
#include "common.h"

#define OASIS_WAVES 16
#define OASIS_KREG 17
#define OASIS_POS 64

namespace {

__device__ __forceinline__ double oasis_wsum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool CACHED>
__global__ __launch_bounds__(OASIS_WAVES * 64) void oasis_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                    float* __restrict__ dlogits, double* __restrict__ part, int C, int HW,
                                                                    int tiles, int is_real, float scale) {
    __shared__ float s_m[OASIS_WAVES][OASIS_POS], s_s[OASIS_WAVES][OASIS_POS];
    __shared__ float s_t[OASIS_POS];
    __shared__ double s_red[OASIS_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x / tiles, p = (blockIdx.x % tiles) * OASIS_POS + lane;
    const bool active = p < HW;
    const float* lp = logits + (long long)n * C * HW + p;
    // effective class: index + 1 (real) or 0 (fake); -1 marks an index outside the codebook (the loss becomes NaN, nothing is indexed by it)
    int t = 0;
    if (active && is_real) {
        const long long tt = (long long)target[(long long)n * HW + p] + 1;
        t = (tt >= 1 && tt < C) ? (int)tt : -1;
    }
    if (w == 0 && t < 0) s_t[lane] = __builtin_nanf("");

    float v[OASIS_KREG];
    float m = -INFINITY, s = 0.f;
    double sc = 0.0;                                   // sum of this thread's logits of class >= 1
    if (CACHED) {
#pragma unroll
        for (int k = 0; k < OASIS_KREG; ++k) {
            const int c = w + OASIS_WAVES * k;
            v[k] = (active && c < C) ? lp[(long long)c * HW] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < OASIS_KREG; ++k) m = fmaxf(m, v[k]);
#pragma unroll
        for (int k = 0; k < OASIS_KREG; ++k) {
            const int c = w + OASIS_WAVES * k;
            if (active && c < C) {
                s += expf(v[k] - m);
                if (c >= 1) sc += (double)v[k];
                if (c == t) s_t[lane] = v[k];
            }
        }
    } else if (active) {
        for (int c0 = w; c0 < C; c0 += 4 * OASIS_WAVES) {
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + OASIS_WAVES * j;
                x[j] = c < C ? lp[(long long)c * HW] : -INFINITY;
            }
            const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
            if (mx > m) {
                s *= expf(m - mx);                     // (first round: s = 0 and expf(-inf) = 0)
                m = mx;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + OASIS_WAVES * j;
                if (c < C) {
                    s += expf(x[j] - m);
                    if (c >= 1) sc += (double)x[j];
                    if (c == t) s_t[lane] = x[j];
                }
            }
        }
    }
    s_m[w][lane] = m;
    s_s[w][lane] = s;
    __syncthreads();

    double loss_p = 0.0;
    if (active) {
        float M = -INFINITY, S = 0.f;
#pragma unroll
        for (int i = 0; i < OASIS_WAVES; ++i) M = fmaxf(M, s_m[i][lane]);
#pragma unroll
        for (int i = 0; i < OASIS_WAVES; ++i) S += s_s[i][lane] * expf(s_m[i][lane] - M);     // a wave without channels: 0 * expf(-inf) = 0
        loss_p = (double)logf(S) + ((double)M - (double)s_t[lane]);
        if (dlogits) {
            float* dp = dlogits + (long long)n * C * HW + p;
            const float inv = 1.f / S;
            if (CACHED) {
#pragma unroll
                for (int k = 0; k < OASIS_KREG; ++k) {
                    const int c = w + OASIS_WAVES * k;
                    if (c < C) dp[(long long)c * HW] = scale * (expf(v[k] - M) * inv - (c == t ? 1.f : 0.f));
                }
            } else {
                for (int c = w; c < C; c += OASIS_WAVES)
                    dp[(long long)c * HW] = scale * (expf(lp[(long long)c * HW] - M) * inv - (c == t ? 1.f : 0.f));
            }
        }
    }
    // workgroup partials: the loss from wave 0 (every wave holds the same values), the class >= 1 sum over the waves in order
    const double L = oasis_wsum_d(loss_p), Q = oasis_wsum_d(sc);
    if (lane == 0) s_red[w] = Q;
    __syncthreads();
    if (threadIdx.x == 0) {
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < OASIS_WAVES; ++i) q += s_red[i];
        part[2 * (long long)blockIdx.x] = L;
        part[2 * (long long)blockIdx.x + 1] = q;
    }
}

// one workgroup: thread i adds the partials i, i + 256, ... in ascending order, then the 256 sums are added lane-tree by wave
__global__ __launch_bounds__(256) void oasis_ce_final_kernel(const double* __restrict__ part, int blocks, double scale, double inv_count,
                                                             float* __restrict__ loss, float* __restrict__ score) {
    __shared__ double red[2][4];
    double l = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) {
        l += part[2 * (long long)i];
        q += part[2 * (long long)i + 1];
    }
    l = oasis_wsum_d(l);
    q = oasis_wsum_d(q);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = l;
        red[1][threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        loss[0] = (float)((((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) * scale);
        if (score) score[0] = (float)((((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) * inv_count);
    }
}

long long oasis_blocks(int N, int HW) {
    if (N <= 0 || HW <= 0) return 0;
    return (long long)N * dcvic_cdiv(HW, OASIS_POS);
}

}  // namespace

extern "C" long long dcvic_oasis_ce_workspace_doubles(int N, int HW) { return 2 * oasis_blocks(N, HW); }

extern "C" int dcvic_oasis_ce_f32(const float* logits, const int64_t* target, int is_real, double scale, float* loss, float* dlogits,
                                  float* score, double* workspace, int N, int C, int HW, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && HW > 0, "oasis_ce: empty tensor N=%d HW=%d", N, HW);
    DCVIC_CHECK_ARG(C >= 2, "oasis_ce: C=%d, needs the fake class and at least one codebook entry (C >= 2)", C);
    DCVIC_CHECK_ARG(logits && loss && workspace, "oasis_ce: null pointer (logits %p, loss %p, workspace %p)", (const void*)logits, (void*)loss,
                    (void*)workspace);
    DCVIC_CHECK_ARG(target || !is_real, "oasis_ce: null target with is_real");
    const long long blocks = oasis_blocks(N, HW);
    DCVIC_CHECK_ARG(blocks <= 0x3fffffff && (long long)C * HW <= 0x7fffffffLL, "oasis_ce: N=%d C=%d HW=%d too large", N, C, HW);
    const int tiles = dcvic_cdiv(HW, OASIS_POS);
    if (C <= OASIS_KREG * OASIS_WAVES)
        oasis_ce_kernel<true><<<(unsigned)blocks, OASIS_WAVES * 64, 0, (hipStream_t)stream>>>(logits, target, dlogits, workspace, C, HW, tiles,
                                                                                                  is_real ? 1 : 0, (float)scale);
    else
        oasis_ce_kernel<false><<<(unsigned)blocks, OASIS_WAVES * 64, 0, (hipStream_t)stream>>>(logits, target, dlogits, workspace, C, HW, tiles,
                                                                                                   is_real ? 1 : 0, (float)scale);
    DCVIC_CHECK_LAUNCH("oasis_ce");
    oasis_ce_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(workspace, (int)blocks, scale, 1.0 / ((double)N * (double)(C - 1) * (double)HW), loss,
                                                               score);
    DCVIC_CHECK_LAUNCH("oasis_ce_final");
    return DCVIC_OK;
}
