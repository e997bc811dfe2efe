// gumbel.hip -- the hard Gumbel-softmax sample of the VQ indices in training mode (reference: hyperprior_dc_vic_model.py:254-260,
// `F.gumbel_softmax(logits, dim=1, hard=True, **gumbel_kwargs)` times the detached codebook, then post_quant_conv) behind two entry
// points, for a draw e ~ Exp(1) the caller supplies:
//   dcvic_gumbel_lut_f32      z = logits - logf(e); idx = first argmax over the classes; latent = post_quant_conv(codebook[idx])
//   dcvic_gumbel_lut_bwd_f32  dlogits_j = s_j * (v_j - sum_k s_k v_k) / tau with s = softmax(z / tau), v_j = codebook[j] . (pq_w^T glatent):
//                             the derivative of one_hot - s.detach() + s through the frozen codebook and the frozen 1x1 convolution
// include/dcvic_gumbel.h states the contract.
//
// Layout of the work: that of csrc/chan_ce_core.h, whose constants are used.  A workgroup of 16 waves owns 64 consecutive positions of
// one image: lane = position, so every class row a wave touches is one contiguous 256-byte segment.  The waves split the class axis
// interleaved (wave w owns c = w, w + 16, ...).  The forward streams both inputs once and keeps a running (max, index) per lane.  The
// backward keeps, up to KREG * 16 = 272 classes (the shipped codebooks have 256), its slice of z / tau and of v in registers: logits
// and noise are read once and dlogits is written once from registers; wider tensors stream, reading the two inputs three times.  The
// codebook sits in LDS (a wave reads one entry at a time: a broadcast), h in registers.  The per-wave (max, index) pairs and (sum, sum
// s v) pairs meet in LDS and every thread merges them in wave order, so all 16 waves hold the same bits.  No atomics.
//
// The backward's two rounds.  Round one finds the position's largest z / tau, M, and its class I.  v is then formed relative to that
// class, vc_j = v_j - v_I (v_I from the same fmaf chain, so vc_I is exactly 0): sum_k s_k v_k - v_I = sum_k s_k vc_k has no term of
// the dominant class, and v_j - sum_k s_k v_k = vc_j - sum_k s_k vc_k keeps its digits where the softmax saturates (s_I -> 1), where
// the plain form would leave the rounding error of v_I.  Round two sums exp(z / tau - M) and exp(z / tau - M) * vc over the waves.
#include <float.h>

#include "chan_ce_core.h"
#include "dcvic_gumbel.h"
#include "vq_lut.h"

namespace {

using chan_ce::KREG;
using chan_ce::POS;
using chan_ce::WAVES;

constexpr int MAX_D = 8;                 // h lives in registers
constexpr int MAX_CB_FLOATS = 8192;      // the codebook's LDS image: 32 KiB

// z = logit + g with g = -log(e), e clamped to [FLT_MIN, FLT_MAX]: g is finite for every e (a NaN becomes FLT_MIN)
__device__ __forceinline__ float gumbel_z(float logit, float e) { return logit + (-logf(fminf(fmaxf(e, FLT_MIN), FLT_MAX))); }

// the (max, lowest index of it) over the waves' pairs, in wave order; (-inf, 0) where no wave holds a class
__device__ __forceinline__ void merge_max(const float (*s_m)[POS], const int (*s_i)[POS], int lane, float& M, int& I) {
    M = -INFINITY;
    I = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const float m = s_m[i][lane];
        const int j = s_i[i][lane];
        if (m > M || (m == M && j < I)) {
            M = m;
            I = j;
        }
    }
}

__global__ __launch_bounds__(WAVES * 64) void gumbel_lut_kernel(const float* __restrict__ logits, const float* __restrict__ noise,
                                                                int64_t* __restrict__ idx, float* __restrict__ latent,
                                                                const float* __restrict__ cb, const float* __restrict__ pq_w,
                                                                const float* __restrict__ pq_b, int C, int D, int HW, int tiles) {
    __shared__ float s_m[WAVES][POS];
    __shared__ int s_i[WAVES][POS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x / tiles, p = (blockIdx.x % tiles) * POS + lane;
    const bool active = p < HW;
    const long long base = (long long)n * C * HW + p;
    float best = -INFINITY;
    int bi = 0;
    if (active) {
        for (int c0 = w; c0 < C; c0 += 4 * WAVES) {
            float z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + WAVES * j;
                z[j] = c < C ? gumbel_z(logits[base + (long long)c * HW], noise[base + (long long)c * HW]) : -INFINITY;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (z[j] > best) {             // ascending classes, strict: the lowest index of this thread's maximum
                    best = z[j];
                    bi = c0 + WAVES * j;
                }
        }
    }
    s_m[w][lane] = best;
    s_i[w][lane] = bi;
    __syncthreads();
    if (!active) return;
    float M;
    int I;
    merge_max(s_m, s_i, lane, M, I);
    if (w == 0 && idx) idx[(long long)n * HW + p] = (int64_t)I;
    for (int c = w; c < D; c += WAVES) latent[(long long)n * D * HW + (long long)c * HW + p] = dcvic_lut_latent(cb, pq_w, pq_b, I, c, D);
}

// v of class c: codebook[c] . h, one fmaf chain in ascending d (s_cb: the codebook's LDS image)
__device__ __forceinline__ float class_dot(const float* s_cb, int c, int D, const float (&h)[MAX_D]) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < MAX_D; ++d)
        if (d < D) a = fmaf(s_cb[c * D + d], h[d], a);
    return a;
}

template <bool CACHED>
__global__ __launch_bounds__(WAVES * 64) void gumbel_lut_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ noise,
                                                                    const float* __restrict__ glatent, const float* __restrict__ cb,
                                                                    const float* __restrict__ pq_w, float* __restrict__ dlogits, float tau,
                                                                    int C, int D, int HW, int tiles) {
    __shared__ float s_m[WAVES][POS], s_s[WAVES][POS], s_t[WAVES][POS];
    __shared__ int s_i[WAVES][POS];
    extern __shared__ float s_cb[];            // [C][D]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x / tiles, p = (blockIdx.x % tiles) * POS + lane;
    const bool active = p < HW;
    const long long base = (long long)n * C * HW + p;
    const float* lp = logits + base;
    const float* ep = noise + base;
    for (int i = threadIdx.x; i < C * D; i += WAVES * 64) s_cb[i] = cb[i];

    // round one: z / tau, this thread's (max, index)
    float zt[KREG], vc[KREG];
    float m = -INFINITY;
    int mi = 0;
    if (CACHED) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int c = w + WAVES * k;
            zt[k] = (active && c < C) ? gumbel_z(lp[(long long)c * HW], ep[(long long)c * HW]) / tau : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < KREG; ++k)
            if (zt[k] > m) {
                m = zt[k];
                mi = w + WAVES * k;
            }
    } else if (active) {
        for (int c = w; c < C; c += WAVES) {
            const float x = gumbel_z(lp[(long long)c * HW], ep[(long long)c * HW]) / tau;
            if (x > m) {
                m = x;
                mi = c;
            }
        }
    }
    // h = pq_w^T glatent of this position (every wave forms the same bits)
    float h[MAX_D];
#pragma unroll
    for (int d = 0; d < MAX_D; ++d) h[d] = 0.f;
    if (active) {
        for (int c = 0; c < D; ++c) {
            const float g = glatent[(long long)n * D * HW + (long long)c * HW + p];
#pragma unroll
            for (int d = 0; d < MAX_D; ++d)
                if (d < D) h[d] = fmaf(pq_w[c * D + d], g, h[d]);
        }
    }
    s_m[w][lane] = m;
    s_i[w][lane] = mi;
    __syncthreads();                           // also: the codebook's image is complete

    float M;
    int I;
    merge_max(s_m, s_i, lane, M, I);
    const float v_ref = class_dot(s_cb, I, D, h);

    // round two: sum exp(zt - M) and sum exp(zt - M) * vc over this thread's classes; zt becomes exp(zt - M)
    float s = 0.f, t = 0.f;
    if (CACHED) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int c = w + WAVES * k;
            if (active && c < C) {
                zt[k] = expf(zt[k] - M);
                vc[k] = class_dot(s_cb, c, D, h) - v_ref;
                s += zt[k];
                t = fmaf(zt[k], vc[k], t);
            }
        }
    } else if (active) {
        for (int c = w; c < C; c += WAVES) {
            const float e = expf(gumbel_z(lp[(long long)c * HW], ep[(long long)c * HW]) / tau - M);
            s += e;
            t = fmaf(e, class_dot(s_cb, c, D, h) - v_ref, t);
        }
    }
    s_s[w][lane] = s;
    s_t[w][lane] = t;
    __syncthreads();
    if (!active) return;
    float S = 0.f, T = 0.f;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        S += s_s[i][lane];
        T += s_t[i][lane];
    }
    // S >= 1 (the class I contributes exp(0)); a wave without classes adds 0
    const float inv = 1.f / S;
    T *= inv;                                  // sum_k s_k vc_k
    float* dp = dlogits + base;
    if (CACHED) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int c = w + WAVES * k;
            if (c < C) dp[(long long)c * HW] = zt[k] * inv * (vc[k] - T) / tau;
        }
    } else {
        for (int c = w; c < C; c += WAVES) {
            const float e = expf(gumbel_z(lp[(long long)c * HW], ep[(long long)c * HW]) / tau - M);
            dp[(long long)c * HW] = e * inv * ((class_dot(s_cb, c, D, h) - v_ref) - T) / tau;
        }
    }
}

// the checks both entry points share, after their own null-pointer checks
int check_sizes(const char* name, double tau, int N, int C, int D, int HW) {
    DCVIC_CHECK_ARG(N > 0 && C > 0 && D > 0 && HW > 0, "%s: empty tensor N=%d C=%d D=%d HW=%d", name, N, C, D, HW);
    DCVIC_CHECK_ARG(tau > 0.0 && tau <= (double)FLT_MAX && (double)(float)tau > 0.0, "%s: tau=%g, needs a finite value > 0", name, tau);
    DCVIC_CHECK_ARG(N <= 65535, "%s: N=%d, batch too large (at most 65535)", name, N);
    DCVIC_CHECK_ARG(D <= MAX_D, "%s: D=%d, at most %d latent channels", name, D, MAX_D);
    DCVIC_CHECK_ARG((long long)C * D <= MAX_CB_FLOATS, "%s: C=%d D=%d, the codebook is staged in LDS: C * D <= %d", name, C, D, MAX_CB_FLOATS);
    DCVIC_CHECK_ARG(chan_ce::fits(N, C, HW), "%s: N=%d C=%d HW=%d too large", name, N, C, HW);
    return DCVIC_OK;
}

}  // namespace

extern "C" int dcvic_gumbel_lut_f32(const float* logits, const float* noise, int64_t* idx, float* latent, const float* codebook,
                                    const float* pq_w, const float* pq_b, double tau, int N, int C, int D, int HW, void* stream) {
    DCVIC_CHECK_ARG(logits && noise && latent && codebook && pq_w,
                    "gumbel_lut: null pointer (logits %p, noise %p, latent %p, codebook %p, pq_w %p)", (const void*)logits, (const void*)noise,
                    (void*)latent, (const void*)codebook, (const void*)pq_w);
    if (int rc = check_sizes("gumbel_lut", tau, N, C, D, HW)) return rc;
    const int tiles = dcvic_cdiv(HW, POS);
    gumbel_lut_kernel<<<(unsigned)chan_ce::blocks(N, HW), WAVES * 64, 0, (hipStream_t)stream>>>(logits, noise, idx, latent, codebook, pq_w, pq_b, C, D,
                                                                                                HW, tiles);
    DCVIC_CHECK_LAUNCH("gumbel_lut");
    return DCVIC_OK;
}

extern "C" int dcvic_gumbel_lut_bwd_f32(const float* logits, const float* noise, const float* glatent, const float* codebook,
                                        const float* pq_w, double tau, float* dlogits, int N, int C, int D, int HW, void* stream) {
    DCVIC_CHECK_ARG(logits && noise && glatent && codebook && pq_w && dlogits,
                    "gumbel_lut_bwd: null pointer (logits %p, noise %p, glatent %p, codebook %p, pq_w %p, dlogits %p)", (const void*)logits,
                    (const void*)noise, (const void*)glatent, (const void*)codebook, (const void*)pq_w, (void*)dlogits);
    if (int rc = check_sizes("gumbel_lut_bwd", tau, N, C, D, HW)) return rc;
    const int tiles = dcvic_cdiv(HW, POS);
    auto kernel = C <= KREG * WAVES ? gumbel_lut_bwd_kernel<true> : gumbel_lut_bwd_kernel<false>;
    kernel<<<(unsigned)chan_ce::blocks(N, HW), WAVES * 64, (size_t)C * D * sizeof(float), (hipStream_t)stream>>>(logits, noise, glatent, codebook, pq_w,
                                                                                                              dlogits, (float)tau, C, D, HW, tiles);
    DCVIC_CHECK_LAUNCH("gumbel_lut_bwd");
    return DCVIC_OK;
}
