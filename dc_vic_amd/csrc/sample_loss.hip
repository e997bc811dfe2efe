// sample_loss.hip -- the two code losses of the rate-distortion trainers with one weight per image (include/dcvic_sample_loss.h;
// reference: src/trainer/dual_cond_rate_distortion_vq_code_trainer.py:71-98,189-198 `apply_loss_weight` over the maps of
// FocalCrossEntropyLoss / VanillaMSELoss with reduction 'none').  Both are  loss = sum_n w[n] * S[n]  with S[n] image n's own sum:
//   dcvic_focal_ce_sample_f32  launches chan_ce_kernel (csrc/chan_ce_core.h) with WEIGHTED: the arithmetic of dcvic_focal_ce_f32, the
//                              factor on the gradient is w[n] in place of the one scale;
//   dcvic_sq_err_sample_f32    S[n] = sum (a - b)^2 and da = 2 w[n] (a - b) in one pass over a and b.
//
// Every first-pass workgroup belongs to ONE image and writes the unweighted fp64 sum of its elements to the workspace, `per` partials
// per image, image after image.  sample_final_kernel (one workgroup, four waves) gives each image to one wave: lane i adds the image's
// partials i, i + 64, ... in ascending order, a lane tree adds the 64 sums -- so S[n] depends on image n's partials alone and is the same
// bits in a batch of 1 and of N.  Wave v adds w[n] * S[n] over n = v, v + 4, ... in ascending order, then the four sums are added in
// order.  No atomics: the same inputs give the same bits on every run.
#include "chan_ce_core.h"
#include "dcvic_sample_loss.h"

namespace {

using chan_ce::wsum_d;

constexpr int SQ_THREADS = 256, SQ_PER_THREAD = 8, SQ_MAX_BLOCKS = 64;

// workgroups per image of sq_err_sample_kernel: one per 2048 elements, at most 64; a larger image is walked by a grid stride
long long sq_err_blocks(long long M) {
    if (M <= 0) return 0;
    const long long b = (M + SQ_THREADS * SQ_PER_THREAD - 1) / (SQ_THREADS * SQ_PER_THREAD);
    return b < SQ_MAX_BLOCKS ? b : SQ_MAX_BLOCKS;
}

// workgroup (n, b) of `per` per image: thread t takes the elements b * 256 + t + k * per * 256, k ascending
__global__ __launch_bounds__(SQ_THREADS) void sq_err_sample_kernel(const float* __restrict__ a, long long a_bs, const float* __restrict__ b,
                                                                   const float* __restrict__ w, float* __restrict__ da,
                                                                   double* __restrict__ part, long long M, int per) {
    __shared__ double red[SQ_THREADS / 64];
    const int n = blockIdx.x / per, blk = blockIdx.x % per;
    const float* ap = a + (long long)n * a_bs;
    const float* bp = b + (long long)n * M;
    float* dp = da ? da + (long long)n * M : nullptr;
    const float w2 = 2.f * w[n];
    const long long stride = (long long)per * SQ_THREADS;
    double s = 0.0;
    for (long long i = (long long)blk * SQ_THREADS + threadIdx.x; i < M; i += stride) {
        const float x = ap[i], y = bp[i];
        const double d = (double)x - (double)y;
        s += d * d;
        if (dp) dp[i] = w2 * (x - y);
    }
    s = wsum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void sample_final_kernel(const double* __restrict__ part, int per, int N, const float* __restrict__ w,
                                                           float* __restrict__ loss, float* __restrict__ per_sample) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, v = threadIdx.x >> 6;
    double total = 0.0;
    for (int n = v; n < N; n += 4) {
        const double* pn = part + (long long)n * per;
        double s = 0.0;
        for (int i = lane; i < per; i += 64) s += pn[i];
        s = wsum_d(s);
        if (lane == 0 && per_sample) per_sample[n] = (float)s;
        total += (double)w[n] * s;
    }
    if (lane == 0) red[v] = total;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

}  // namespace

extern "C" long long dcvic_focal_ce_sample_workspace_doubles(int N, int HW) { return chan_ce::blocks(N, HW); }

extern "C" long long dcvic_sq_err_sample_workspace_doubles(int N, long long M) { return N > 0 ? (long long)N * sq_err_blocks(M) : 0; }

extern "C" int dcvic_focal_ce_sample_f32(const float* logits, const int64_t* target, const float* w, double gamma, float* loss, float* dlogits,
                                         float* per_sample, double* workspace, int N, int C, int HW, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && C > 0 && HW > 0, "focal_ce_sample: empty tensor N=%d C=%d HW=%d", N, C, HW);
    DCVIC_CHECK_ARG(C >= 2, "focal_ce_sample: C=%d, a cross entropy needs at least two classes (C >= 2)", C);
    DCVIC_CHECK_ARG(gamma == 0.0 || gamma >= 1.0,
                    "focal_ce_sample: gamma=%g, needs 0 (plain cross entropy) or >= 1 (the derivative is unbounded at p_t = 1 for 0 < gamma < 1)",
                    gamma);
    DCVIC_CHECK_ARG(logits && target && w && loss && workspace,
                    "focal_ce_sample: null pointer (logits %p, target %p, w %p, loss %p, workspace %p)", (const void*)logits, (const void*)target,
                    (const void*)w, (void*)loss, (void*)workspace);
    DCVIC_CHECK_ARG(chan_ce::fits(N, C, HW), "focal_ce_sample: N=%d C=%d HW=%d too large", N, C, HW);
    const long long blocks = chan_ce::blocks(N, HW);
    const int tiles = dcvic_cdiv(HW, chan_ce::POS);
    auto kernel = C <= chan_ce::KREG * chan_ce::WAVES ? chan_ce::chan_ce_kernel<true, false, true> : chan_ce::chan_ce_kernel<false, false, true>;
    kernel<<<(unsigned)blocks, chan_ce::WAVES * 64, 0, (hipStream_t)stream>>>(logits, target, dlogits, workspace, C, HW, tiles, 0, gamma, 0.f, w);
    DCVIC_CHECK_LAUNCH("focal_ce_sample");
    sample_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(workspace, tiles, N, w, loss, per_sample);
    DCVIC_CHECK_LAUNCH("focal_ce_sample_final");
    return DCVIC_OK;
}

extern "C" int dcvic_sq_err_sample_f32(const float* a, long long a_bs, const float* b, const float* w, float* loss, float* da, float* per_sample,
                                       double* workspace, int N, long long M, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && M > 0, "sq_err_sample: empty tensor N=%d M=%lld", N, M);
    DCVIC_CHECK_ARG(a_bs >= M, "sq_err_sample: batch stride %lld of a below its %lld elements per image", a_bs, M);
    DCVIC_CHECK_ARG(a && b && w && loss && workspace, "sq_err_sample: null pointer (a %p, b %p, w %p, loss %p, workspace %p)", (const void*)a,
                    (const void*)b, (const void*)w, (void*)loss, (void*)workspace);
    const int per = (int)sq_err_blocks(M);
    DCVIC_CHECK_ARG((long long)N * per <= 0x3fffffff && M <= (1LL << 40), "sq_err_sample: N=%d M=%lld too large", N, M);
    sq_err_sample_kernel<<<(unsigned)(N * per), SQ_THREADS, 0, (hipStream_t)stream>>>(a, a_bs, b, w, da, workspace, M, per);
    DCVIC_CHECK_LAUNCH("sq_err_sample");
    sample_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(workspace, per, N, w, loss, per_sample);
    DCVIC_CHECK_LAUNCH("sq_err_sample_final");
    return DCVIC_OK;
}
