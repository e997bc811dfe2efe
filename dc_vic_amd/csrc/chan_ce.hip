// chan_ce.hip -- the cross entropy over the channel axis of logits [N][C][HW] as ONE pass, behind two entry points:
//   dcvic_oasis_ce_f32  the OASIS GAN loss (reference: src/losses/oasis_gan_loss.py `OasisGANLoss.forward`, and
//                       src/trainer/dual_cond_oasis_gan_distortion_vq_code_trainer.py `calc_avg_d_score_for_log`): the
//                       (C = n_embed + 1)-way cross entropy per VQ token position against `index + 1` (real) or 0 (fake), its
//                       gradient, and the mean of the channels 1.. that the trainer logs;
//   dcvic_focal_ce_f32  focal cross entropy (reference: src/losses/cross_entropy_loss.py:33-53 `FocalCrossEntropyLoss.forward`):
//                       per position ce = logsumexp_c(z) - z[t], p_t = exp(-ce), f = (1 - p_t)^gamma * ce, the scaled sum of f,
//                       and d/dz_j = (p_j - [j == t]) * (q^gamma + gamma * q^(gamma-1) * p_t * ce).
//
// Layout of the work.  A workgroup of 16 waves owns 64 consecutive positions of one image: lane = position, so every channel row
// a wave touches is one contiguous 256-byte segment.  The waves split the channel axis interleaved (wave w owns c = w, w + 16, ...);
// up to KREG * 16 = 272 channels (the trainers have 257 and 256) a lane keeps its slice of the logits in registers, so the logits
// are read exactly once and the gradient is written from registers.  Wider tensors stream: an online (max, sum) pass, then -- only
// when the gradient is asked for -- a second read of the logits.  Per-wave (max, sum) pairs meet in LDS and every wave merges
// them in wave order, so all 16 waves hold the same bits.  Per-workgroup fp64 partials go to the workspace; a one-workgroup pass
// adds them in a fixed order.  No atomics: the same inputs give the same bits on every run.
//
// The kernel (csrc/chan_ce_core.h, shared with csrc/sample_loss.hip) is one template; its OASIS flag selects the three places where the two losses differ:
//   1. the effective class: OASIS `is_real ? target + 1, valid in [1, C) : 0` (target may be null when fake); focal `target`,
//      valid in [0, C);
//   2. OASIS also sums each thread's logits of class >= 1 in fp64 (the logged score): a second double per workgroup partial;
//   3. the per-position value f and the factor A on (p_j - [j == t]): OASIS f = ce, A = 1; focal f = q^gamma * ce,
//      A = q^gamma + gamma * q^(gamma-1) * p_t * ce, formed in fp64 from ce: q = -expm1(-ce) keeps its digits as p_t -> 1, where
//      1 - exp(-ce) has none.  At gamma = 0 focal is f = ce, A = 1 and gives the bits of OASIS on the shifted classes.
#include "chan_ce_core.h"
#include "dcvic_loss.h"

namespace {

using chan_ce::KREG;
using chan_ce::POS;
using chan_ce::WAVES;
using chan_ce::chan_ce_kernel;
using chan_ce::wsum_d;

// one workgroup: thread i adds the partials i, i + 256, ... in ascending order, then the 256 sums are added lane-tree by wave.
// OASIS: two doubles per workgroup partial, the second is the class >= 1 sum behind `score` (which may be null)
template <bool OASIS>
__global__ __launch_bounds__(256) void chan_ce_final_kernel(const double* __restrict__ part, int blocks, double scale, double inv_count,
                                                            float* __restrict__ loss, float* __restrict__ score) {
    constexpr int STRIDE = OASIS ? 2 : 1;
    __shared__ double red[STRIDE][4];
    double l = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) {
        l += part[STRIDE * (long long)i];
        if constexpr (OASIS) q += part[2 * (long long)i + 1];
    }
    l = wsum_d(l);
    if constexpr (OASIS) q = wsum_d(q);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = l;
        if constexpr (OASIS) red[1][threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        loss[0] = (float)((((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) * scale);
        if constexpr (OASIS)
            if (score) score[0] = (float)((((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) * inv_count);
    }
}

// the size check and the launches, after the entry point's own argument checks
template <bool OASIS>
int chan_ce_launch(const float* logits, const int64_t* target, int is_real, double gamma, double scale, float* loss, float* dlogits, float* score,
                   double* workspace, int N, int C, int HW, hipStream_t stream) {
    constexpr const char* name = OASIS ? "oasis_ce" : "focal_ce";
    const long long blocks = chan_ce::blocks(N, HW);
    DCVIC_CHECK_ARG(chan_ce::fits(N, C, HW), "%s: N=%d C=%d HW=%d too large", name, N, C, HW);
    const int tiles = dcvic_cdiv(HW, POS);
    auto kernel = C <= KREG * WAVES ? chan_ce_kernel<true, OASIS> : chan_ce_kernel<false, OASIS>;
    kernel<<<(unsigned)blocks, WAVES * 64, 0, stream>>>(logits, target, dlogits, workspace, C, HW, tiles, is_real, gamma, (float)scale, nullptr);
    DCVIC_CHECK_LAUNCH(name);
    chan_ce_final_kernel<OASIS><<<1, 256, 0, stream>>>(workspace, (int)blocks, scale, 1.0 / ((double)N * (double)(C - 1) * (double)HW), loss, score);
    DCVIC_CHECK_LAUNCH(OASIS ? "oasis_ce_final" : "focal_ce_final");
    return DCVIC_OK;
}

}  // namespace

extern "C" long long dcvic_oasis_ce_workspace_doubles(int N, int HW) { return 2 * chan_ce::blocks(N, HW); }

extern "C" long long dcvic_focal_ce_workspace_doubles(int N, int HW) { return chan_ce::blocks(N, HW); }

extern "C" int dcvic_oasis_ce_f32(const float* logits, const int64_t* target, int is_real, double scale, float* loss, float* dlogits,
                                  float* score, double* workspace, int N, int C, int HW, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && HW > 0, "oasis_ce: empty tensor N=%d HW=%d", N, HW);
    DCVIC_CHECK_ARG(C >= 2, "oasis_ce: C=%d, needs the fake class and at least one codebook entry (C >= 2)", C);
    DCVIC_CHECK_ARG(logits && loss && workspace, "oasis_ce: null pointer (logits %p, loss %p, workspace %p)", (const void*)logits, (void*)loss,
                    (void*)workspace);
    DCVIC_CHECK_ARG(target || !is_real, "oasis_ce: null target with is_real");
    return chan_ce_launch<true>(logits, target, is_real ? 1 : 0, 0.0, scale, loss, dlogits, score, workspace, N, C, HW, (hipStream_t)stream);
}

extern "C" int dcvic_focal_ce_f32(const float* logits, const int64_t* target, double gamma, double scale, float* loss, float* dlogits,
                                  double* workspace, int N, int C, int HW, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && C > 0 && HW > 0, "focal_ce: empty tensor N=%d C=%d HW=%d", N, C, HW);
    DCVIC_CHECK_ARG(C >= 2, "focal_ce: C=%d, a cross entropy needs at least two classes (C >= 2)", C);
    DCVIC_CHECK_ARG(gamma == 0.0 || gamma >= 1.0,
                    "focal_ce: gamma=%g, needs 0 (plain cross entropy) or >= 1 (the derivative is unbounded at p_t = 1 for 0 < gamma < 1)", gamma);
    DCVIC_CHECK_ARG(logits && target && loss && workspace, "focal_ce: null pointer (logits %p, target %p, loss %p, workspace %p)",
                    (const void*)logits, (const void*)target, (void*)loss, (void*)workspace);
    return chan_ce_launch<false>(logits, target, 0, gamma, scale, loss, dlogits, nullptr, workspace, N, C, HW, (hipStream_t)stream);
}
