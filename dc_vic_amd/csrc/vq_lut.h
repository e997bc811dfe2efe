// vq_lut.h -- the latent of one codebook entry behind the 1x1 post_quant_conv, shared by argmax_lut_kernel (csrc/vq.hip) and
// gumbel_lut_kernel (csrc/gumbel.hip): one fmaf chain, so equal indices give equal bits in both.
#pragma once
#include "common.h"

// latent[c] = pq_b[c] + sum_d pq_w[c][d] * cb[bi][d]   (pq_b may be null)
__device__ __forceinline__ float dcvic_lut_latent(const float* __restrict__ cb, const float* __restrict__ pq_w, const float* __restrict__ pq_b,
                                                   int bi, int c, int D) {
    float a = 0.f;
    for (int d = 0; d < D; ++d) a = fmaf(pq_w[c * D + d], cb[bi * D + d], a);
    if (pq_b) a += pq_b[c];
    return a;
}
