/* dcvic_gumbel.h -- the hard Gumbel-softmax sample of the VQ indices in training mode and its straight-through gradient
 * (csrc/gumbel.hip).  Declared outside dcvic.h's, dcvic_loss.h's, dcvic_rate.h's, dcvic_train.h's, dcvic_vq.h's and
 * dcvic_sample_loss.h's tables, which are frozen.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, fp32 data, every launch on the
 * hipStream_t passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local message in dcvic_last_error().
 *
 * The reference (hyperprior_dc_vic_model.py:254-260) decodes, in training mode with model.gumbel_sampling,
 *   ret    = F.gumbel_softmax(logits, dim=1, hard=True, tau=tau)     = one_hot(idx) - s.detach() + s
 *   latent = post_quant_conv(ret @ codebook.detach())
 * with z = logits + g, g = -log(e), e ~ Exp(1), s = softmax(z / tau) over the class axis, idx = argmax s.  Both entry points take the
 * draw e as an input tensor (the caller owns the generator), so they are functions of their arguments.
 *
 * Tensors, all dense: logits, noise, dlogits [N][C][HW]; idx int64 [N][HW]; latent, glatent [N][D][HW]; codebook [C][D];
 * pq_w [D][D] (the 1x1 post_quant_conv, [out][in]); pq_b [D] or NULL.
 *
 * Contract (that of dcvic_loss.h and dcvic_rate.h): no atomics, two runs give equal bits; image n's outputs depend on image n's
 * inputs alone, not on N; no output depends on what an output buffer held; every noise value is clamped on load to
 * [FLT_MIN, FLT_MAX], so no value of e (0, negative, Inf, NaN) yields a NaN; idx is in [0, C) by construction and is the only value
 * used as an address.  Limits, refused before any launch: tau finite and > 0, N <= 65535, D <= 8, C * D <= 8192 (the codebook is
 * staged in 32 KiB of LDS), C * HW < 2^31. */
#ifndef DCVIC_GUMBEL_H
#define DCVIC_GUMBEL_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward.  Per position: z_j = logits_j + (-logf(e_j)); idx = the lowest j with the largest z_j (the rule of dcvic_argmax_lut_f32:
 * tau > 0 does not move the argmax, so z is not divided); latent[c] = pq_b[c] + sum_d pq_w[c][d] * codebook[idx][d] by the fmaf
 * chain of dcvic_argmax_lut_f32 (one device function, csrc/vq_lut.h): for equal idx the latent has that entry point's bits.
 * The value of the straight-through one-hot, (1 - s_idx) + s_idx, is taken as exactly 1; in fp32 the reference's is 1 or 1 +- 1 ulp,
 * and 0 +- 1 ulp of s_j in the other classes.  idx may be NULL. */
int dcvic_gumbel_lut_f32(const float* logits, const float* noise, int64_t* idx, float* latent, const float* codebook, const float* pq_w,
                         const float* pq_b, double tau, int N, int C, int D, int HW, void* stream);

/* Backward: dlogits (written, not accumulated) for a gradient glatent on the latent.  Per position, with s = softmax(z / tau)
 * recomputed from logits and noise (nothing is kept from the forward call):
 *   h = pq_w^T glatent,  v_j = codebook[j] . h,  dlogits_j = s_j * (v_j - sum_k s_k v_k) / tau
 * the derivative of one_hot - s.detach() + s through the product with the frozen codebook and the frozen post_quant_conv.  v is
 * formed relative to the most likely class's, so a saturated softmax keeps the digits of its small gradients. */
int dcvic_gumbel_lut_bwd_f32(const float* logits, const float* noise, const float* glatent, const float* codebook, const float* pq_w,
                             double tau, float* dlogits, int N, int C, int D, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif
