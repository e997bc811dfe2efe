/* dcvic_rate.h -- the differentiable rate term of libdcvic_hip.so: the training-mode (additive-noise) forward of the two entropy
 * models, the gradients of the rate loss they feed, and the entropy bottleneck's auxiliary quantile loss (csrc/rate_train.hip).
 * Declared outside dcvic.h's and dcvic_loss.h's frozen tables.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, fp32 NCHW with dense channel
 * planes, every launch on the hipStream_t passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local
 * message in dcvic_last_error(), and bitwise-reproducible results (fp64 sums in a fixed order, no atomics).  Every argument check
 * happens before the first launch and its message starts with the entry point's name.
 *
 * Common to both rate entry points:
 *   - sample_weight is [N] (device) or NULL for 1; scale is a host scalar; together they state the trainer's reduction:
 *       loss[0] += sum_n scale * w[n] * b[n],   b[n] = -(sum over image n of ln p) / ln 2 of THIS call, summed in fp64, n ascending
 *       bits[n] += b[n]
 *     Both ACCUMULATE (the caller zeroes them; the CHARM slices and the hyper-latent add up).  Every other output is overwritten
 *     and no result depends on what an output or the workspace held before.
 *   - The gradients are those of this call's loss term.  With g_p = -scale * w[n] / (p ln 2), both lower bounds use CompressAI's
 *     LowerBound backward literally: a gradient passes a bound max(x, bound) when x >= bound or when the incoming gradient is
 *     negative.  For the likelihood bound 1e-9: g_p passes to p_raw when p_raw >= 1e-9 or g_p < 0.
 *   - b[n] and the data gradients of image n do not depend on the batch the image is in; the bits of bits / loss / lik do not
 *     depend on which gradient outputs are requested.
 *   - bits or loss need N <= 1024 and the workspace.
 */
#ifndef DCVIC_RATE_H
#define DCVIC_RATE_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The entropy bottleneck's RAW parameters (CompressAI 1.2.4 names, filters (3,3,3,3)), one device pointer per tensor, each dense:
 *   matrix[0] [C][3][1], matrix[1..3] [C][3][3], matrix[4] [C][1][3];  bias[0..3] [C][3][1], bias[4] [C][1][1];  factor[0..3] [C][3][1].
 * The kernels apply softplus to the matrices and tanh to the factors themselves.  The structs live in HOST memory. */
typedef struct {
    const float* matrix[5];
    const float* bias[5];
    const float* factor[4];
} dcvic_eb_params;

/* The gradients w.r.t. those raw values, same shapes; all 14 pointers must be set. */
typedef struct {
    float* matrix[5];
    float* bias[5];
    float* factor[4];
} dcvic_eb_grads;

/* GaussianConditional.forward(training=True) of CompressAI 1.2.4 as driven by ste_gaussian_conditional.py:16-23 with
 * scale_bound 0.11 and likelihood bound 1e-9 (csrc/rate_train.hip).  y, noise, mu, sigma: [N][C][HW] views with batch strides
 * y_bs, noise_bs and ms_bs (mu and sigma share theirs); noise holds values in [-0.5, 0.5].  Per element
 *   yt = y + noise,  v = |yt - mu|,  s = max(sigma, 0.11),  a = (0.5 - v) / s,  b = (-0.5 - v) / s
 *   p_raw = Phi(a) - Phi(b),  Phi(x) = 0.5 erfc(-x / sqrt 2),  p = max(p_raw, 1e-9)
 * Outputs, each may be NULL:
 *   y_hat (batch stride yh_bs) = rint(y - mu) + mu     the STE output, the bits of dcvic_gaussian_rate_f32's y_hat
 *   lik   (batch stride lik_bs) = p
 *   bits [N], loss [1]                                  as stated above
 *   dy    (batch stride dy_bs: six 32-channel slices fill one 192-channel tensor) = g_raw * dp_raw/dyt
 *   dmu, dsigma (batch stride dms_bs; dmu = -dy)
 * with phi the standard normal density and sign(0) = 0:
 *   dp_raw/dyt = -sign(yt - mu) * (phi(a) - phi(b)) / s,   dp_raw/ds = -(a phi(a) - b phi(b)) / s
 *   dsigma = the gradient w.r.t. s when sigma >= 0.11 or that gradient is negative, else 0.
 * Rejected: a null y, mu, sigma or noise; N, C or HW <= 0; a batch stride below C*HW; no output at all; bits or loss with
 * N > 1024 or without workspace.  workspace: N * dcvic_rate_blocks(C*HW) doubles (needed for bits or loss only).
 * The float4 or scalar form is chosen from C*HW, the strides and the alignment only, never from N. */
int dcvic_gaussian_rate_train_f32(const float* y, long long y_bs, const float* mu, const float* sigma, long long ms_bs,
                                  const float* noise, long long noise_bs, const float* sample_weight, double scale,
                                  float* y_hat, long long yh_bs, float* lik, long long lik_bs, float* bits, float* loss,
                                  float* dy, long long dy_bs, float* dmu, float* dsigma, long long dms_bs,
                                  double* workspace, int N, int C, int HW, void* stream);

/* EntropyBottleneck.forward(training=True) of CompressAI 1.2.4, filters (3,3,3,3) (csrc/rate_train.hip).  z, noise: dense
 * [N][C][HW]; medians[c * med_stride] (quantiles + 1 with stride 3, or a dense vector with stride 1).  Per element, with
 * logits_c the channel's cumulative (matrix_k <- softplus, factor_k <- tanh; h <- M_k h + b_k; h <- h + f_k * tanh(h) for k < 4):
 *   zt = z + noise,  lower = logits_c(zt - 0.5),  upper = logits_c(zt + 0.5),  sg = -sign(lower + upper)  (a constant)
 *   p_raw = |sigmoid(sg * upper) - sigmoid(sg * lower)|,  p = max(p_raw, 1e-9)
 * Outputs, each may be NULL (dense [N][C][HW] unless stated):
 *   z_hat = rint(z - med) + med        the bits of dcvic_eb_rate_f32's z_hat
 *   lik = p;  bits [N], loss [1]       as stated above; bits[n] adds the channels in ascending order
 *   dz                                 the gradient of the loss term w.r.t. z
 *   grads                              the gradient w.r.t. the 58 raw values of every channel, through softplus and tanh, summed
 *                                      over N*HW in fp64 in a fixed order and ACCUMULATED (+=) into the caller's buffers
 * Rejected: a null z, noise, params (or one of its 14 pointers) or medians; N, C or HW <= 0; med_stride <= 0; grads with a null
 * pointer in it; no output at all; bits or loss with N > 1024 or without workspace.
 * workspace: dcvic_eb_rate_train_workspace_doubles(N, C, HW) doubles (needed for bits or loss only; 0 for an empty tensor). */
long long dcvic_eb_rate_train_workspace_doubles(int N, int C, int HW);
int dcvic_eb_rate_train_f32(const float* z, const float* noise, const dcvic_eb_params* params, const float* medians, int med_stride,
                            const float* sample_weight, double scale, float* z_hat, float* lik, float* bits, float* loss,
                            float* dz, const dcvic_eb_grads* grads, double* workspace, int N, int C, int HW, void* stream);

/* EntropyBottleneck.loss() of CompressAI 1.2.4: with quantiles [C][3] (dense) and target [3] = (-t, 0, t), t = ln(2 / tail_mass - 1),
 *   aux[0] = sum_c sum_k |logits_c(quantiles[c][k]) - target[k]|          (fp64 sum in a fixed order; overwritten)
 *   dquantiles[c][k] = sign(logits_c(q) - target[k]) * dlogits_c/dx (q)    (overwritten, or += with accumulate != 0)
 * The parameters are stop-gradient there, so quantiles is the only gradient.  aux or dquantiles may be NULL, not both.
 * Rejected: a null params (or one of its pointers), quantiles or target; C <= 0; neither output. */
int dcvic_eb_aux_loss_f32(const dcvic_eb_params* params, const float* quantiles, const float* target, float* aux, float* dquantiles,
                          int accumulate, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
