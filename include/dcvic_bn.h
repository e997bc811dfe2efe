/* dcvic_bn.h -- per-channel batch statistics over (N, H, W) and their backward: torch.nn.BatchNorm2d in training mode and taming's
 * ActNorm, for the normalised GAN discriminators (csrc/bn_train.hip).  Declared outside the tables of dcvic.h and the other eight
 * headers, which are frozen.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, fp32 data, every launch on the
 * hipStream_t passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local message in dcvic_last_error().
 *
 * Tensors are [N][C][HW], dense within an image, each with its own batch stride (>= C * HW: a channel-slice view is welcome).
 * M = N * HW is the number of values per channel.  Sums are fp64, in an order that depends on (N, C, HW) alone: no atomics, the
 * same inputs give the same bits on every run and for every batch stride.  No output depends on what it, or the workspace, held
 * before (dgamma / dbeta / dloc / dscale are added to only when `accumulate` is set).  No allocation and no synchronisation inside.
 *
 * The variance is E[x^2] - mean^2 of the fp64 sums: its relative error is about 1e-16 * (1 + mean^2 / var), i.e. exact to fp32 up to a
 * channel mean of about 1e4 standard deviations and without digits past about 1e8 (tested up to 1e3).
 *
 * `act` is DCVIC_ACT_NONE or DCVIC_ACT_LRELU02 (LeakyReLU(0.2) applied to the normalised value; in the backward its derivative is
 * taken from the sign of the output y: 1 where y > 0, else 0.2).
 *
 * Refused before any launch, with the entry point's name in front: M < 2, N > 65535, a null required pointer, an empty size, a batch
 * stride below C * HW, eps that is not finite and positive, momentum outside [0, 1], another `act`, a workspace that is misaligned
 * (8 bytes) or below dcvic_bn_workspace_bytes(N, C, HW). */
#ifndef DCVIC_BN_H
#define DCVIC_BN_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace every entry point below needs for [N][C][HW] (0 for an empty tensor). */
long long dcvic_bn_workspace_bytes(int N, int C, int HW);

/* Statistics only: mean[c] and the UNBIASED standard deviation std[c] = sqrt(max(var, 0) * M / (M - 1)) (ActNorm's initialisation). */
int dcvic_bn_stats_f32(const float* x, long long x_bs, float* mean, float* std_unbiased, void* workspace, long long workspace_bytes,
                       int N, int C, int HW, void* stream);

/* BatchNorm2d, training mode.  mean[c] and the biased variance var[c] over the batch, rstd = 1 / sqrt(max(var, 0) + eps),
 *   y = act((x - mean) * rstd * gamma[c] + beta[c])            (a constant channel gives act(beta[c]) exactly)
 *   save_mean[c] = mean, save_rstd[c] = rstd                   (required: the backward reads them)
 *   running_mean = (1 - momentum) * running_mean + momentum * mean
 *   running_var  = (1 - momentum) * running_var  + momentum * var * M / (M - 1)      (both NULL: no update)
 * y may be x (in place). */
int dcvic_bn_train_fwd_f32(const float* x, long long x_bs, float* y, long long y_bs, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, double momentum, double eps, float* save_mean, float* save_rstd,
                           int act, void* workspace, long long workspace_bytes, int N, int C, int HW, void* stream);

/* Its backward for a gradient g on y.  With xhat = (x - save_mean) * save_rstd and g' = g * act'(y) (y is read only with an act):
 *   dbeta[c] = sum g',  dgamma[c] = sum g' * xhat,  dx = gamma * rstd * (g' - dbeta / M - xhat * dgamma / M)
 * dgamma / dbeta (both or neither; NULL: not wanted) are overwritten, or added to with `accumulate`; dx is written. */
int dcvic_bn_train_bwd_f32(const float* x, long long x_bs, const float* g, long long g_bs, const float* y, long long y_bs,
                           const float* save_mean, const float* save_rstd, const float* gamma, float* dx, long long dx_bs,
                           float* dgamma, float* dbeta, int accumulate, int act, void* workspace, long long workspace_bytes,
                           int N, int C, int HW, void* stream);

/* ActNorm: y = act(scale[c] * (x + loc[c])).  Every value depends on its own image alone. */
int dcvic_actnorm_fwd_f32(const float* x, long long x_bs, float* y, long long y_bs, const float* loc, const float* scale, int act,
                          int N, int C, int HW, void* stream);

/* Its backward: dscale[c] = sum g' * (x + loc), dloc[c] = scale * sum g', dx = scale * g'  (g', dloc / dscale as above). */
int dcvic_actnorm_bwd_f32(const float* x, long long x_bs, const float* g, long long g_bs, const float* y, long long y_bs,
                          const float* loc, const float* scale, float* dx, long long dx_bs, float* dloc, float* dscale,
                          int accumulate, int act, void* workspace, long long workspace_bytes, int N, int C, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif
