/* dcvic_sample_loss.h -- the two code losses of the rate-distortion trainers with one weight per image (csrc/sample_loss.hip).
 * Declared outside dcvic.h's, dcvic_loss.h's, dcvic_rate.h's, dcvic_train.h's and dcvic_vq.h's tables, which are frozen.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, fp32 data, every launch on the
 * hipStream_t passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local message in dcvic_last_error(), and
 * bitwise-reproducible results (fp64 sums in a fixed order, no atomics).
 *
 * Under trainer.sample_beta_batch the reference weights a loss map per image (apply_loss_weight,
 * src/trainer/dual_cond_rate_distortion_vq_code_trainer.py:71-98,189-198): the mean over every axis but the batch, then
 * (loss * weight).mean().  For every `reduction` that is sum_n w[n] * S[n] with S[n] image n's own sum of per-element terms and w a
 * vector the host forms (train/losses.py sample_loss_weights).  Both entry points compute exactly that:
 *   loss[0]       = sum_n w[n] * S[n]           (fp64, images in ascending order within four interleaved groups, then the groups)
 *   per_sample[n] = S[n], unweighted            (optional: NULL skips it)
 *   the gradient of loss[0] w.r.t. the first operand (optional: NULL gives the value only)
 * S[n], per_sample[n] and image n's plane of the gradient depend on image n's data and w[n] alone, not on N or on the other images.
 * The value's bits do not depend on whether the gradient is asked for, and no output depends on what loss, per_sample, the gradient
 * or the workspace held before.  w is required: NULL is an error, not a vector of ones. */
#ifndef DCVIC_SAMPLE_LOSS_H
#define DCVIC_SAMPLE_LOSS_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Focal cross entropy over the channel axis, per-image weights: logits [N][C][HW] (dense), int64 classes [N][HW], w [N].
 * Per position f = q^gamma * ce exactly as dcvic_focal_ce_f32 forms it (dcvic_loss.h; the same kernel core), S[n] = sum_p f(n, p),
 *   dlogits[n][j][p] = w[n] * (p_j - [j == t]) * (q^gamma + gamma * q^(gamma-1) * p_t * ce)
 * so with w[n] = s for every n the gradient has the bits of dcvic_focal_ce_f32 at scale s.  gamma is 0 or >= 1, C >= 2.  A class
 * outside [0, C) makes S[n] and the loss NaN; it is never used as an address.
 * workspace: dcvic_focal_ce_sample_workspace_doubles(N, HW) doubles (0 for an empty tensor). */
long long dcvic_focal_ce_sample_workspace_doubles(int N, int HW);
int dcvic_focal_ce_sample_f32(const float* logits, const int64_t* target, const float* w, double gamma, float* loss, float* dlogits,
                              float* per_sample, double* workspace, int N, int C, int HW, void* stream);

/* Squared error, per-image weights, value and gradient in one pass: a [N][M] with batch stride a_bs >= M (a channel-slice view), b and
 * da [N][M] dense, w [N].
 *   S[n] = sum_i (a[n][i] - b[n][i])^2,   da[n][i] = 2 * w[n] * (a[n][i] - b[n][i])
 * workspace: dcvic_sq_err_sample_workspace_doubles(N, M) doubles (0 for an empty tensor). */
long long dcvic_sq_err_sample_workspace_doubles(int N, long long M);
int dcvic_sq_err_sample_f32(const float* a, long long a_bs, const float* b, const float* w, float* loss, float* da, float* per_sample,
                            double* workspace, int N, long long M, void* stream);

#ifdef __cplusplus
}
#endif
#endif
