/* dcvic_loss.h -- training-loss entry points of libdcvic_hip.so that came after dcvic.h's table was frozen.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, fp32 NCHW with dense channel
 * planes, every launch on the hipStream_t passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local
 * message in dcvic_last_error(), and bitwise-reproducible results (fp64 sums in a fixed order, no atomics).
 */
#ifndef DCVIC_LOSS_H
#define DCVIC_LOSS_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Focal cross entropy over the channel axis (src/losses/cross_entropy_loss.py:33-53 `FocalCrossEntropyLoss.forward`;
 * csrc/chan_ce.hip) on logits [N][C][HW] (fp32, dense) and int64 classes [N][HW].  Per position
 *   ce = logsumexp_c(z) - z[t],  p_t = exp(-ce),  q = 1 - p_t,  f = q^gamma * ce
 *   loss[0] = scale * sum_positions f      (the caller passes weight / (N*HW) for reduction "mean", weight for "sum")
 *   dlogits[j] = scale * (p_j - [j == t]) * (q^gamma + gamma * q^(gamma-1) * p_t * ce), or NULL for the value only
 * gamma is 0 (plain cross entropy) or >= 1: for 0 < gamma < 1 the derivative is unbounded at p_t = 1.  Needs C >= 2.  A class
 * outside [0, C) makes the loss NaN; it is never used as an address.  The value's bits do not depend on whether dlogits is given,
 * and no output depends on what loss, dlogits or workspace held before.
 * workspace: dcvic_focal_ce_workspace_doubles(N, HW) doubles (0 for an empty tensor). */
long long dcvic_focal_ce_workspace_doubles(int N, int HW);
int dcvic_focal_ce_f32(const float* logits, const int64_t* target, double gamma, double scale, float* loss, float* dlogits,
                       double* workspace, int N, int C, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif
