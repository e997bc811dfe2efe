/* dcvic_msssim_loss.h -- the image distortions MSSSIMLoss and L1Loss of the rate-distortion trainer, value and gradient
 * (csrc/msssim_loss.hip).  Declared outside dcvic.h's, dcvic_loss.h's, dcvic_rate.h's, dcvic_train.h's, dcvic_vq.h's,
 * dcvic_sample_loss.h's and dcvic_gumbel.h's tables, which are frozen.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, fp32 data, every launch on the
 * hipStream_t passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local message in dcvic_last_error().
 * Sums are fp64 in a fixed order that depends on the plane's (image's) size only, no atomics: two runs give equal bits, and with the same
 * `scale` image n's values and gradient have the same bits in any batch.  No result depends on what an output or the workspace held.
 * No allocation and no synchronisation inside: a call can sit in a captured region.  Every refusal comes before any launch. */
#ifndef DCVIC_MSSSIM_LOSS_H
#define DCVIC_MSSSIM_LOSS_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MS-SSIM of pytorch-msssim 0.2.1 with data_range = 1 (C1 = 0.01^2, C2 = 0.03^2) on float planes taken as they are -- the reference's
 * MSSSIMLoss applies it to the trainer's [-1, 1] images, `fake` unclamped; restated, parity with the package unpinned.
 * real, fake: contiguous [N][C][H][W], min(H, W) > 160.  Per plane V = prod_{s<4} relu(mean cs_s)^w_s * relu(mean ssim_4)^w_4 over
 * five scales (11-tap Gaussian, sigma 1.5, valid; avg_pool2d(2, padding = size % 2) in between).
 *   loss[0]      = scale * sum over the N*C planes of (1 - V)            (fp64; written, not accumulated)
 *   per_plane[p] = V                                                     (fp64 [N*C]; optional, NULL skips it)
 *   dfake        = d loss[0] / d fake                                    (fp32, shape of fake; optional: NULL gives the forward only;
 *                                                                         written, not accumulated; `real` is a constant)
 * A plane with a factor <= 0 has V = 0 and an all-zero gradient.  loss[0]'s bits do not depend on whether dfake is asked for.
 * workspace: dcvic_msssim_loss_workspace_bytes(N, C, H, W) bytes, 256-byte aligned (0 for sizes the entry point refuses). */
long long dcvic_msssim_loss_workspace_bytes(int N, int C, int H, int W);
int dcvic_msssim_loss_f32(const float* real, const float* fake, int N, int C, int H, int W, double scale, double* loss, double* per_plane,
                          float* dfake, void* workspace, long long workspace_bytes, void* stream);

/* Absolute error: a, b contiguous [N][n_per_image].
 *   loss[0] = scale * sum |a - b|                                        (fp64; written)
 *   da      = scale * sign(a - b), sign(0) = 0                           (fp32, shape of a; optional)
 * workspace: dcvic_abs_err_workspace_bytes(N, n_per_image) bytes (0 for an empty tensor). */
long long dcvic_abs_err_workspace_bytes(int N, long long n_per_image);
int dcvic_abs_err_f32(const float* a, const float* b, long long n_per_image, int N, double scale, double* loss, float* da, void* workspace,
                      long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
