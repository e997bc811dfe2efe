/* dcvic_train.h -- training-step entry points of libdcvic_hip.so that came after dcvic.h's table was frozen (csrc/train.hip).
 * Declared outside dcvic.h's, dcvic_loss.h's and dcvic_rate.h's tables.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, fp32 NCHW with dense channel
 * planes, every launch on the hipStream_t passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local
 * message in dcvic_last_error(), and bitwise-reproducible results (fixed-order reductions, no atomics).  Every argument check
 * happens before the first launch and its message starts with the entry point's name.
 */
#ifndef DCVIC_TRAIN_H
#define DCVIC_TRAIN_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weight gradient of ONE source of a convolution whose input is a list of channel-slice views (dcvic_conv_io.src): X is
 * [N][Cs][Hx][Wx] with its own batch stride x_bs, and the result goes to channels [c_off, c_off + Cs) of dW [M][Cx_total][KH][KW]
 *   dW[m][c_off + c][ky][kx] (+)= sum_{n,oy,ox} G[n][m][oy][ox] * X[n][c][oy*s+ky-pt][ox*s+kx-pl]
 * (written, or added with accumulate != 0; the other channels of dW are not touched).  Same kernel, fp32 MFMA partials and
 * ascending-slab reduction as dcvic_conv_wgrad_f32; the pixel slabs are those of the whole layer (Cx_total), so one call per
 * source gives, bit for bit, what dcvic_conv_wgrad_f32 gives on the concatenated input -- no concatenation needed.
 * Rejected: a null pointer; Cs <= 0, c_off < 0 or c_off + Cs > Cx_total; a batch stride below its map; what dcvic_conv_wgrad_f32
 * rejects.  workspace: dcvic_conv_wgrad_workspace_floats(N, M, Cx_total, KH, KW, Hg, NULL) floats. */
int dcvic_conv_wgrad_src_f32(const float* G, long long g_bs, int M, int Hg, int Wg, const float* X, long long x_bs, int Cs,
                             int Hx, int Wx, int N, int KH, int KW, int stride, int pt, int pl, float* dW, int Cx_total,
                             int c_off, int accumulate, float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
