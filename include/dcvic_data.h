/* dcvic_data.h -- the device half of the training data feed (csrc/data.hip): Pillow's 8-bit resampling of a crop's source window,
 * the horizontal flip, the [-1, 1] conversion and the NCHW layout, for a whole batch in one launch.  Declared outside dcvic.h's,
 * dcvic_loss.h's, dcvic_rate.h's, dcvic_train.h's, dcvic_vq.h's, dcvic_sample_loss.h's, dcvic_gumbel.h's and dcvic_msssim_loss.h's
 * tables, which are frozen.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, the launch on the hipStream_t
 * passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local message in dcvic_last_error().
 *
 * The reference's transform (data_transform.py:19-73) is PIL.Image.resize of the whole image, RandomCrop, RandomHorizontalFlip,
 * ToTensor, Normalize(.5, .5).  Pillow's resize of 8-bit images (Resample.c) is two integer passes, horizontal then vertical,
 *   u8 = clip8((2^21 + sum_k pixel[xmin + k] * coeff[k]) >> 22)       int32, arithmetic shift, the clip applied to the shifted value
 * with per output index a first source index xmin, a tap count and `count` coefficients of 22 fraction bits; a pass whose axis keeps
 * its size is skipped.  The caller restates the tables on the host (dc_vic_amd/train/data.py pil_coeffs) for the S output rows and
 * columns of one crop only and ships the source rectangle those read, so the kernel resamples that window and nothing else. */
#ifndef DCVIC_DATA_H
#define DCVIC_DATA_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVIC_DATA_MAX_KSIZE 17   /* taps per output and axis: bicubic (support 2) down to a scale of 1/4 */
#define DCVIC_DATA_MAX_S 32768

/* One image of the batch.  Every offset is in bytes from the slab's first byte.  The window is src_h rows of src_w RGB-interleaved
 * uint8 pixels, row r at src_off + r * src_stride.  Per axis, k = 0 means "copy" (the resize leaves the axis unchanged: the window's
 * extent on that axis must be S), else the axis's tables start at tab_*: int32 coefficients [S][k], then int32 xmin [S], then int32
 * count [S], xmin relative to the window, xmin + count within it, count <= k. */
typedef struct dcvic_crop_desc {
    long long src_off;
    long long tab_x;
    long long tab_y;
    int src_h;
    int src_w;
    int src_stride;
    int flip;
    int kx;
    int ky;
} dcvic_crop_desc;

/* out [N][3][S][S] fp32, dense: out[n][c][y][x] = table[v[y][flip ? S - 1 - x : x][c]] with v the window after the horizontal pass
 * (if kx) and the vertical pass (if ky) on its uint8 result.  table: 256 fp32 on the device, the caller's uint8 -> model-range map.
 * desc_dev: N descriptors on the device (they may lie in the slab); desc_host: the same N descriptors in host memory, on which every
 * check below is made.
 *
 * Contract, that of the other entry points: every output element is written exactly once and nothing depends on what the output
 * held; image n's output depends on descriptor n and what it points to alone, not on N; two runs give equal bits (integer sums in
 * a fixed order); no allocation, no synchronisation, one launch, no workspace.  Table entries read from the slab are clamped to the
 * window on load (xmin to [0, extent], count to [0, min(k, extent - xmin)]), so no table content makes the kernel read outside the
 * window.  Refused before any launch, with "u8_resample_crop:" in front: null pointers; N < 1 or S < 1; N > 65535; S >
 * DCVIC_DATA_MAX_S; a slab that is not 4-byte aligned or descriptors that are not 8-byte aligned; kx or ky outside [0, DCVIC_DATA_MAX_KSIZE]; a window with src_h or src_w < 1,
 * src_stride < 3 * src_w or any byte outside [0, slab_bytes); a "copy" axis whose extent is not S; a table that is not 4-byte aligned
 * or reaches outside the slab. */
int dcvic_u8_resample_crop_f32(const unsigned char* slab, long long slab_bytes, const dcvic_crop_desc* desc_dev,
                               const dcvic_crop_desc* desc_host, int N, int S, const float* table, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
