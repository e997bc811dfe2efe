/* dcvic_vq.h -- which search kernel dcvic_vq_argmin_f32 launched (csrc/vq.hip).  Declared outside dcvic.h's, dcvic_loss.h's,
 * dcvic_rate.h's and dcvic_train.h's tables, which are frozen.
 *
 * Same library, same conventions as dcvic.h.  Debug / test aid, state PER CALLING THREAD, like dcvic_conv_last_variant.
 */
#ifndef DCVIC_VQ_H
#define DCVIC_VQ_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCVIC_VQ_NONE    0   /* no call on this thread yet, or the last call was refused before a launch */
#define DCVIC_VQ_SHARD   1   /* vq_shard_mfma_kernel: 256-code shards, fp32 MFMA dots (D = 4, n_e % 256 == 0, 16-byte codebook) */
#define DCVIC_VQ_PACKED2 2   /* vq_argmin4_kernel<2>: 4 vectors per lane (D = 4, n_e % 8 == 0, n_e <= 1024, N * cdiv(HW, 1024) >= 2048) */
#define DCVIC_VQ_PACKED1 3   /* vq_argmin4_kernel<1>: 2 vectors per lane (the same codebooks, smaller launches) */
#define DCVIC_VQ_LDS4    4   /* vq_argmin_kernel<4>: the codebook as one LDS image */
#define DCVIC_VQ_LDS8    5   /* vq_argmin_kernel<8> */

/* The kernel the calling thread's last dcvic_vq_argmin_f32 launched, one of the DCVIC_VQ_* codes above. */
int dcvic_vq_last_variant(void);

#ifdef __cplusplus
}
#endif
#endif
