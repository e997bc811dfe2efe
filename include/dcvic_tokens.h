/* dcvic_tokens.h -- the ingest of a stored selection set (csrc/tokens.hip): uint8 crops to the model's fp32 NCHW input, and stored VQ
 * tokens to the encoder's index, latent and feature tensors.  Declared outside dcvic.h's and the other late headers' tables, which
 * are frozen.
 *
 * Same library, same conventions as dcvic.h: plain C types, DEVICE pointers into caller-owned memory, the launch on the hipStream_t
 * passed in (as void*), 0 on success or a negative DCVIC_E* code with a thread-local message in dcvic_last_error().
 *
 * Contract of both entry points, that of the other entry points: arguments are checked before any launch; every output element is
 * written exactly once and nothing depends on what an output held; image n's output depends on image n's input alone, not on N; no
 * atomics, so two runs give equal bits; no allocation, no synchronisation, one launch, no workspace: the call can be captured into
 * a graph. */
#ifndef DCVIC_TOKENS_H
#define DCVIC_TOKENS_H

#include "dcvic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src: uint8 [N][H][W][3], dense, at ANY byte address (a slice of a larger resident array: item n starts n * H * W * 3 bytes after
 * src, which is not aligned for odd sizes).  out: fp32 [N][3][H][W], dense, out[n][c][y][x] = table[src[n][y][x][c]].  table: 256
 * fp32 on the device, the caller's uint8 -> model-range map.
 *
 * Four pixels are loaded as three 32-bit words where their 12 bytes start on a 4-byte address and lie inside the item, byte by byte
 * otherwise; no byte outside [src, src + N * H * W * 3) is read.  Refused before any launch, with "u8_hwc_to_f32_nchw:" in front:
 * null pointers; N, H or W < 1; N > 65535; H * W > 2^28; an output that is not 4-byte aligned. */
int dcvic_u8_hwc_to_f32_nchw(const unsigned char* src, int N, int H, int W, const float* table, float* out, void* stream);

/* tokens: [N][h][w] of token_bytes = 1 (uint8) or 8 (int64) bytes each.  codebook: fp32 [n_e][D].  With t the token at (n, y, x)
 * and ok = 0 <= t < n_e, each output that is not null receives
 *   idx  int64 [N][h][w]           t, whatever its value
 *   zq   fp32  [N][D][h][w]        codebook[t][d] if ok, else NaN            (the bits of embedding(idx).permute(0, 3, 1, 2))
 *   feat fp32  [N][D + n_e][h][w]  channels [0, D) as zq; channel D + j is 1.0 if ok and j == t, else 0.0
 *                                                                            (the bits of cat[zq, one_hot(idx)])
 * A token outside [0, n_e) is never used as an address (the rule dcvic_focal_ce_f32 uses for targets).  Lanes run along h * w, so
 * every channel plane is written coalesced.  Refused before any launch, with "vq_token_feat:" in front: null tokens or codebook;
 * all three outputs null; N, h, w, D or n_e < 1; N > 65535; h * w > 2^28; D + n_e > 2^19; token_bytes other than 1 or 8; int64
 * tokens or idx not 8-byte aligned; codebook, zq or feat not 4-byte aligned. */
int dcvic_vq_token_feat_f32(const void* tokens, int token_bytes, const float* codebook, int N, int h, int w, int D, int n_e,
                            long long* idx, float* zq, float* feat, void* stream);

#ifdef __cplusplus
}
#endif
#endif
