// Conv2d(k3, s1, p1) -- optionally behind a nearest x2 upsample -- as an implicit GEMM on bf16 MFMA with fp32 accumulation (gfx950).
//
// Opt-in reconstruction precision for the layers after the path's last integer decision (the frozen VQGAN decoder and the SFT
// fusion blocks, layers.allow_bf16): weights are rounded to bf16 once at pack time (round to nearest even), activations stay fp32 in
// HBM and are rounded to bf16 (v_cvt_pk_bf16_f32, NaN stays NaN) while a tile is staged into LDS.  The fp32 kernels are untouched.
//
// GEMM view: out[co][pixel] = sum_{chunk, tap, channel} Wt[co][tap][ci] * IN[ci][pixel + tap offset].
// Workgroup: 128 output channels x a 4-row x 32-column pixel tile, 4 waves of 64 channels x 2 rows x 32 columns each.
// Per 32-channel input chunk the halo (6 x 34 positions, or 4 x 18 low-resolution positions with the x2 upsample) is staged in LDS as
// [position][32 channels] bf16 with an 80-byte position stride (conflict-free ds_read_b128: 16 lanes x 80 B cover 64 distinct banks).
// The next chunk's halo is loaded into registers while the current one is computed.  Weights are read from global memory (L2-resident,
// at most 4.7 MB per layer) straight in MFMA operand order, one tap ahead of the MFMAs that use them.
//
// Reduction order of every output element: input-channel chunks of 32 ascending, taps ascending, then the MFMA's own k order within a
// chunk -- a function of the layer only (no split-K, no atomics, fixed tile geometry), so a result never depends on N, on the batch an
// image is decoded in, or on the workgroup it lands in.
//
// MFMA shape: BF16_MFMA = 32 (v_mfma_f32_32x32x16_bf16, 2 x 2 tiles per wave, two k-steps per tap) or 16 (v_mfma_f32_16x16x32_bf16,
// 4 x 4 tiles per wave, one k-step per tap): same output tile per wave, same LDS image, packed weights in each shape's operand order.
// The shipped build is the one measured faster; the other is kept for A/B builds (-DBF16_MFMA=...).
#include <hip/hip_bf16.h>

#include "conv_common.h"

#ifndef BF16_MFMA
#define BF16_MFMA 32
#endif
static_assert(BF16_MFMA == 32 || BF16_MFMA == 16, "BF16_MFMA must be 32 or 16");

#define BF_CO 128      // output channels per workgroup
#define BF_TH 4        // output rows per workgroup
#define BF_TW 32       // output columns per workgroup
#define BF_KC 32       // input channels per LDS chunk
#define BF_PS 40       // LDS position stride in bf16 elements (32 channels + 8 pad = 80 bytes)

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Bf16Args {
    int Cin, Cout, N, H, W, Ho, Wo;       // H x W: input (low-resolution with the upsample), Ho x Wo: output
    const float* src[DCVIC_MAX_SRC];
    int srcC[DCVIC_MAX_SRC];
    long long src_bs[DCVIC_MAX_SRC];
    const unsigned short* wp;             // packed bf16 weights
    int n_chunks, tiles_x, tiles_y, co_tiles;
};

__device__ __forceinline__ unsigned int bf16_pack2(float a, float b) {
    // plain casts: hipcc emits v_cvt_pk_bf16_f32 (round to nearest even, a NaN stays a NaN)
    const __hip_bfloat16 lo = __float2bfloat16(a), hi = __float2bfloat16(b);
    return (unsigned int)__bfloat16_as_ushort(lo) | ((unsigned int)__bfloat16_as_ushort(hi) << 16);
}

template <bool UPS>
struct BfHalo {
    static constexpr int HR = UPS ? 4 : BF_TH + 2;           // staged rows
    static constexpr int HC = UPS ? BF_TW / 2 + 2 : BF_TW + 2;  // staged columns
    static constexpr int NP = HR * HC;
    static constexpr int NTASK = NP * (BF_KC / 2);           // (position, channel pair) tasks per chunk
    static constexpr int NIT = (NTASK + NTHREADS - 1) / NTHREADS;
};

// Loads one chunk's halo (fp32, zero outside the image and past Cin) into registers: v[i] = 2 channels of task tid + i * NTHREADS.
template <bool UPS>
__device__ __forceinline__ void bf_load_chunk(const Bf16Args& A, int n, int chunk, int hy0, int hx0, float (&v)[BfHalo<UPS>::NIT][2]) {
    using HL = BfHalo<UPS>;
    const long long plane = (long long)A.H * A.W;
#pragma unroll
    for (int i = 0; i < HL::NIT; ++i) {
        const int e = threadIdx.x + i * NTHREADS;
        v[i][0] = 0.f; v[i][1] = 0.f;
        if (e < HL::NTASK) {
            const int pos = e % HL::NP, cp = e / HL::NP;
            const int gy = hy0 + pos / HL::HC, gx = hx0 + pos % HL::HC;
            const int c = chunk * BF_KC + 2 * cp;
            if (c < A.Cin && gy >= 0 && gy < A.H && gx >= 0 && gx < A.W) {
                int s = 0, cb = 0;
                if (c >= A.srcC[0]) { s = 1; cb = A.srcC[0]; if (c >= cb + A.srcC[1]) { s = 2; cb += A.srcC[1]; } }
                const float* p = A.src[s] + (long long)n * A.src_bs[s] + (long long)(c - cb) * plane + (long long)gy * A.W + gx;
                v[i][0] = p[0];
                v[i][1] = p[plane];     // sources carry a multiple of 8 channels: c + 1 is in the same source
            }
        }
    }
}

template <bool UPS>
__device__ __forceinline__ void bf_store_chunk(unsigned short* lds, const float (&v)[BfHalo<UPS>::NIT][2]) {
    using HL = BfHalo<UPS>;
#pragma unroll
    for (int i = 0; i < HL::NIT; ++i) {
        const int e = threadIdx.x + i * NTHREADS;
        if (e < HL::NTASK) {
            const int pos = e % HL::NP, cp = e / HL::NP;
            *reinterpret_cast<unsigned int*>(lds + pos * BF_PS + 2 * cp) = bf16_pack2(v[i][0], v[i][1]);
        }
    }
}

// LDS position of output pixel (row r, column x) of the tile shifted by tap (dy, dx), all tile-relative
template <bool UPS>
__device__ __forceinline__ int bf_pos(int r, int x, int dy, int dx) {
    using HL = BfHalo<UPS>;
    // plain: halo origin (y0 - 1, x0 - 1); upsample: low-resolution origin (y0/2 - 1, x0/2 - 1) with y0 % 4 == 0, x0 % 32 == 0
    if constexpr (UPS) return (((r + dy + 2) >> 1)) * HL::HC + ((x + dx + 2) >> 1);
    else return (r + dy + 1) * HL::HC + (x + dx + 1);
}

template <bool UPS>
__global__ __launch_bounds__(NTHREADS) void conv3x3_bf16_kernel(Bf16Args A, ConvKArgs K) {
    using HL = BfHalo<UPS>;
    __shared__ __attribute__((aligned(16))) unsigned short lds[HL::NP * BF_PS];
    int b = blockIdx.x;
    const int cot = b % A.co_tiles; b /= A.co_tiles;
    const int tx = b % A.tiles_x; b /= A.tiles_x;
    const int ty = b % A.tiles_y;
    const int n = b / A.tiles_y;
    const int y0 = ty * BF_TH, x0 = tx * BF_TW;
    const int hy0 = UPS ? (y0 >> 1) - 1 : y0 - 1, hx0 = UPS ? (x0 >> 1) - 1 : x0 - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wco = wave & 1, wrow = (wave >> 1) * 2;      // wave: channels [64 wco, +64) of the tile, rows wrow, wrow + 1

#if BF16_MFMA == 32
    constexpr int MT = 2, NT = 2, NV = 16, KS = 2;        // m-tiles (32 channels), n-tiles (one 32-pixel row), accumulators, k-steps per tap
    const int cb0 = cot * 4 + wco * 2;                    // first 32-channel weight block of the wave
    const int lcol = lane & 31, kofs = 8 * (lane >> 5);
#else
    constexpr int MT = 4, NT = 4, NV = 4, KS = 1;         // 16-channel m-tiles; n-tile t = (row t >> 1, columns 16 (t & 1) ..)
    const int cb0 = cot * 8 + wco * 4;
    const int lcol = lane & 15, kofs = 8 * (lane >> 4);
#endif
    typedef float accv_t __attribute__((ext_vector_type(NV)));
    accv_t acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < NV; ++i) acc[m][t][i] = 0.f;

    // weights: [block][chunk][tap][k-step][lane][8]; one 1 KiB fragment per (block, chunk, tap, k-step)
    const bf16x8* wfr = reinterpret_cast<const bf16x8*>(A.wp);
    const long long blk_stride = (long long)A.n_chunks * 9 * KS * 64;

    float v[HL::NIT][2];
    bf_load_chunk<UPS>(A, n, 0, hy0, hx0, v);
    for (int ch = 0; ch < A.n_chunks; ++ch) {
        if (ch) __syncthreads();                          // every wave is done reading the previous chunk
        bf_store_chunk<UPS>(lds, v);
        __syncthreads();
        if (ch + 1 < A.n_chunks) bf_load_chunk<UPS>(A, n, ch + 1, hy0, hx0, v);
        const bf16x8* wc = wfr + (long long)cb0 * blk_stride + (long long)ch * 9 * KS * 64 + lane;
        bf16x8 a[2][MT][KS];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int k = 0; k < KS; ++k) a[0][m][k] = wc[m * blk_stride + k * 64];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int cur = tap & 1;
            if (tap + 1 < 9) {
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int k = 0; k < KS; ++k) a[cur ^ 1][m][k] = wc[m * blk_stride + ((tap + 1) * KS + k) * 64];
            }
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                bf16x8 bfr[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#if BF16_MFMA == 32
                    const int p = bf_pos<UPS>(wrow + t, lcol, dy, dx);
#else
                    const int p = bf_pos<UPS>(wrow + (t >> 1), (t & 1) * 16 + lcol, dy, dx);
#endif
                    bfr[t] = *reinterpret_cast<const bf16x8*>(lds + p * BF_PS + k * 16 + kofs);
                }
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
#if BF16_MFMA == 32
                        acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][m][k], bfr[t], acc[m][t], 0, 0, 0);
#else
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[cur][m][k], bfr[t], acc[m][t], 0, 0, 0);
#endif
                    }
            }
        }
    }

    // epilogue: lane holds NV output channels of one pixel per (m, t); bias -> act -> (+res) -> (affine) -> store
    const long long HWo = (long long)A.Ho * A.Wo;
    dcvic_epilogue_dispatch(K, [&](auto res_c, auto aff_c) {
        constexpr bool RES = decltype(res_c)::value, AFF = decltype(aff_c)::value;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#if BF16_MFMA == 32
            const int y = y0 + wrow + t, x = x0 + lcol;
#else
            const int y = y0 + wrow + (t >> 1), x = x0 + (t & 1) * 16 + lcol;
#endif
            if (y < A.Ho && x < A.Wo) {
#pragma unroll
                for (int m = 0; m < MT; ++m) {
#if BF16_MFMA == 32
                    const int cbase = (cb0 + m) * 32 + 4 * (lane >> 5);
                    auto co_of = [&](int r) { return cbase + (r & 3) + 8 * (r >> 2); };
                    dcvic_conv_epilogue<16, 8, RES, AFF>(K, n, acc[m][t], co_of, (long long)y * A.Wo + x, HWo);
#else
                    const int cbase = (cb0 + m) * 16 + 4 * (lane >> 4);
                    auto co_of = [&](int r) { return cbase + r; };
                    dcvic_conv_epilogue<4, 4, RES, AFF>(K, n, acc[m][t], co_of, (long long)y * A.Wo + x, HWo);
#endif
                }
            }
        }
    });
}

// w[Cout][Cin][3][3] fp32 -> bf16 (round to nearest even) in the MFMA A-operand order of the build's shape, zero past Cout / Cin
__global__ void conv3x3_bf16_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ packed, int Cin, int Cout, int n_chunks,
                                         long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
#if BF16_MFMA == 32
    const int ks = (int)((e >> 9) & 1);
    const long long r = e >> 10;
    const int co = (int)(r / 9 / n_chunks) * 32 + (lane & 31);
    const int ci = (int)(r / 9 % n_chunks) * BF_KC + ks * 16 + 8 * (lane >> 5) + j;
#else
    const long long r = e >> 9;
    const int co = (int)(r / 9 / n_chunks) * 16 + (lane & 15);
    const int ci = (int)(r / 9 % n_chunks) * BF_KC + 8 * (lane >> 4) + j;
#endif
    const int tap = (int)(r % 9);
    const float x = (co < Cout && ci < Cin) ? w[((long long)co * Cin + ci) * 9 + tap] : 0.f;
    packed[e] = __bfloat16_as_ushort(__float2bfloat16(x));
}

extern "C" size_t dcvic_conv3x3_bf16_packed_bytes(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0) return 0;
    return (size_t)((Cout + BF_CO - 1) / BF_CO) * BF_CO * ((Cin + BF_KC - 1) / BF_KC) * BF_KC * 9 * sizeof(unsigned short);
}

extern "C" int dcvic_conv3x3_bf16_mfma_shape(void) { return BF16_MFMA; }

extern "C" int dcvic_conv3x3_bf16_pack_f32(const float* w, void* packed, int Cin, int Cout, void* stream) {
    DCVIC_CHECK_ARG(w && packed && Cin > 0 && Cout > 0, "conv3x3_bf16_pack: bad argument");
    const int n_chunks = (Cin + BF_KC - 1) / BF_KC;
    const long long total = (long long)(dcvic_conv3x3_bf16_packed_bytes(Cin, Cout) / sizeof(unsigned short));
    conv3x3_bf16_pack_kernel<<<dcvic_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(w, (unsigned short*)packed, Cin, Cout, n_chunks, total);
    DCVIC_CHECK_LAUNCH("conv3x3_bf16_pack");
    return DCVIC_OK;
}

extern "C" int dcvic_conv3x3_bf16_f32(int Cin, int Cout, int upsample, const void* packed, const dcvic_conv_io* io, void* stream) {
    const DcvicConvRules rules = {"conv3x3_bf16", Cin, Cout, DCVIC_MAX_SRC, 8, false, upsample ? DCVIC_OUT_X2 : DCVIC_OUT_SAME, true, false, 0};
    ConvKArgs K;   // the epilogue's view of the launch (conv_common.h)
    if (const int rc = dcvic_conv_check_io(rules, packed, io, &K)) return rc;
    if (const int rc = dcvic_conv_tiles("conv3x3_bf16", &K, BF_KC, BF_CO, BF_TH, BF_TW)) return rc;
    Bf16Args A;
    memset(&A, 0, sizeof(A));
    A.Cin = Cin; A.Cout = Cout; A.N = K.N; A.H = K.H; A.W = K.W; A.Ho = K.Hout; A.Wo = K.Wout;
    for (int i = 0; i < DCVIC_MAX_SRC; ++i) { A.src[i] = K.src[i]; A.srcC[i] = K.srcC[i]; A.src_bs[i] = K.src_bs[i]; }
    A.wp = (const unsigned short*)packed;
    A.n_chunks = K.n_chunks; A.tiles_x = K.tiles_x; A.tiles_y = K.tiles_y; A.co_tiles = K.n_cotiles;
    if (upsample) conv3x3_bf16_kernel<true><<<(unsigned)K.nblocks, NTHREADS, 0, (hipStream_t)stream>>>(A, K);
    else conv3x3_bf16_kernel<false><<<(unsigned)K.nblocks, NTHREADS, 0, (hipStream_t)stream>>>(A, K);
    DCVIC_CHECK_LAUNCH("conv3x3_bf16");
    return DCVIC_OK;
}
