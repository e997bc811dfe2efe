// The ingest of a stored selection set (include/dcvic_tokens.h): uint8 HWC crops to fp32 NCHW through the caller's table, and stored
// VQ tokens to the encoder's index / latent / feature tensors in one launch.  Both kernels move bytes and compute nothing: lanes run
// along the pixel axis so that every output plane is written coalesced.
#include "common.h"
#include "dcvic_tokens.h"

namespace {

constexpr int THREADS = 256;
constexpr int PX = 4;                          // pixels per thread of u8_hwc_to_f32_nchw: 12 source bytes, three 32-bit words
constexpr int CH = 16;                         // channels per workgroup of vq_token_feat

// A thread owns pixels [4g, 4g + 4) of item blockIdx.y.  The 12 bytes are three word loads when the item's base is 4-byte aligned
// (then every group's first byte is) and the group lies wholly inside the item; else each byte that exists is loaded on its own.
__global__ __launch_bounds__(THREADS) void u8_hwc_to_f32_nchw_kernel(const unsigned char* __restrict__ src, int HW, const float* __restrict__ table,
                                                                    float* __restrict__ out) {
    __shared__ float conv[256];
    conv[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int p0 = ((int)blockIdx.x * THREADS + (int)threadIdx.x) * PX;
    if (p0 >= HW) return;
    const unsigned char* item = src + (size_t)blockIdx.y * HW * 3;
    float* o = out + (size_t)blockIdx.y * 3 * HW;
    const int np = min(PX, HW - p0);
    unsigned char b[3 * PX];
    if (np == PX && ((uintptr_t)item & 3) == 0) {
        const unsigned* q = (const unsigned*)(item + 3 * (size_t)p0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned v = q[k];
            b[4 * k] = v & 255u;
            b[4 * k + 1] = v >> 8 & 255u;
            b[4 * k + 2] = v >> 16 & 255u;
            b[4 * k + 3] = v >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * PX; ++k) b[k] = k < 3 * np ? item[3 * (size_t)p0 + k] : 0;
    }
    const bool wide = np == PX && (HW & 3) == 0 && ((uintptr_t)out & 15) == 0;     // then every plane and every group start on 16 bytes
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* oc = o + (size_t)c * HW + p0;
        if (wide) {
            *(float4*)oc = make_float4(conv[b[c]], conv[b[3 + c]], conv[b[6 + c]], conv[b[9 + c]]);
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j)
                if (j < np) oc[j] = conv[b[3 * j + c]];
        }
    }
}

// A thread owns position p of image blockIdx.y and the channels [c0, c0 + CH) of the feature tensor, c0 = blockIdx.z * CH: channels
// below D are codebook entries (written to zq and feat), channel D + j is the one-hot of code j.  blockIdx.z == 0 writes idx.
template <typename TOK>
__global__ __launch_bounds__(THREADS) void vq_token_feat_kernel(const TOK* __restrict__ tokens, const float* __restrict__ codebook, int hw, int D, int n_e,
                                                               int channels, long long* __restrict__ idx, float* __restrict__ zq,
                                                               float* __restrict__ feat) {
    const int p = (int)blockIdx.x * THREADS + (int)threadIdx.x;
    if (p >= hw) return;
    const size_t n = blockIdx.y;
    const long long t = (long long)tokens[n * hw + p];
    const bool ok = t >= 0 && t < n_e;
    const int ts = ok ? (int)t : 0;            // the only value used as an address
    if (blockIdx.z == 0 && idx) idx[n * hw + p] = t;
    const int c0 = (int)blockIdx.z * CH, c1 = min(c0 + CH, channels);
    for (int c = c0; c < c1; ++c) {
        if (c < D) {
            const float v = ok ? codebook[(size_t)ts * D + c] : __int_as_float(0x7fc00000);
            if (zq) zq[(n * D + c) * hw + p] = v;
            if (feat) feat[(n * (D + n_e) + c) * hw + p] = v;
        } else {
            feat[(n * (D + n_e) + c) * hw + p] = ok && c - D == ts ? 1.f : 0.f;     // channels > D only with feat
        }
    }
}

}  // namespace

extern "C" int dcvic_u8_hwc_to_f32_nchw(const unsigned char* src, int N, int H, int W, const float* table, float* out, void* stream) {
    DCVIC_CHECK_ARG(src && table && out, "u8_hwc_to_f32_nchw: null pointer (src %p, table %p, out %p)", (const void*)src, (const void*)table,
                    (void*)out);
    DCVIC_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "u8_hwc_to_f32_nchw: empty batch (N=%d, H=%d, W=%d)", N, H, W);
    DCVIC_CHECK_ARG(N <= 65535, "u8_hwc_to_f32_nchw: N=%d, at most 65535 images per launch", N);
    DCVIC_CHECK_ARG((long long)H * W <= (1LL << 28), "u8_hwc_to_f32_nchw: H * W = %lld, at most 2^28", (long long)H * W);
    DCVIC_CHECK_ARG(((uintptr_t)out & 3) == 0, "u8_hwc_to_f32_nchw: out %p must be 4-byte aligned", (void*)out);
    const int HW = H * W;
    u8_hwc_to_f32_nchw_kernel<<<dim3((unsigned)dcvic_cdiv(HW, THREADS * PX), (unsigned)N), THREADS, 0, (hipStream_t)stream>>>(src, HW, table, out);
    DCVIC_CHECK_LAUNCH("u8_hwc_to_f32_nchw");
    return DCVIC_OK;
}

extern "C" int dcvic_vq_token_feat_f32(const void* tokens, int token_bytes, const float* codebook, int N, int h, int w, int D, int n_e,
                                       long long* idx, float* zq, float* feat, void* stream) {
    DCVIC_CHECK_ARG(tokens && codebook, "vq_token_feat: null pointer (tokens %p, codebook %p)", tokens, (const void*)codebook);
    DCVIC_CHECK_ARG(idx || zq || feat, "vq_token_feat: no output requested (idx, zq and feat are all null)");
    DCVIC_CHECK_ARG(N >= 1 && h >= 1 && w >= 1 && D >= 1 && n_e >= 1, "vq_token_feat: empty problem (N=%d, h=%d, w=%d, D=%d, n_e=%d)", N, h, w, D, n_e);
    DCVIC_CHECK_ARG(N <= 65535, "vq_token_feat: N=%d, at most 65535 images per launch", N);
    DCVIC_CHECK_ARG((long long)h * w <= (1LL << 28), "vq_token_feat: h * w = %lld, at most 2^28", (long long)h * w);
    DCVIC_CHECK_ARG((long long)D + n_e <= (1LL << 19), "vq_token_feat: D + n_e = %lld, at most 2^19", (long long)D + n_e);
    DCVIC_CHECK_ARG(token_bytes == 1 || token_bytes == 8, "vq_token_feat: token_bytes=%d, tokens are uint8 (1) or int64 (8)", token_bytes);
    DCVIC_CHECK_ARG((token_bytes == 1 || ((uintptr_t)tokens & 7) == 0) && ((uintptr_t)idx & 7) == 0,
                    "vq_token_feat: int64 tokens %p and idx %p must be 8-byte aligned", tokens, (void*)idx);
    DCVIC_CHECK_ARG(((uintptr_t)zq & 3) == 0 && ((uintptr_t)feat & 3) == 0 && ((uintptr_t)codebook & 3) == 0,
                    "vq_token_feat: codebook %p, zq %p and feat %p must be 4-byte aligned", (const void*)codebook, (void*)zq, (void*)feat);
    const int hw = h * w, channels = feat ? D + n_e : zq ? D : 0;
    const dim3 grid((unsigned)dcvic_cdiv(hw, THREADS), (unsigned)N, (unsigned)max(1, dcvic_cdiv(channels, CH)));
    if (token_bytes == 1)
        vq_token_feat_kernel<unsigned char><<<grid, THREADS, 0, (hipStream_t)stream>>>((const unsigned char*)tokens, codebook, hw, D, n_e, channels, idx, zq, feat);
    else
        vq_token_feat_kernel<long long><<<grid, THREADS, 0, (hipStream_t)stream>>>((const long long*)tokens, codebook, hw, D, n_e, channels, idx, zq, feat);
    DCVIC_CHECK_LAUNCH("vq_token_feat");
    return DCVIC_OK;
}
