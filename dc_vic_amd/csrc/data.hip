// The device half of the training data feed (include/dcvic_data.h): one launch per batch resamples each crop's uint8 source window
// with Pillow's two integer passes, flips, converts through the caller's 256-entry table and writes fp32 NCHW.
//
// A workgroup of 256 threads owns a TH x TW = 8 x 32 output tile of one image; thread (ly, lx) owns output row ty + ly, column
// tx + lx, and keeps that column's and that row's coefficients in registers.  The tile's source rows [r_lo, r_hi), found from the
// row tables' bounds, are walked in chunks of RMAX: the row pass turns each chunk row into TW uint8 RGB values in LDS (lanes along x:
// neighbouring lanes read neighbouring source bytes), the column pass accumulates each thread's taps that fall into the chunk.  One
// chunk serves every scale the feed produces (8 rows at scale 1/4 read 8 * 4 + 17 rows); the chunk loop only bounds the LDS for any
// table.  The work is a few MB of bytes per batch: the launch is latency, not throughput.
#include "common.h"
#include "dcvic_data.h"

namespace {

constexpr int TW = 32, TH = 8, THREADS = TW * TH, RMAX = 64, KMAX = DCVIC_DATA_MAX_KSIZE;
constexpr unsigned HALF = 1u << 21;            // Pillow: ss0 = 1 << (PRECISION_BITS - 1), PRECISION_BITS = 22

// Sums are formed in unsigned arithmetic (wrap-around is defined) and shifted as int: Pillow's int32 sum and arithmetic shift.
__device__ __forceinline__ unsigned clip8(unsigned s) {
    const int v = (int)s >> 22;
    return (unsigned)min(max(v, 0), 255);
}

// Output index o's entry of one axis: first source index, tap count and coefficients, clamped to the window's extent.  k = 0 is
// "copy": one tap of weight 1.0, for which clip8 returns the pixel itself.
__device__ __forceinline__ void load_axis(const unsigned char* slab, long long tab, int k, int S, int o, int extent, int& first, int& cnt,
                                          int (&c)[KMAX]) {
    const bool live = o < S;
    const int* t = (const int*)(slab + tab);
    first = !live ? 0 : k == 0 ? o : t[(size_t)S * k + o];
    cnt = !live ? 0 : k == 0 ? 1 : t[(size_t)S * k + S + o];
    first = min(max(first, 0), extent);
    cnt = min(max(cnt, 0), min(max(k, 1), extent - first));
#pragma unroll
    for (int j = 0; j < KMAX; ++j) c[j] = j >= cnt ? 0 : k == 0 ? (1 << 22) : t[(size_t)o * k + j];
}

__global__ __launch_bounds__(THREADS) void u8_resample_crop_kernel(const unsigned char* __restrict__ slab, const dcvic_crop_desc* __restrict__ desc,
                                                                  int S, int tiles_x, const float* __restrict__ table,
                                                                  float* __restrict__ out) {
    __shared__ unsigned hrow[RMAX][TW];        // the row pass's result: R | G << 8 | B << 16
    __shared__ float conv[256];
    __shared__ int rowb[TH][2];
    const int t = threadIdx.x, lx = t % TW, ly = t / TW;
    const dcvic_crop_desc d = desc[blockIdx.y];
    const int ox = (int)(blockIdx.x % tiles_x) * TW + lx, oy = (int)(blockIdx.x / tiles_x) * TH + ly;

    int xmin, xcnt, cx[KMAX], ymin, ycnt, cy[KMAX];
    load_axis(slab, d.tab_x, d.kx, S, ox, d.src_w, xmin, xcnt, cx);
    load_axis(slab, d.tab_y, d.ky, S, oy, d.src_h, ymin, ycnt, cy);
    conv[t] = table[t];
    if (lx == 0) {
        rowb[ly][0] = ymin;
        rowb[ly][1] = ycnt;
    }
    __syncthreads();
    int r_lo = d.src_h, r_hi = 0;               // the same for every thread of the block
#pragma unroll
    for (int j = 0; j < TH; ++j)
        if (rowb[j][1] > 0) {
            r_lo = min(r_lo, rowb[j][0]);
            r_hi = max(r_hi, rowb[j][0] + rowb[j][1]);
        }

    const unsigned char* src = slab + d.src_off;
    unsigned a0 = HALF, a1 = HALF, a2 = HALF;
    for (int cr = r_lo; cr < r_hi; cr += RMAX) {
        const int rows = min(RMAX, r_hi - cr);
        for (int r = ly; r < rows; r += TH) {
            const unsigned char* p = src + (long long)(cr + r) * d.src_stride + 3 * xmin;
            unsigned s0 = HALF, s1 = HALF, s2 = HALF;
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < xcnt) {
                    const unsigned c = (unsigned)cx[j];
                    s0 += p[3 * j] * c;
                    s1 += p[3 * j + 1] * c;
                    s2 += p[3 * j + 2] * c;
                }
            hrow[r][lx] = clip8(s0) | clip8(s1) << 8 | clip8(s2) << 16;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            const int r = ymin + j - cr;
            if (j < ycnt && r >= 0 && r < rows) {
                const unsigned v = hrow[r][lx], c = (unsigned)cy[j];
                a0 += (v & 255u) * c;
                a1 += (v >> 8 & 255u) * c;
                a2 += (v >> 16) * c;
            }
        }
        __syncthreads();
    }
    if (ox < S && oy < S) {
        const int xf = d.flip ? S - 1 - ox : ox;
        const size_t plane = (size_t)S * S, at = ((size_t)blockIdx.y * 3 * S + oy) * S + xf;
        out[at] = conv[clip8(a0)];
        out[at + plane] = conv[clip8(a1)];
        out[at + 2 * plane] = conv[clip8(a2)];
    }
}

}  // namespace

extern "C" int dcvic_u8_resample_crop_f32(const unsigned char* slab, long long slab_bytes, const dcvic_crop_desc* desc_dev,
                                          const dcvic_crop_desc* desc_host, int N, int S, const float* table, float* out, void* stream) {
    DCVIC_CHECK_ARG(slab && desc_dev && desc_host && table && out,
                    "u8_resample_crop: null pointer (slab %p, desc_dev %p, desc_host %p, table %p, out %p)", (const void*)slab, (const void*)desc_dev,
                    (const void*)desc_host, (const void*)table, (void*)out);
    DCVIC_CHECK_ARG(N >= 1 && S >= 1, "u8_resample_crop: empty batch (N=%d, S=%d)", N, S);
    DCVIC_CHECK_ARG(N <= 65535, "u8_resample_crop: N=%d, at most 65535 images per launch", N);
    DCVIC_CHECK_ARG(S <= DCVIC_DATA_MAX_S, "u8_resample_crop: S=%d, at most %d", S, DCVIC_DATA_MAX_S);
    DCVIC_CHECK_ARG(slab_bytes >= 1 && ((uintptr_t)slab & 3) == 0, "u8_resample_crop: slab %p of %lld bytes must be 4-byte aligned and not empty",
                    (const void*)slab, slab_bytes);
    DCVIC_CHECK_ARG(((uintptr_t)desc_dev & 7) == 0 && ((uintptr_t)desc_host & 7) == 0, "u8_resample_crop: descriptors (device %p, host %p) must be 8-byte aligned",
                    (const void*)desc_dev, (const void*)desc_host);
    for (int n = 0; n < N; ++n) {
        const dcvic_crop_desc& d = desc_host[n];
        DCVIC_CHECK_ARG(d.kx >= 0 && d.kx <= DCVIC_DATA_MAX_KSIZE && d.ky >= 0 && d.ky <= DCVIC_DATA_MAX_KSIZE,
                        "u8_resample_crop: image %d has ksize x %d, y %d, outside [0, %d]", n, d.kx, d.ky, DCVIC_DATA_MAX_KSIZE);
        DCVIC_CHECK_ARG(d.src_h >= 1 && d.src_w >= 1 && d.src_stride >= 3LL * d.src_w && d.src_off >= 0 && d.src_off <= slab_bytes &&
                            (long long)(d.src_h - 1) * d.src_stride + 3LL * d.src_w <= slab_bytes - d.src_off,
                        "u8_resample_crop: image %d's window (%d x %d, stride %d, at byte %lld) lies outside its slab of %lld bytes", n, d.src_h,
                        d.src_w, d.src_stride, d.src_off, slab_bytes);
        DCVIC_CHECK_ARG((d.kx != 0 || d.src_w == S) && (d.ky != 0 || d.src_h == S),
                        "u8_resample_crop: image %d copies an axis whose window extent (%d x %d) is not S=%d", n, d.src_h, d.src_w, S);
        const long long tabs[2] = {d.tab_x, d.tab_y};
        const int ks[2] = {d.kx, d.ky};
        for (int a = 0; a < 2; ++a)
            DCVIC_CHECK_ARG(ks[a] == 0 || (tabs[a] >= 0 && (tabs[a] & 3) == 0 && tabs[a] <= slab_bytes &&
                                           4LL * S * (ks[a] + 2) <= slab_bytes - tabs[a]),
                            "u8_resample_crop: image %d's %c table (ksize %d, at byte %lld) is misaligned or lies outside its slab of %lld bytes", n,
                            a ? 'y' : 'x', ks[a], tabs[a], slab_bytes);
    }
    const int tiles_x = dcvic_cdiv(S, TW), tiles_y = dcvic_cdiv(S, TH);
    u8_resample_crop_kernel<<<dim3((unsigned)(tiles_x * tiles_y), (unsigned)N), THREADS, 0, (hipStream_t)stream>>>(slab, desc_dev, S, tiles_x, table,
                                                                                                                out);
    DCVIC_CHECK_LAUNCH("u8_resample_crop");
    return DCVIC_OK;
}
