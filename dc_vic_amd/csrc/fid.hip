// HiFiC patch FID (the reference's scripts/calc_metrics.py:220-320: 256 x 256 patches through pytorch-fid's FID-Inception, pool3
// features, Frechet distance).  Parity with the pytorch_fid package unpinned (it is not in the reference tree).  The convolutions run on
// the project's conv kernels; this file holds what the network needs besides them:
//   * patch -> network input: ToTensor (u8 / 255 in fp32), F.interpolate(size=(S, S), mode="bilinear", align_corners=False), 2 x - 1;
//   * the Inception pools: max 3x3 / s2 valid, avg 3x3 / s1 / p1 with count_include_pad=False, max 3x3 / s1 / p1, global mean;
//   * the feature statistics: per-feature sums and the upper triangle of F^T F, accumulated in fp64 on the device.
// Every value depends on its own patch only and every sum has a fixed order: results are bitwise reproducible and batch-invariant (the
// statistics re-associate only at batch boundaries).
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int POOL_THREADS = 256;
constexpr int MEAN_THREADS = 256;                 // one wave per (image, channel) plane
constexpr int G_TILE = 64, G_THREADS = 256, G_KC = 16;
constexpr long long MAX_GRID_Y = 65535;

// One output pixel (all 3 channels) of one patch.  The source coordinate, the weights and the blend are computed in fp64 from the
// ToTensor value (float)u8 / 255.f and rounded once, so the result is within half an fp32 ulp of the fp64 F.interpolate of the same
// fp32 input (plus fp64 rounding).  Neighbour indices are clamped to the patch, and the patch to the image (the caller checks origins).
__global__ __launch_bounds__(RS_THREADS) void patch_resize_kernel(const unsigned char* __restrict__ img, int H, int W,
                                                                  const int* __restrict__ origins, int ph, int pw, int S, double sy,
                                                                  double sx, float* __restrict__ out, long long out_bs) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= S * S) return;
    const int b = blockIdx.y;
    const int oy = i / S, ox = i - oy * S;
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    double fy = sy * ((double)oy + 0.5) - 0.5, fx = sx * ((double)ox + 0.5) - 0.5;
    fy = fy < 0.0 ? 0.0 : fy;
    fx = fx < 0.0 ? 0.0 : fx;
    const int iy0 = (int)fy, ix0 = (int)fx;
    const int iy1 = iy0 + (iy0 < ph - 1 ? 1 : 0), ix1 = ix0 + (ix0 < pw - 1 ? 1 : 0);
    const double ly1 = fy - iy0, ly0 = 1.0 - ly1, lx1 = fx - ix0, lx0 = 1.0 - lx1;
    const int ry0 = min(y0 + iy0, H - 1), ry1 = min(y0 + iy1, H - 1);
    const int cx0 = min(x0 + ix0, W - 1), cx1 = min(x0 + ix1, W - 1);
    const unsigned char* r0 = img + (long long)ry0 * W * 3;
    const unsigned char* r1 = img + (long long)ry1 * W * 3;
    float* o = out + (long long)b * out_bs + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v00 = (float)r0[cx0 * 3 + c] / 255.f, v01 = (float)r0[cx1 * 3 + c] / 255.f;
        const double v10 = (float)r1[cx0 * 3 + c] / 255.f, v11 = (float)r1[cx1 * 3 + c] / 255.f;
        const double v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
        o[(long long)c * S * S] = (float)(2.0 * v - 1.0);
    }
}

// MODE 0: max 3x3 / s2, no padding.  MODE 1: avg 3x3 / s1 / p1 over the in-image taps only (count_include_pad=False), summed in fp64
// and rounded once.  MODE 2: max 3x3 / s1 / p1 (padding never wins).  Max pools propagate NaN as torch does.  One output per thread.
template <int MODE>
__global__ __launch_bounds__(POOL_THREADS) void pool3_kernel(const float* __restrict__ x, long long x_bs, float* __restrict__ y,
                                                             long long y_bs, int C, int H, int W, int Ho, int Wo, long long total) {
    const long long idx = (long long)blockIdx.x * POOL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % Wo);
    long long t = idx / Wo;
    const int oy = (int)(t % Ho);
    t /= Ho;
    const int c = (int)(t % C);
    const long long n = t / C;
    const float* xp = x + n * x_bs + (long long)c * H * W;
    const int s = MODE == 0 ? 2 : 1, p = MODE == 0 ? 0 : 1;
    const int iy0 = oy * s - p, ix0 = ox * s - p;
    float m = -INFINITY;
    double acc = 0.0;
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = iy0 + dy;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ix0 + dx;
            if (ix < 0 || ix >= W) continue;
            const float v = xp[(long long)iy * W + ix];
            if (MODE == 1) {
                acc += (double)v;
                ++cnt;
            } else if (v > m || isnan(v)) {
                m = v;
            }
        }
    }
    y[n * y_bs + (long long)c * Ho * Wo + (long long)oy * Wo + ox] = MODE == 1 ? (float)(acc / cnt) : m;
}

// y[n, c] = mean of plane (n, c): one wave per plane, lane-strided fp64 sums then a fixed butterfly, divided and rounded once.
__global__ __launch_bounds__(MEAN_THREADS) void mean_hw_kernel(const float* __restrict__ x, long long x_bs, float* __restrict__ y,
                                                               long long y_bs, int C, int HW, long long planes) {
    const long long pl = (long long)blockIdx.x * (MEAN_THREADS / 64) + (threadIdx.x >> 6);
    if (pl >= planes) return;                               // a whole wave leaves together: the shuffles below see full waves
    const int lane = threadIdx.x & 63;
    const long long n = pl / C;
    const int c = (int)(pl - n * C);
    const float* xp = x + n * x_bs + (long long)c * HW;
    double s = 0.0;
    for (int i = lane; i < HW; i += 64) s += (double)xp[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) y[n * y_bs + c] = (float)(s / HW);
}

// gram[i][j] += sum_b F[b][i] F[b][j] for one 64 x 64 tile (ti, tj), ti <= tj, entries with i <= j only.  Products of fp32 values are
// exact in fp64; each entry is one fma chain over the batch in row order, added to the buffer once: no atomics, fixed order.
__global__ __launch_bounds__(G_THREADS) void gram_kernel(const float* __restrict__ F, long long f_rs, int B, int D, int ntile,
                                                         double* __restrict__ gram) {
    __shared__ double As[G_KC][G_TILE], Bs[G_KC][G_TILE];
    int t = blockIdx.x, ti = 0;
    while (t >= ntile - ti) {
        t -= ntile - ti;
        ++ti;
    }
    const int tj = ti + t;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int k0 = 0; k0 < B; k0 += G_KC) {
        for (int e = threadIdx.x; e < G_KC * G_TILE; e += G_THREADS) {
            const int kk = e / G_TILE, col = e % G_TILE, row = k0 + kk;
            const int ci = ti * G_TILE + col, cj = tj * G_TILE + col;
            As[kk][col] = row < B && ci < D ? (double)F[(long long)row * f_rs + ci] : 0.0;
            Bs[kk][col] = row < B && cj < D ? (double)F[(long long)row * f_rs + cj] : 0.0;
        }
        __syncthreads();
        const int kn = B - k0 < G_KC ? B - k0 : G_KC;
        for (int kk = 0; kk < kn; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = As[kk][ty * 4 + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = Bs[kk][tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = ti * G_TILE + ty * 4 + r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = tj * G_TILE + tx * 4 + c;
            if (i < D && j < D && i <= j) gram[(long long)i * D + j] += acc[r][c];
        }
    }
}

// sum[j] += sum_b F[b][j], rows in order.
__global__ void colsum_kernel(const float* __restrict__ F, long long f_rs, int B, int D, double* __restrict__ sum) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= D) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)F[(long long)b * f_rs + j];
    sum[j] += s;
}

}  // namespace

extern "C" int dcvic_fid_patch_resize_f32(const unsigned char* img, int H, int W, const int* origins, int B, int ph, int pw, int S,
                                          float* out, long long out_bs, void* stream) {
    DCVIC_CHECK_ARG(img && origins && out && H > 0 && W > 0 && B > 0 && B <= MAX_GRID_Y && ph > 0 && pw > 0 && ph <= H && pw <= W && S > 0 &&
                    S <= 4096, "fid_patch_resize: bad argument");
    DCVIC_CHECK_ARG(out_bs >= 3LL * S * S, "fid_patch_resize: batch stride %lld < 3 * %d * %d", out_bs, S, S);
    // F.interpolate(size=...) scale: (double)in / out, as torch's area_pixel_compute_scale takes it
    const double sy = (double)ph / S, sx = (double)pw / S;
    patch_resize_kernel<<<dim3(dcvic_cdiv(S * S, RS_THREADS), B), RS_THREADS, 0, (hipStream_t)stream>>>(img, H, W, origins, ph, pw, S, sy, sx,
                                                                                                       out, out_bs);
    DCVIC_CHECK_LAUNCH("fid_patch_resize");
    return DCVIC_OK;
}

extern "C" int dcvic_fid_pool3_f32(int mode, const float* x, long long x_bs, int N, int C, int H, int W, float* y, long long y_bs,
                                   void* stream) {
    DCVIC_CHECK_ARG(x && y && N > 0 && C > 0 && H > 0 && W > 0 && mode >= 0 && mode <= 2, "fid_pool3: bad argument");
    DCVIC_CHECK_ARG(mode != 0 || (H >= 3 && W >= 3), "fid_pool3: a 3x3 / s2 valid pool needs H, W >= 3");
    const int Ho = mode == 0 ? (H - 3) / 2 + 1 : H, Wo = mode == 0 ? (W - 3) / 2 + 1 : W;
    DCVIC_CHECK_ARG(N == 1 || (x_bs >= (long long)C * H * W && y_bs >= (long long)C * Ho * Wo), "fid_pool3: batch stride too small");
    const long long total = (long long)N * C * Ho * Wo;
    const long long blocks = (total + POOL_THREADS - 1) / POOL_THREADS;
    DCVIC_CHECK_ARG(blocks <= 0x7fffffffLL, "fid_pool3: too many outputs");
    auto* k = mode == 0 ? pool3_kernel<0> : mode == 1 ? pool3_kernel<1> : pool3_kernel<2>;
    k<<<(unsigned)blocks, POOL_THREADS, 0, (hipStream_t)stream>>>(x, x_bs, y, y_bs, C, H, W, Ho, Wo, total);
    DCVIC_CHECK_LAUNCH("fid_pool3");
    return DCVIC_OK;
}

extern "C" int dcvic_fid_mean_hw_f32(const float* x, long long x_bs, int N, int C, int HW, float* y, long long y_bs, void* stream) {
    DCVIC_CHECK_ARG(x && y && N > 0 && C > 0 && HW > 0, "fid_mean_hw: bad argument");
    DCVIC_CHECK_ARG(N == 1 || (x_bs >= (long long)C * HW && y_bs >= C), "fid_mean_hw: batch stride too small");
    const long long planes = (long long)N * C;
    const long long blocks = (planes + MEAN_THREADS / 64 - 1) / (MEAN_THREADS / 64);
    DCVIC_CHECK_ARG(blocks <= 0x7fffffffLL, "fid_mean_hw: too many planes");
    mean_hw_kernel<<<(unsigned)blocks, MEAN_THREADS, 0, (hipStream_t)stream>>>(x, x_bs, y, y_bs, C, HW, planes);
    DCVIC_CHECK_LAUNCH("fid_mean_hw");
    return DCVIC_OK;
}

extern "C" int dcvic_fid_stats_accum_f64(const float* F, long long f_rs, int B, int D, double* sum, double* gram, void* stream) {
    DCVIC_CHECK_ARG(F && sum && gram && B > 0 && D > 0 && D <= 16384 && (B == 1 || f_rs >= D), "fid_stats_accum: bad argument");
    const int ntile = dcvic_cdiv(D, G_TILE);
    gram_kernel<<<ntile * (ntile + 1) / 2, G_THREADS, 0, (hipStream_t)stream>>>(F, f_rs, B, D, ntile, gram);
    DCVIC_CHECK_LAUNCH("fid_stats_gram");
    colsum_kernel<<<dcvic_cdiv(D, 256), 256, 0, (hipStream_t)stream>>>(F, f_rs, B, D, sum);
    DCVIC_CHECK_LAUNCH("fid_stats_colsum");
    return DCVIC_OK;
}
