// MS-SSIM and PSNR of image pairs in [-1, 1] (trainer validation; the reference's calc_ms_ssim / calc_psnr, src/utils/img_utils.py:104-160,
// on pytorch-msssim 0.2.1).  Parity with the package unpinned (it is not in the reference tree); restated:
//   * both images become trunc((v + 1) * 0.5 * 255) -- fp32, no contraction (this file builds with -ffp-contract=off), so the integer
//     planes equal torch's `.int()` / numpy's `astype(uint8)` bit for bit;
//   * per scale, per plane: 11-tap Gaussian (sigma 1.5, torch's fp32 window) separable valid filtering of x, y, x^2, y^2, xy;
//     cs_map = (2 s_xy + C2) / (s_x^2 + s_y^2 + C2), ssim_map = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs_map, means over the map;
//   * 5 scales, avg_pool2d(2, padding = size % 2, count_include_pad) in between (exact in fp32: every value is a multiple of 4^-s <= 255);
//   * per plane prod_{s<4} relu(cs_s)^w_s * relu(ssim_4)^w_4, averaged over the channels; PSNR = 10 log10(255^2 / mse) on the integers.
// The squared-error sum is an exact integer.  Every other sum has a fixed order that depends on the plane's size only: results are bitwise
// reproducible and batch-invariant.  No allocation or synchronisation: the launch path can be captured into a graph.
#include "ssim_core.h"

namespace {

using namespace ssim_core;                                // the tile kernels and the geometry, shared with csrc/msssim_loss.hip

constexpr int FIN_THREADS = 256, FIN_MAX_C = 64;
// torch's fp32 window: g = exp(-(k - 5)^2 / 4.5) / sum, as _fspecial_gauss_1d(11, 1.5) computes it (symmetric)
constexpr float c_win[WIN] = {0x1.0d9570p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
                              0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d9570p-10f};
// C1 = (K1 * data_range)^2, C2 = (K2 * data_range)^2: Python doubles, rounded to fp32 where they meet the fp32 maps
constexpr float kC1 = (float)((0.01 * 255.0) * (0.01 * 255.0)), kC2 = (float)((0.03 * 255.0) * (0.03 * 255.0));

// One workgroup per image: wave w takes planes c = w, w + 4, ...; lane l sums tiles l, l + 64, ... of every scale in order, then a fixed
// butterfly; the plane values are averaged in channel order by thread 0.  The squared errors are integers: any order is exact.
__global__ __launch_bounds__(FIN_THREADS) void msssim_finish_kernel(const unsigned char* __restrict__ ws, Geom g, int C, bool want_ms,
                                                                    double* __restrict__ ms, double* __restrict__ psnr, double* __restrict__ sse) {
    __shared__ double val[FIN_MAX_C];
    __shared__ unsigned long long sse_tot;
    const int n = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (want_ms) {
        for (int c = w; c < C; c += FIN_THREADS / 64) {
            const long long pl = (long long)n * C + c;
            double m[SCALES];
#pragma unroll
            for (int s = 0; s < SCALES; ++s) {
                const double* p = (const double*)(ws + g.off_part[s]) + pl * g.tiles[s] * 2 + (s == SCALES - 1 ? 1 : 0);
                double t = 0.0;
                for (int k = lane; k < g.tiles[s]; k += 64) t += p[(long long)k * 2];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
                m[s] = t / (double)g.count[s];
            }
            if (lane == 0) {
                double v = 1.0;
#pragma unroll
                for (int s = 0; s < SCALES; ++s) v *= pow(fmax(m[s], 0.0), kWeights[s]);
                val[c] = v;
            }
        }
    }
    if (w == 0) {
        const unsigned long long* p = (const unsigned long long*)(ws + g.off_sse) + (long long)n * C * g.pool_tiles[0];
        const long long len = (long long)C * g.pool_tiles[0];
        unsigned long long u = 0;
        for (long long k = lane; k < len; k += 64) u += p[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);
        if (lane == 0) sse_tot = u;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (want_ms) {
        double t = 0.0;
        for (int c = 0; c < C; ++c) t += val[c];
        ms[n] = t / (double)C;
    }
    const double e = (double)sse_tot;
    const double mse = e / ((double)C * g.H[0] * g.W[0]);
    sse[n] = e;
    psnr[n] = 10.0 * log10(65025.0 / mse);                 // identical images: inf, as numpy
}

}  // namespace

extern "C" long long dcvic_msssim_workspace_bytes(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return 0;
    return geometry((long long)N * C, H, W, H >= MIN_SIDE && W >= MIN_SIDE).bytes;
}

extern "C" int dcvic_msssim_psnr_f64(const float* x, const float* y, int N, int C, int H, int W, double* ms_ssim, double* psnr, double* sse,
                                     void* workspace, long long workspace_bytes, void* stream) {
    DCVIC_CHECK_ARG(x && y && psnr && sse && workspace && N > 0 && C > 0 && C <= FIN_MAX_C && H > 0 && W > 0, "msssim_psnr: bad argument");
    DCVIC_CHECK_ARG((long long)H * W <= 0x7fffffffLL, "msssim_psnr: plane of %d x %d too large", H, W);
    const bool want_ms = ms_ssim != nullptr;
    DCVIC_CHECK_ARG(!want_ms || (H >= MIN_SIDE && W >= MIN_SIDE), "msssim_psnr: MS-SSIM needs min(H, W) > 160, got %d x %d", H, W);
    const long long planes = (long long)N * C;
    const Geom g = geometry(planes, H, W, want_ms);
    DCVIC_CHECK_ARG(workspace_bytes >= g.bytes, "msssim_psnr: workspace of %lld bytes, need %lld", workspace_bytes, g.bytes);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    Window win;
    for (int k = 0; k < WIN; ++k) win.g[k] = c_win[k];
    float S, e;                                             // the 2-D window's sum S = 1 - e
    window_sums(win, &S, &e);
    // planes go on grid.y, at most 65535 per launch: groups of planes with offset pointers (a plane's values do not depend on the group)
    for (int s = 0; s < SCALES; ++s) {
        for (long long p0 = 0; p0 < planes; p0 += MAX_GRID_Y) {
            const unsigned np = (unsigned)(planes - p0 < MAX_GRID_Y ? planes - p0 : MAX_GRID_Y);
            const float* xs = s == 0 ? x : (const float*)(ws + g.off_img[s]);
            const float* ys = s == 0 ? y : xs + planes * g.H[s] * g.W[s];
            const long long in_off = p0 * g.H[s] * g.W[s];
            if (s < SCALES - 1) {                           // the next scale's planes (and at scale 0 the squared errors)
                float* xn = want_ms ? (float*)(ws + g.off_img[s + 1]) : nullptr;
                float* yn = want_ms ? xn + planes * g.H[s + 1] * g.W[s + 1] : nullptr;
                const long long out_off = p0 * g.H[s + 1] * g.W[s + 1];
                if (xn) {
                    xn += out_off;
                    yn += out_off;
                }
                const dim3 grid((unsigned)g.pool_tiles[s], np);
                if (s == 0)
                    msssim_pool_kernel<true><<<grid, PL_TX * PL_TY, 0, st>>>(xs + in_off, ys + in_off, g.H[0], g.W[0], g.H[1], g.W[1],
                                                                           g.pool_tiles_x[0], xn, yn,
                                                                           (unsigned long long*)(ws + g.off_sse) + p0 * g.pool_tiles[0]);
                else if (want_ms)
                    msssim_pool_kernel<false><<<grid, PL_TX * PL_TY, 0, st>>>(xs + in_off, ys + in_off, g.H[s], g.W[s], g.H[s + 1], g.W[s + 1],
                                                                            g.pool_tiles_x[s], xn, yn, nullptr);
                DCVIC_CHECK_LAUNCH("msssim_pool");
            }
            if (!want_ms) continue;
            double* part = (double*)(ws + g.off_part[s]) + p0 * g.tiles[s] * 2;
            const dim3 grid((unsigned)g.tiles[s], np);
            if (s == 0)
                msssim_stats_kernel<true><<<grid, ST_THREADS, 0, st>>>(xs + in_off, ys + in_off, g.H[s], g.W[s], g.H[s] - HALO, g.W[s] - HALO,
                                                                      g.tiles_x[s], win, S, e, kC1, kC2, part);
            else
                msssim_stats_kernel<false><<<grid, ST_THREADS, 0, st>>>(xs + in_off, ys + in_off, g.H[s], g.W[s], g.H[s] - HALO, g.W[s] - HALO,
                                                                       g.tiles_x[s], win, S, e, kC1, kC2, part);
            DCVIC_CHECK_LAUNCH("msssim_stats");
        }
        if (!want_ms) break;
    }
    msssim_finish_kernel<<<N, FIN_THREADS, 0, st>>>(ws, g, C, want_ms, ms_ssim, psnr, sse);
    DCVIC_CHECK_LAUNCH("msssim_finish");
    return DCVIC_OK;
}
