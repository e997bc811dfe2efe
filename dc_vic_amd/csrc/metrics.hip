// Full-reference image metrics (scripts/calc_metrics.py: LPIPS and DISTS).  DISTS (Ding et al. 2020, the DISTS_pytorch package)
// restated; parity with the package unpinned (it is not in the reference tree):
//   * L2pool(x) = sqrt(depthwise_conv2d(x^2, g, stride 2, pad 1) + 1e-12), g = outer(a, a) / 16, a = [1, 2, 1]  (hanning(5)[1:-1] * 2);
//   * per (image, channel) moments of two feature maps: mu_x, mu_y, var_x, var_y (two-pass definitions), cov_xy = mean(xy) - mu_x mu_y;
//   * DISTS = 1 - sum_taps sum_c (alpha_c S1 + beta_c S2), S1 = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1),
//     S2 = (2 cov + c2) / (var_x + var_y + c2), c1 = c2 = 1e-6, alpha / beta already divided by their joint sum.
// Every sum has a fixed order that depends on the plane length only: results are bitwise reproducible and batch-invariant.
#include "common.h"

namespace {

constexpr int L2P_TX = 64, L2P_TY = 4;          // one output per thread, 64 x 4 outputs per workgroup
constexpr int MOM_THREADS = 256, MOM_PER_THREAD = 16;
constexpr int MOM_CHUNK = MOM_THREADS * MOM_PER_THREAD;   // elements of one plane per partial (4096)
constexpr int FIN_THREADS = 256;                              // finishing pass: 4 planes (one per wave) per workgroup
constexpr int SCORE_MAX_C = 2048;
constexpr long long MAX_GRID_Y = 65535;

// One output of the Hann 3x3 / stride-2 / pad-1 pool of squares.  x^2 and the integer weights are exact in fp64 and the 9-term sum
// is rounded at most a few times at fp64 precision, so the fp32 result is the correctly rounded value up to a rare double rounding.
__global__ __launch_bounds__(L2P_TX * L2P_TY) void l2pool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int Ho,
                                                                 int Wo, int tiles_x) {
    const int ox = (blockIdx.x % tiles_x) * L2P_TX + (threadIdx.x % L2P_TX);
    const int oy = (blockIdx.x / tiles_x) * L2P_TY + (threadIdx.x / L2P_TX);
    if (ox >= Wo || oy >= Ho) return;
    const long long pl = blockIdx.y;
    const float* xp = x + pl * H * W;
    double acc = 0.0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy - 1 + dy;
        if (iy < 0 || iy >= H) continue;
        const double wy = dy == 1 ? 2.0 : 1.0;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox - 1 + dx;
            if (ix < 0 || ix >= W) continue;
            const double v = (double)xp[(long long)iy * W + ix];
            acc = fma(wy * (dx == 1 ? 2.0 : 1.0) * v, v, acc);
        }
    }
    y[pl * Ho * Wo + (long long)oy * Wo + ox] = (float)sqrt(acc * 0.0625 + 1e-12);
}

// Sum of 5 doubles over the workgroup: butterfly inside each wave, then the 4 wave sums in wave order (fixed order).
__device__ __forceinline__ void block_sum5(double (&s)[5], double (*red)[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < 5; ++j) red[w][j] = s[j];
    __syncthreads();
    if (threadIdx.x < 5) {
        double t = 0.0;
        for (int i = 0; i < MOM_THREADS / 64; ++i) t += red[i][threadIdx.x];
        s[0] = t;
    }
}

// Partial sums of one MOM_CHUNK slice of one plane, shifted by the plane's first element (sx, sy): with dx = x - sx, dy = y - sy,
// part = [sum dx, sum dy, sum dx^2, sum dy^2, sum dx dy].  x - sx is exact in fp64, and the shift removes the mean's cancellation
// from the variance (a plane of mean 1e3 and std 1e-3 keeps its digits); a constant plane sums to exactly 0.  f1 == f0 (a plane's own
// mean, as LPIPS takes it) reads the plane once.
__global__ __launch_bounds__(MOM_THREADS) void moments_partial_kernel(const float* __restrict__ f0, const float* __restrict__ f1, long long HW,
                                                                      double* __restrict__ part) {
    __shared__ double red[MOM_THREADS / 64][5];
    const long long pl = blockIdx.y;
    const float* a = f0 + pl * HW;
    const float* b = f1 + pl * HW;
    const bool same = f0 == f1;
    const float ax = a[0], bx = b[0];
    const long long i0 = (long long)blockIdx.x * MOM_CHUNK + threadIdx.x;
    float va[MOM_PER_THREAD], vb[MOM_PER_THREAD];
#pragma unroll
    for (int k = 0; k < MOM_PER_THREAD; ++k) {                  // all loads first: 32 in flight per lane
        const long long i = i0 + (long long)k * MOM_THREADS;
        va[k] = i < HW ? a[i] : ax;                               // out of range reads as the shift: contributes exact zeros
    }
    if (same) {
#pragma unroll
        for (int k = 0; k < MOM_PER_THREAD; ++k) vb[k] = va[k];
    } else {
#pragma unroll
        for (int k = 0; k < MOM_PER_THREAD; ++k) {
            const long long i = i0 + (long long)k * MOM_THREADS;
            vb[k] = i < HW ? b[i] : bx;
        }
    }
    const double sx = ax, sy = bx;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < MOM_PER_THREAD; ++k) {
        const double dx = (double)va[k] - sx, dy = (double)vb[k] - sy;
        s[0] += dx;
        s[1] += dy;
        s[2] = fma(dx, dx, s[2]);
        s[3] = fma(dy, dy, s[3]);
        s[4] = fma(dx, dy, s[4]);
    }
    block_sum5(s, red);
    if (threadIdx.x < 5) part[(pl * gridDim.x + blockIdx.x) * 5 + threadIdx.x] = s[0];
}

// One wave per plane: lane l sums the partials of chunks l, l + 64, ... in order, then a butterfly over the 64 lanes (a fixed
// tree: the same bits every run), then lane 0 writes the moments.
__global__ __launch_bounds__(FIN_THREADS) void moments_finish_kernel(const float* __restrict__ f0, const float* __restrict__ f1, long long HW,
                                                                     const double* __restrict__ part, int chunks, int C, long long planes,
                                                                     double* __restrict__ out, long long out_bs) {
    const long long pl = (long long)blockIdx.x * (FIN_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pl >= planes) return;                                     // whole waves leave together
    const double* p = part + pl * chunks * 5;
    double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < chunks; k += 64)
#pragma unroll
        for (int j = 0; j < 5; ++j) t[j] += p[(long long)k * 5 + j];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t[j] += __shfl_xor(t[j], o, 64);
    if (lane != 0) return;
    const double inv = 1.0 / (double)HW;
    const double mx = t[0] * inv, my = t[1] * inv;                // means of the shifted values
    double* o = out + (pl / C) * out_bs + (pl % C) * 5;
    o[0] = (double)f0[pl * HW] + mx;
    o[1] = (double)f1[pl * HW] + my;
    o[2] = fmax(t[2] * inv - mx * mx, 0.0);
    o[3] = fmax(t[3] * inv - my * my, 0.0);
    o[4] = t[4] * inv - mx * my;                                  // covariance is shift-invariant
}

// One workgroup per image: every thread scores some channels into LDS, then thread 0 sums them in channel order -- first the alpha
// (mean) terms, then the beta (structure) terms, as the package accumulates dist1 and dist2.
__global__ __launch_bounds__(256) void dists_score_kernel(const double* __restrict__ mom, long long mom_bs, const double* __restrict__ alpha,
                                                          const double* __restrict__ beta, int C, double* __restrict__ out) {
    __shared__ double ta[SCORE_MAX_C], tb[SCORE_MAX_C];
    const int n = blockIdx.x;
    const double c1 = 1e-6, c2 = 1e-6;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const double* m = mom + (long long)n * mom_bs + (long long)c * 5;
        const double mx = m[0], my = m[1], vx = m[2], vy = m[3], cxy = m[4];
        ta[c] = alpha[c] * ((2.0 * mx * my + c1) / (mx * mx + my * my + c1));
        tb[c] = beta[c] * ((2.0 * cxy + c2) / (vx + vy + c2));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double d1 = 0.0, d2 = 0.0;
        for (int c = 0; c < C; ++c) d1 += ta[c];
        for (int c = 0; c < C; ++c) d2 += tb[c];
        out[n] = 1.0 - (d1 + d2);
    }
}

// out[n] = sum_k mom[n][k].mu_x in tap order: the LPIPS value of image n from the spatial means of its per-tap distance maps.
__global__ void lpips_score_kernel(const double* __restrict__ mom, int N, int taps, double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double t = 0.0;
    for (int k = 0; k < taps; ++k) t += mom[((long long)n * taps + k) * 5];
    out[n] = t;
}

}  // namespace

extern "C" int dcvic_l2pool_f32(const float* x, float* y, long long planes, int H, int W, void* stream) {
    DCVIC_CHECK_ARG(x && y && planes > 0 && H > 0 && W > 0, "l2pool: bad argument");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int tiles_x = dcvic_cdiv(Wo, L2P_TX);
    const long long tiles = (long long)tiles_x * dcvic_cdiv(Ho, L2P_TY);
    DCVIC_CHECK_ARG(tiles <= 0x7fffffffLL, "l2pool: plane too large");
    for (long long p0 = 0; p0 < planes; p0 += 65535) {              // grid.y limit
        const int np = (int)(planes - p0 < 65535 ? planes - p0 : 65535);
        l2pool_kernel<<<dim3((unsigned)tiles, np), L2P_TX * L2P_TY, 0, (hipStream_t)stream>>>(x + p0 * H * W, y + p0 * Ho * Wo, H, W, Ho, Wo,
                                                                                              tiles_x);
        DCVIC_CHECK_LAUNCH("l2pool");
    }
    return DCVIC_OK;
}

extern "C" long long dcvic_pair_moments_workspace_doubles(long long planes, long long HW) {
    if (planes <= 0 || HW <= 0) return 0;
    return planes * dcvic_cdiv(HW, MOM_CHUNK) * 5;
}

extern "C" int dcvic_pair_moments_f64(const float* f0, const float* f1, int N, int C, long long HW, double* out, long long out_bs,
                                      double* workspace, void* stream) {
    DCVIC_CHECK_ARG(f0 && f1 && out && workspace && N > 0 && C > 0 && HW > 0 && out_bs >= 5LL * C, "pair_moments: bad argument");
    const long long planes = (long long)N * C;
    const long long chunks = (HW + MOM_CHUNK - 1) / MOM_CHUNK;
    DCVIC_CHECK_ARG(chunks <= 0x7fffffffLL, "pair_moments: plane too large");
    // planes go on grid.y, at most 65535 per launch: groups of planes with offset pointers (a plane's partials do not depend on the group)
    for (long long p0 = 0; p0 < planes; p0 += MAX_GRID_Y) {
        const unsigned np = (unsigned)(planes - p0 < MAX_GRID_Y ? planes - p0 : MAX_GRID_Y);
        moments_partial_kernel<<<dim3((unsigned)chunks, np), MOM_THREADS, 0, (hipStream_t)stream>>>(f0 + p0 * HW, f1 + p0 * HW, HW,
                                                                                                    workspace + p0 * chunks * 5);
        DCVIC_CHECK_LAUNCH("pair_moments_partial");
    }
    moments_finish_kernel<<<dcvic_cdiv(planes, FIN_THREADS / 64), FIN_THREADS, 0, (hipStream_t)stream>>>(f0, f1, HW, workspace, (int)chunks, C,
                                                                                                       planes, out, out_bs);
    DCVIC_CHECK_LAUNCH("pair_moments_finish");
    return DCVIC_OK;
}

extern "C" int dcvic_dists_score_f64(const double* mom, long long mom_bs, const double* alpha, const double* beta, int N, int C, double* out,
                                     void* stream) {
    DCVIC_CHECK_ARG(mom && alpha && beta && out && N > 0 && C > 0 && C <= SCORE_MAX_C && mom_bs >= 5LL * C, "dists_score: bad argument");
    dists_score_kernel<<<N, 256, 0, (hipStream_t)stream>>>(mom, mom_bs, alpha, beta, C, out);
    DCVIC_CHECK_LAUNCH("dists_score");
    return DCVIC_OK;
}

extern "C" int dcvic_lpips_score_f64(const double* mom, int N, int taps, double* out, void* stream) {
    DCVIC_CHECK_ARG(mom && out && N > 0 && taps > 0, "lpips_score: bad argument");
    lpips_score_kernel<<<dcvic_cdiv(N, 256), 256, 0, (hipStream_t)stream>>>(mom, N, taps, out);
    DCVIC_CHECK_LAUNCH("lpips_score");
    return DCVIC_OK;
}
