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
#include "common.h"

namespace {

constexpr int ST_TX = 64, ST_TY = 16;                     // stats: output tile of one workgroup (4 rows per thread)
constexpr int ST_THREADS = 256;
constexpr int WIN = 11, HALO = WIN - 1;
constexpr int IN_W = ST_TX + HALO, IN_H = ST_TY + HALO;   // 74 x 26 input pixels per tile
constexpr int PL_TX = 64, PL_TY = 4;                      // pool: one output per thread
constexpr int FIN_THREADS = 256, FIN_MAX_C = 64;
constexpr int SCALES = 5;
constexpr long long MAX_GRID_Y = 65535;
constexpr int MIN_SIDE = 161;                             // pytorch-msssim asserts min(H, W) > (11 - 1) * 2^4

// torch's fp32 window: g = exp(-(k - 5)^2 / 4.5) / sum, as _fspecial_gauss_1d(11, 1.5) computes it (symmetric)
__constant__ float c_win[WIN] = {0x1.0d9570p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
                                 0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d9570p-10f};
// the package's weights, a torch.FloatTensor: fp32 values
constexpr double kWeights[SCALES] = {0x1.6f0068p-5, 0x1.247454p-2, 0x1.334d6ap-2, 0x1.e3f142p-3, 0x1.10ff98p-3};
// C1 = (K1 * data_range)^2, C2 = (K2 * data_range)^2: Python doubles, rounded to fp32 where they meet the fp32 maps
constexpr float kC1 = (float)((0.01 * 255.0) * (0.01 * 255.0)), kC2 = (float)((0.03 * 255.0) * (0.03 * 255.0));

__device__ __forceinline__ float to_u8(float v) { return truncf((v + 1.f) * 0.5f * 255.f); }

// sigma_ab of the package, G(ab) - G(a) G(b), from the moments of da = a - sa, db = b - sb (sa, sb: the tile's shifts) and the window's
// 2-D sum S = 1 - e: G(a) = G(da) + sa S, G(ab) = G(da db) + sa G(db) + sb G(da) + sa sb S.  The shift keeps G(da^2) small where the
// variance is small (no fp32 cancellation against mu^2); the e terms keep the value the package's, whose window does not sum to 1.
// Symmetric in (a, b): identical planes give sigma_xy == sigma_x^2 == sigma_y^2 bit for bit.
__device__ __forceinline__ float cov(float gab, float ga, float gb, float sa, float sb, float S, float e) {
    return (gab - ga * gb) + e * ((sa * gb + sb * ga) + sa * sb * S);
}

// Sum of 2 doubles over the workgroup: butterfly inside each wave, then the wave sums in wave order (fixed order).
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[2]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        red[w][0] = a;
        red[w][1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0.0;
        for (int i = 0; i < ST_THREADS / 64; ++i) {
            a += red[i][0];
            b += red[i][1];
        }
    }
}

// One 64 x 16 tile of the valid ssim / cs maps of one plane at one scale.  U8: the input is the raw [-1, 1] image (scale 0), truncated
// on load; otherwise a pooled plane.  part[(plane * tiles + tile) * 2 + {0, 1}] = sum over the tile of cs_map, ssim_map (fp64).
template <bool U8>
__global__ __launch_bounds__(ST_THREADS) void msssim_stats_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                                  int Ho, int Wo, int tiles_x, float S, float e, double* __restrict__ part) {
    __shared__ float sx[IN_H][IN_W], sy[IN_H][IN_W];
    __shared__ float hq[5][IN_H][ST_TX];
    __shared__ double red[ST_THREADS / 64][2];
    const long long pl = blockIdx.y;
    const float* xp = x + pl * H * W;
    const float* yp = y + pl * H * W;
    const int ox0 = (blockIdx.x % tiles_x) * ST_TX, oy0 = (blockIdx.x / tiles_x) * ST_TY;
    const int t = threadIdx.x;
    // the tile's shifts: the pixel at the centre of its input window (inside the plane)
    const long long ci = (long long)min(oy0 + IN_H / 2, H - 1) * W + min(ox0 + IN_W / 2, W - 1);
    const float sa = U8 ? to_u8(xp[ci]) : xp[ci], sb = U8 ? to_u8(yp[ci]) : yp[ci];
    for (int i = t; i < IN_H * IN_W; i += ST_THREADS) {
        const int r = i / IN_W, c = i % IN_W;
        const int gy = oy0 + r, gx = ox0 + c;
        float dx = 0.f, dy = 0.f;                          // outside the plane: feeds only outputs outside the valid map
        if (gy < H && gx < W) {
            const long long o = (long long)gy * W + gx;
            const float vx = xp[o], vy = yp[o];
            dx = (U8 ? to_u8(vx) : vx) - sa;               // exact: both are multiples of 4^-s in [0, 255]
            dy = (U8 ? to_u8(vy) : vy) - sb;
        }
        sx[r][c] = dx;
        sy[r][c] = dy;
    }
    __syncthreads();
    // horizontal pass: 26 rows x 64 columns, 5 moments
    const int c = t & (ST_TX - 1);
    for (int r = t / ST_TX; r < IN_H; r += ST_THREADS / ST_TX) {
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = c_win[k], a = sx[r][c + k], b = sy[r][c + k];
            m0 = fmaf(w, a, m0);
            m1 = fmaf(w, b, m1);
            m2 = fmaf(w, a * a, m2);
            m3 = fmaf(w, b * b, m3);
            m4 = fmaf(w, a * b, m4);
        }
        hq[0][r][c] = m0;
        hq[1][r][c] = m1;
        hq[2][r][c] = m2;
        hq[3][r][c] = m3;
        hq[4][r][c] = m4;
    }
    __syncthreads();
    // vertical pass: 4 consecutive output rows per thread from 14 rows of the horizontal moments
    const int r0 = (t / ST_TX) * 4;
    float acc[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[q][o] = 0.f;
#pragma unroll
    for (int j = 0; j < WIN + 3; ++j) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = hq[q][r0 + j][c];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = j - o;
            if (k >= 0 && k < WIN) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[q][o] = fmaf(c_win[k], v[q], acc[q][o]);
            }
        }
    }
    double cs_sum = 0.0, ss_sum = 0.0;
    const int ox = ox0 + c;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int oy = oy0 + r0 + o;
        if (oy < Ho && ox < Wo) {
            const float gx = acc[0][o], gy = acc[1][o];
            const float mux = sa * S + gx, muy = sb * S + gy;
            const float sxx = cov(acc[2][o], gx, gx, sa, sa, S, e);
            const float syy = cov(acc[3][o], gy, gy, sb, sb, S, e);
            const float sxy = cov(acc[4][o], gx, gy, sa, sb, S, e);
            const float cs = (2.f * sxy + kC2) / (sxx + syy + kC2);
            const float ss = (2.f * mux * muy + kC1) / (mux * mux + muy * muy + kC1) * cs;
            cs_sum += (double)cs;
            ss_sum += (double)ss;
        }
    }
    block_sum2(cs_sum, ss_sum, red);
    if (t == 0) {
        double* p = part + (pl * gridDim.x + blockIdx.x) * 2;
        p[0] = cs_sum;
        p[1] = ss_sum;
    }
}

// avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2), count_include_pad) of x and y -> px, py (either pair may be absent: PSNR only).
// U8 (scale 0): the input is truncated on load, and -- every input pixel lies in exactly one window -- the exact squared-error sum of the
// integer planes is written per (plane, tile) to sse_part.
template <bool U8>
__global__ __launch_bounds__(PL_TX * PL_TY) void msssim_pool_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                                   int Hp, int Wp, int tiles_x, float* __restrict__ px, float* __restrict__ py,
                                                                   unsigned long long* __restrict__ sse_part) {
    __shared__ unsigned long long red[PL_TX * PL_TY / 64];
    const long long pl = blockIdx.y;
    const int ox = (blockIdx.x % tiles_x) * PL_TX + (threadIdx.x % PL_TX);
    const int oy = (blockIdx.x / tiles_x) * PL_TY + (threadIdx.x / PL_TX);
    unsigned long long sse = 0;
    if (ox < Wp && oy < Hp) {
        const float* xp = x + pl * H * W;
        const float* yp = y + pl * H * W;
        const int iy0 = 2 * oy - (H & 1), ix0 = 2 * ox - (W & 1);
        float ax = 0.f, ay = 0.f;
        unsigned d2 = 0;
        // torch's order: rows, then columns; padded positions are skipped (they would add zeros)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int iy = iy0 + dy;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ix = ix0 + dx;
                if (ix < 0 || ix >= W) continue;
                const long long o = (long long)iy * W + ix;
                float vx = xp[o], vy = yp[o];
                if (U8) {
                    vx = to_u8(vx);
                    vy = to_u8(vy);
                    const int d = (int)vx - (int)vy;
                    d2 += (unsigned)(d * d);
                }
                ax += vx;
                ay += vy;
            }
        }
        if (px) {
            const long long o = pl * Hp * Wp + (long long)oy * Wp + ox;
            px[o] = ax * 0.25f;
            py[o] = ay * 0.25f;
        }
        sse = d2;
    }
    if (!U8) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sse += __shfl_xor(sse, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sse;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int i = 0; i < PL_TX * PL_TY / 64; ++i) s += red[i];
        sse_part[pl * gridDim.x + blockIdx.x] = s;
    }
}

struct Geom {
    int H[SCALES], W[SCALES];                 // plane size at each scale
    int tiles_x[SCALES], tiles[SCALES];       // stats tiles per plane
    long long count[SCALES];                  // valid-map pixels per plane
    int pool_tiles_x[SCALES - 1], pool_tiles[SCALES - 1];
    long long off_sse, off_part[SCALES], off_img[SCALES];   // workspace byte offsets (off_img[0] unused)
    long long bytes;
};

long long align256(long long b) { return (b + 255) & ~255LL; }

// Workspace: [sse partials (u64) | stats partials per scale (2 doubles per plane and tile) | pooled x, y per scale 1..4 (fp32)].
// With ms == false (PSNR only) only the first section.
Geom geometry(long long planes, int H, int W, bool ms) {
    Geom g{};
    g.H[0] = H;
    g.W[0] = W;
    for (int s = 1; s < SCALES; ++s) {
        g.H[s] = g.H[s - 1] / 2 + g.H[s - 1] % 2;
        g.W[s] = g.W[s - 1] / 2 + g.W[s - 1] % 2;
    }
    for (int s = 0; s < SCALES - 1; ++s) {
        g.pool_tiles_x[s] = dcvic_cdiv(g.W[s + 1], PL_TX);
        g.pool_tiles[s] = g.pool_tiles_x[s] * dcvic_cdiv(g.H[s + 1], PL_TY);
    }
    long long b = 0;
    g.off_sse = b;
    b = align256(b + planes * g.pool_tiles[0] * (long long)sizeof(unsigned long long));
    if (ms) {
        for (int s = 0; s < SCALES; ++s) {
            const int Ho = g.H[s] - HALO, Wo = g.W[s] - HALO;
            g.count[s] = (long long)Ho * Wo;
            g.tiles_x[s] = dcvic_cdiv(Wo, ST_TX);
            g.tiles[s] = g.tiles_x[s] * dcvic_cdiv(Ho, ST_TY);
            g.off_part[s] = b;
            b = align256(b + planes * g.tiles[s] * 2LL * (long long)sizeof(double));
        }
        for (int s = 1; s < SCALES; ++s) {
            g.off_img[s] = b;
            b = align256(b + 2 * planes * g.H[s] * (long long)g.W[s] * (long long)sizeof(float));
        }
    }
    g.bytes = b;
    return g;
}

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
    double S1 = 0.0;                                        // the window's sum and the 2-D window's, S = S1^2 = 1 - e
    for (float v : {0x1.0d9570p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f}) S1 += 2.0 * v;
    S1 += 0x1.106560p-2;
    const float S = (float)(S1 * S1), e = (float)(1.0 - S1 * S1);
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
                                                                      g.tiles_x[s], S, e, part);
            else
                msssim_stats_kernel<false><<<grid, ST_THREADS, 0, st>>>(xs + in_off, ys + in_off, g.H[s], g.W[s], g.H[s] - HALO, g.W[s] - HALO,
                                                                       g.tiles_x[s], S, e, part);
            DCVIC_CHECK_LAUNCH("msssim_stats");
        }
        if (!want_ms) break;
    }
    msssim_finish_kernel<<<N, FIN_THREADS, 0, st>>>(ws, g, C, want_ms, ms_ssim, psnr, sse);
    DCVIC_CHECK_LAUNCH("msssim_finish");
    return DCVIC_OK;
}
