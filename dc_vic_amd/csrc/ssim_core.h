// ssim_core.h -- what the validation MS-SSIM (csrc/ssim.hip) and the MS-SSIM training loss (csrc/msssim_loss.hip) share: the scale
// weights of pytorch-msssim 0.2.1, the shifted-moment (co)variance, the per-tile statistics kernel, the 2x2 average pool and
// the geometry of the five scales.  The arithmetic is fp32 without contraction: both translation units build with -ffp-contract=off.
#pragma once
#include "common.h"

namespace ssim_core {

constexpr int ST_TX = 64, ST_TY = 16;                     // stats: output tile of one workgroup (4 rows per thread)
constexpr int ST_THREADS = 256;
constexpr int WIN = 11, HALO = WIN - 1;
constexpr int IN_W = ST_TX + HALO, IN_H = ST_TY + HALO;   // 74 x 26 input pixels per tile
constexpr int PL_TX = 64, PL_TY = 4;                      // pool: one output per thread
constexpr int SCALES = 5;
constexpr long long MAX_GRID_Y = 65535;
constexpr int MIN_SIDE = 161;                             // pytorch-msssim asserts min(H, W) > (11 - 1) * 2^4

// The 11 taps, passed to the kernels by value: g = exp(-(k - 5)^2 / 4.5) / sum in fp32, as _fspecial_gauss_1d(11, 1.5) computes it.  Each
// translation unit states the literals itself (ssim.hip's are the ones tests/test_ssim_host.py reads; the loss's are held to the same
// values by tests/test_msssim_loss_host.py).
struct Window {
    float g[WIN];
};
// the package's weights, a torch.FloatTensor: fp32 values
constexpr double kWeights[SCALES] = {0x1.6f0068p-5, 0x1.247454p-2, 0x1.334d6ap-2, 0x1.e3f142p-3, 0x1.10ff98p-3};

// the 2-D window's sum S = (sum of the 11 taps)^2 = 1 - e, in fp64 (the symmetric pairs first, then the centre) and rounded once
inline void window_sums(const Window& win, float* S, float* e) {
    double S1 = 0.0;
    for (int k = 0; k < WIN / 2; ++k) S1 += 2.0 * win.g[k];
    S1 += win.g[WIN / 2];
    *S = (float)(S1 * S1);
    *e = (float)(1.0 - S1 * S1);
}

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
// on load; otherwise the planes as they are.  C1, C2: the package's constants for the data range, rounded to fp32.
// part[(plane * tiles + tile) * 2 + {0, 1}] = sum over the tile of cs_map, ssim_map (fp64).
template <bool U8>
__global__ __launch_bounds__(ST_THREADS) void msssim_stats_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                                  int Ho, int Wo, int tiles_x, Window win, float S, float e, float C1, float C2,
                                                                  double* __restrict__ part) {
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
            dx = (U8 ? to_u8(vx) : vx) - sa;               // U8 and pooled integer planes: exact, multiples of 4^-s in [0, 255]
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
            const float w = win.g[k], a = sx[r][c + k], b = sy[r][c + k];
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
                for (int q = 0; q < 5; ++q) acc[q][o] = fmaf(win.g[k], v[q], acc[q][o]);
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
            const float cs = (2.f * sxy + C2) / (sxx + syy + C2);
            const float ss = (2.f * mux * muy + C1) / (mux * mux + muy * muy + C1) * cs;
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

inline long long align256(long long b) { return (b + 255) & ~255LL; }

// Workspace: [sse partials (u64) | stats partials per scale (2 doubles per plane and tile) | pooled x, y per scale 1..4 (fp32)].
// With ms == false (PSNR only) only the first section.
inline Geom geometry(long long planes, int H, int W, bool ms) {
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

}  // namespace ssim_core
