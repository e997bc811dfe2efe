// msssim_loss.hip -- the image distortions MSSSIMLoss and L1Loss of the rate-distortion trainer, value and gradient
// (include/dcvic_msssim_loss.h; reference: src/losses/distortion_loss.py, MS_SSIM(data_range=1, size_average=True, channel=3) of
// pytorch-msssim 0.2.1 on the trainer's [-1, 1] images, `fake` unclamped; parity with the package unpinned, restated as in ssim.hip).
//
// Forward: the tile statistics and the pools of csrc/ssim_core.h on the float planes with C1 = 0.01^2, C2 = 0.03^2 -- (co)variances from
// tile-shifted moments, so near-identical images and flat patches lose nothing to cancellation -- then msssim_loss_finish_kernel: per
// plane the five means in msssim_finish_kernel's order, V = prod relu(f_s)^w_s, 1 - V, and the per-pixel seeds
//   u_s = dLoss/df_s / (Ho_s Wo_s) = -scale w_s V / f_s / (Ho_s Wo_s)         (0 for every scale of a plane with a factor <= 0)
// and msssim_loss_total_kernel: loss = scale * sum_planes (1 - V), one wave, planes lane-strided in ascending order, then a lane tree.
//
// Backward, scales 4 .. 0, one kernel per scale (msssim_grad_kernel): a workgroup owns a 32 x 16 tile of the scale's PLANE.  With
//   D = s_x^2 + s_y^2 + C2,  l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1),  l' = l at scale 4, else 1,
//   Pxy = u l' 2 / D,  Pyy = -u l' cs / D,  Pl = u cs (2 mu_x - 2 mu_y l) / (mu_x^2 + mu_y^2 + C1) at scale 4, else 0,
//   dy_s(p) = sum_q g(q - p) [Pl(q) + Pxy(q) (x(p) - mu_x(q)) + 2 Pyy(q) (y(p) - mu_y(q))]     q over the valid map: the filter's adjoint
// it recomputes the moments on the tile plus a 10-pixel ring of the valid map (from a 52 x 36 input window), forms three maps there
// (zero outside the valid map), filters them with the two-pass window and combines them with its own x(p), y(p).  Near-identical
// images are the regime training lives in: there Pxy x and 2 Pyy y are two large terms whose sum is small.  So the bracket is
// regrouped around the difference d = x - y, whose moments are taken directly (G(dx), G(d), G(dx^2), G(dy^2), G(d^2) in place of the
// forward's five): 1 - cs = s_d^2 / D exactly, and with A1 = 2 u l' / D, A2 = A1 (1 - cs)
//   Pxy (x(p) - mu_x) + 2 Pyy (y(p) - mu_y) = A1 (d(p) - (mu_x - mu_y)) + A2 (y(p) - mu_y)
//   dy_s(p) = adj(B)(p) + d(p) adj(A1)(p) + y(p) adj(A2)(p),   B = Pl - A1 (mu_x - mu_y) - A2 mu_y
// -- the same sum, no cancellation; identical planes give exactly 0.  x, y and the means enter shifted by the tile's centre pixel
// (y(p) - mu_y(q) = dy(p) - (G(dy)(q) - sb e)), as in the forward.  The coarser scale's gradient arrives through the pool's adjoint,
// 1/4 of the one pooled pixel above p.  Every element of dy_s is written exactly once; scale 0 writes dfake.
//
// This file builds with -ffp-contract=off: identical planes give cs == l == 1 and a loss of exactly 0 only if mu^2 + mu^2 and
// 2 mu mu round the same way.
#include "dcvic_msssim_loss.h"
#include "ssim_core.h"

namespace {

using namespace ssim_core;

// C1 = (K1 * data_range)^2, C2 = (K2 * data_range)^2 with data_range = 1: Python doubles, rounded to fp32 where they meet the fp32 maps
constexpr float kC1 = (float)(0.01 * 0.01), kC2 = (float)(0.03 * 0.03);

// torch's fp32 window, _fspecial_gauss_1d(11, 1.5): the values of ssim.hip's c_win
constexpr Window kWindow = {{0x1.0d9570p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f, 0x1.b43c3ep-3f,
                             0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d9570p-10f}};

constexpr int BW_TX = 32, BW_TY = 16, BW_THREADS = 256;             // backward: tile of the plane owned by one workgroup
constexpr int BW_MW = BW_TX + HALO, BW_MH = BW_TY + HALO;           // 42 x 26 valid-map positions that reach the tile
constexpr int BW_IW = BW_MW + HALO, BW_IH = BW_MH + HALO;           // 52 x 36 input pixels under them

struct LossGeom {
    Geom g;
    int bw_tiles_x[SCALES], bw_tiles[SCALES];
    long long off_coef, off_val, off_dy[SCALES];                    // u_s per plane (fp32 [planes][5]); 1 - V (fp64); dy_s, s = 1..4 (fp32)
    long long bytes;
};

// Workspace: [ssim_core::geometry's sections | u_s | 1 - V | dy_1 .. dy_4], each 256-byte aligned.
LossGeom loss_geometry(long long planes, int H, int W) {
    LossGeom L{};
    L.g = geometry(planes, H, W, true);
    long long b = L.g.bytes;
    L.off_coef = b;
    b = align256(b + planes * SCALES * (long long)sizeof(float));
    L.off_val = b;
    b = align256(b + planes * (long long)sizeof(double));
    for (int s = 0; s < SCALES; ++s) {
        L.bw_tiles_x[s] = dcvic_cdiv(L.g.W[s], BW_TX);
        L.bw_tiles[s] = L.bw_tiles_x[s] * dcvic_cdiv(L.g.H[s], BW_TY);
        if (s == 0) continue;
        L.off_dy[s] = b;
        b = align256(b + planes * L.g.H[s] * (long long)L.g.W[s] * (long long)sizeof(float));
    }
    L.bytes = b;
    return L;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per plane: lane l sums tiles l, l + 64, ... of every scale in order, then a fixed butterfly (msssim_finish_kernel's order).
__global__ __launch_bounds__(64) void msssim_loss_finish_kernel(const unsigned char* __restrict__ ws, Geom g, double scale, float* __restrict__ coef,
                                                                double* __restrict__ val, double* __restrict__ per_plane) {
    const long long pl = blockIdx.x;
    const int lane = threadIdx.x;
    double m[SCALES];
#pragma unroll
    for (int s = 0; s < SCALES; ++s) {
        const double* p = (const double*)(ws + g.off_part[s]) + pl * g.tiles[s] * 2 + (s == SCALES - 1 ? 1 : 0);
        double t = 0.0;
        for (int k = lane; k < g.tiles[s]; k += 64) t += p[(long long)k * 2];
        m[s] = wave_sum(t) / (double)g.count[s];
    }
    if (lane != 0) return;
    double v = 1.0;
#pragma unroll
    for (int s = 0; s < SCALES; ++s) v *= pow(fmax(m[s], 0.0), kWeights[s]);
    val[pl] = 1.0 - v;
    if (per_plane) per_plane[pl] = v;
#pragma unroll
    for (int s = 0; s < SCALES; ++s)                        // v > 0 only if every factor is > 0; a NaN stays a NaN
        coef[pl * SCALES + s] = v == 0.0 ? 0.f : (float)(-scale * kWeights[s] * v / m[s] / (double)g.count[s]);
}

__global__ __launch_bounds__(64) void msssim_loss_total_kernel(const double* __restrict__ val, long long planes, double scale, double* __restrict__ loss) {
    double t = 0.0;
    for (long long k = threadIdx.x; k < planes; k += 64) t += val[k];
    t = wave_sum(t);
    if (threadIdx.x == 0) loss[0] = scale * t;
}

// dy_s on one 32 x 16 tile of one plane (see the head of the file).  coef: u_s of plane 0 (stride SCALES per plane); dcoarse: dy_{s+1}
// [planes][Hc][Wc] or null at the last scale; out: dy_s [planes][H][W].
template <bool LAST>
__global__ __launch_bounds__(BW_THREADS) void msssim_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int Ho, int Wo,
                                                                 int tiles_x, Window win, float S, float e, const float* __restrict__ coef,
                                                                 const float* __restrict__ dcoarse, int Hc, int Wc, float* __restrict__ out) {
    __shared__ float sx[BW_IH][BW_IW], sy[BW_IH][BW_IW];
    __shared__ float hq[5][BW_IH][BW_MW];
    __shared__ float pm[3][BW_MH][BW_MW];
    static_assert(sizeof(float) * 3 * BW_MH * BW_TX <= sizeof(hq), "the adjoint's row pass reuses hq");
    float(*ah)[BW_MH][BW_TX] = reinterpret_cast<float(*)[BW_MH][BW_TX]>(&hq[0][0][0]);
    const long long pl = blockIdx.y;
    const int px0 = (blockIdx.x % tiles_x) * BW_TX, py0 = (blockIdx.x / tiles_x) * BW_TY;
    const int t = threadIdx.x;
    const int c = t % BW_TX, r0 = t / BW_TX;                 // this thread's output pixels: column c, rows r0, r0 + 8
    const float u = coef[pl * SCALES];
    const float* dc = dcoarse ? dcoarse + pl * Hc * Wc : nullptr;
    float* op = out + pl * H * W;
    const int px = px0 + c;
    if (u == 0.f) {                                          // a plane with V = 0 (or this scale's seed underflowed): the pool's adjoint only
        for (int r = r0; r < BW_TY; r += BW_THREADS / BW_TX) {
            const int py = py0 + r;
            if (py < H && px < W) op[(long long)py * W + px] = dc ? 0.25f * dc[(long long)((py + (H & 1)) >> 1) * Wc + ((px + (W & 1)) >> 1)] : 0.f;
        }
        return;
    }
    const float* xp = x + pl * H * W;
    const float* yp = y + pl * H * W;
    const long long ci = (long long)min(py0 + BW_TY / 2, H - 1) * W + min(px0 + BW_TX / 2, W - 1);
    const float sa = xp[ci], sb = yp[ci];
    for (int i = t; i < BW_IH * BW_IW; i += BW_THREADS) {
        const int r = i / BW_IW, cc = i % BW_IW;
        const int gy = py0 - HALO + r, gx = px0 - HALO + cc;
        float dx = 0.f, dy = 0.f;                            // outside the plane: feeds only positions outside the valid map
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long long o = (long long)gy * W + gx;
            dx = xp[o] - sa;
            dy = yp[o] - sb;
        }
        sx[r][cc] = dx;
        sy[r][cc] = dy;
    }
    __syncthreads();
    // row pass of the five moments G(dx), G(d), G(dx^2), G(dy^2), G(d^2) with d = dx - dy: 36 rows x 42 map columns
    for (int i = t; i < BW_IH * BW_MW; i += BW_THREADS) {
        const int r = i / BW_MW, j = i % BW_MW;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = win.g[k], a = sx[r][j + k], b = sy[r][j + k], d = a - b;
            m0 = fmaf(w, a, m0);
            m1 = fmaf(w, d, m1);
            m2 = fmaf(w, a * a, m2);
            m3 = fmaf(w, b * b, m3);
            m4 = fmaf(w, d * d, m4);
        }
        hq[0][r][j] = m0;
        hq[1][r][j] = m1;
        hq[2][r][j] = m2;
        hq[3][r][j] = m3;
        hq[4][r][j] = m4;
    }
    __syncthreads();
    // column pass, then B, A1, A2 at the 26 x 42 map positions (i, j) = valid-map pixel (py0 - 10 + i, px0 - 10 + j)
    const float sd = sa - sb;
    for (int idx = t; idx < BW_MH * BW_MW; idx += BW_THREADS) {
        const int i = idx / BW_MW, j = idx % BW_MW;
        const int qy = py0 - HALO + i, qx = px0 - HALO + j;
        float B = 0.f, A1 = 0.f, A2 = 0.f;
        if (qy >= 0 && qy < Ho && qx >= 0 && qx < Wo) {
            float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float w = win.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) a[q] = fmaf(w, hq[q][i + k][j], a[q]);
            }
            const float gx = a[0], gd = a[1], gy = gx - gd;
            const float sxx = cov(a[2], gx, gx, sa, sa, S, e);
            const float syy = cov(a[3], gy, gy, sb, sb, S, e);
            const float sdd = cov(a[4], gd, gd, sd, sd, S, e);
            const float D = sxx + syy + kC2;
            const float omc = sdd / D;                       // 1 - cs
            float lp = 1.f, Pl = 0.f;
            if (LAST) {
                const float mux = sa * S + gx, muy = sb * S + gy;
                const float den = mux * mux + muy * muy + kC1;
                lp = (2.f * mux * muy + kC1) / den;
                Pl = u * (1.f - omc) * (2.f * mux - 2.f * muy * lp) / den;
            }
            A1 = 2.f * (u * lp / D);
            A2 = A1 * omc;
            B = Pl - A1 * (gd - sd * e) - A2 * (gy - sb * e);
        }
        pm[0][i][j] = B;
        pm[1][i][j] = A1;
        pm[2][i][j] = A2;
    }
    __syncthreads();
    // the adjoint's row pass (the window is symmetric): 26 rows x 32 tile columns, into hq's storage
    for (int idx = t; idx < BW_MH * BW_TX; idx += BW_THREADS) {
        const int i = idx / BW_TX, cc = idx % BW_TX;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = win.g[k];
            a0 = fmaf(w, pm[0][i][cc + k], a0);
            a1 = fmaf(w, pm[1][i][cc + k], a1);
            a2 = fmaf(w, pm[2][i][cc + k], a2);
        }
        ah[0][i][cc] = a0;
        ah[1][i][cc] = a1;
        ah[2][i][cc] = a2;
    }
    __syncthreads();
    // the column pass, the local x(p), y(p), and the pool's adjoint of the coarser scale
    for (int r = r0; r < BW_TY; r += BW_THREADS / BW_TX) {
        const int py = py0 + r;
        if (py >= H || px >= W) continue;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = win.g[k];
            a0 = fmaf(w, ah[0][r + k][c], a0);
            a1 = fmaf(w, ah[1][r + k][c], a1);
            a2 = fmaf(w, ah[2][r + k][c], a2);
        }
        const float yv = sy[r + HALO][c + HALO];
        float d = a0 + (sx[r + HALO][c + HALO] - yv) * a1 + yv * a2;
        if (dc) d += 0.25f * dc[(long long)((py + (H & 1)) >> 1) * Wc + ((px + (W & 1)) >> 1)];
        op[(long long)py * W + px] = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------- absolute error
constexpr int AE_THREADS = 256, AE_PER_THREAD = 8, AE_MAX_BLOCKS = 64;

// workgroups per image: one per 2048 elements, at most 64; a larger image is walked by a grid stride
long long abs_err_blocks(long long M) {
    if (M <= 0) return 0;
    const long long b = (M + AE_THREADS * AE_PER_THREAD - 1) / (AE_THREADS * AE_PER_THREAD);
    return b < AE_MAX_BLOCKS ? b : AE_MAX_BLOCKS;
}

// workgroup (n, blk) of `per` per image: thread t takes the elements blk * 256 + t + k * per * 256, k ascending
__global__ __launch_bounds__(AE_THREADS) void abs_err_kernel(const float* __restrict__ a, const float* __restrict__ b, float scale, float* __restrict__ da,
                                                             double* __restrict__ part, long long M, int per) {
    __shared__ double red[AE_THREADS / 64];
    const int n = blockIdx.x / per, blk = blockIdx.x % per;
    const float* ap = a + (long long)n * M;
    const float* bp = b + (long long)n * M;
    float* dp = da ? da + (long long)n * M : nullptr;
    const long long stride = (long long)per * AE_THREADS;
    double s = 0.0;
    for (long long i = (long long)blk * AE_THREADS + threadIdx.x; i < M; i += stride) {
        const float x = ap[i], y = bp[i];
        s += fabs((double)x - (double)y);
        if (dp) dp[i] = x > y ? scale : (x < y ? -scale : (x - y) * 0.f);     // sign(0) = 0; a NaN stays a NaN
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave: image after image, lane l adds the image's partials l, l + 64, ..., a lane tree adds the 64 sums
__global__ __launch_bounds__(64) void abs_err_total_kernel(const double* __restrict__ part, int per, int N, double scale, double* __restrict__ loss) {
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        double s = 0.0;
        for (int i = threadIdx.x; i < per; i += 64) s += part[(long long)n * per + i];
        total += wave_sum(s);
    }
    if (threadIdx.x == 0) loss[0] = scale * total;
}

bool loss_sizes_ok(int N, int C, int H, int W) {
    return N > 0 && C > 0 && H >= MIN_SIDE && W >= MIN_SIDE && (long long)H * W <= 0x7fffffffLL && (long long)N * C <= MAX_GRID_Y;
}

}  // namespace

extern "C" long long dcvic_msssim_loss_workspace_bytes(int N, int C, int H, int W) {
    return loss_sizes_ok(N, C, H, W) ? loss_geometry((long long)N * C, H, W).bytes : 0;
}

extern "C" int dcvic_msssim_loss_f32(const float* real, const float* fake, int N, int C, int H, int W, double scale, double* loss, double* per_plane,
                                     float* dfake, void* workspace, long long workspace_bytes, void* stream) {
    DCVIC_CHECK_ARG(real && fake && loss && workspace, "msssim_loss: null pointer (real %p, fake %p, loss %p, workspace %p)", (const void*)real,
                    (const void*)fake, (void*)loss, workspace);
    DCVIC_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "msssim_loss: empty tensor N=%d C=%d H=%d W=%d", N, C, H, W);
    DCVIC_CHECK_ARG(H >= MIN_SIDE && W >= MIN_SIDE, "msssim_loss: MS-SSIM needs min(H, W) > 160, got %d x %d", H, W);
    DCVIC_CHECK_ARG((long long)H * W <= 0x7fffffffLL, "msssim_loss: plane of %d x %d too large", H, W);
    DCVIC_CHECK_ARG(scale - scale == 0.0, "msssim_loss: scale %g is not finite", scale);
    const long long planes = (long long)N * C;
    DCVIC_CHECK_ARG(planes <= MAX_GRID_Y, "msssim_loss: %lld planes, at most %lld in one call", planes, MAX_GRID_Y);
    const LossGeom L = loss_geometry(planes, H, W);
    const Geom& g = L.g;
    DCVIC_CHECK_ARG(workspace_bytes >= L.bytes, "msssim_loss: workspace of %lld bytes, need %lld", workspace_bytes, L.bytes);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    const Window win = kWindow;
    float S, e;
    window_sums(win, &S, &e);
    auto plane_x = [&](int s) { return s == 0 ? real : (const float*)(ws + g.off_img[s]); };
    auto plane_y = [&](int s) { return s == 0 ? fake : (const float*)(ws + g.off_img[s]) + planes * g.H[s] * g.W[s]; };
    for (int s = 0; s < SCALES; ++s) {
        if (s < SCALES - 1) {
            float* xn = (float*)(ws + g.off_img[s + 1]);
            msssim_pool_kernel<false><<<dim3((unsigned)g.pool_tiles[s], (unsigned)planes), PL_TX * PL_TY, 0, st>>>(
                plane_x(s), plane_y(s), g.H[s], g.W[s], g.H[s + 1], g.W[s + 1], g.pool_tiles_x[s], xn, xn + planes * g.H[s + 1] * g.W[s + 1], nullptr);
            DCVIC_CHECK_LAUNCH("msssim_loss_pool");
        }
        msssim_stats_kernel<false><<<dim3((unsigned)g.tiles[s], (unsigned)planes), ST_THREADS, 0, st>>>(
            plane_x(s), plane_y(s), g.H[s], g.W[s], g.H[s] - HALO, g.W[s] - HALO, g.tiles_x[s], win, S, e, kC1, kC2, (double*)(ws + g.off_part[s]));
        DCVIC_CHECK_LAUNCH("msssim_loss_stats");
    }
    float* coef = (float*)(ws + L.off_coef);
    double* val = (double*)(ws + L.off_val);
    msssim_loss_finish_kernel<<<(unsigned)planes, 64, 0, st>>>(ws, g, scale, coef, val, per_plane);
    DCVIC_CHECK_LAUNCH("msssim_loss_finish");
    msssim_loss_total_kernel<<<1, 64, 0, st>>>(val, planes, scale, loss);
    DCVIC_CHECK_LAUNCH("msssim_loss_total");
    if (!dfake) return DCVIC_OK;
    for (int s = SCALES - 1; s >= 0; --s) {
        const float* dc = s == SCALES - 1 ? nullptr : (const float*)(ws + L.off_dy[s + 1]);
        const int Hc = s == SCALES - 1 ? 0 : g.H[s + 1], Wc = s == SCALES - 1 ? 0 : g.W[s + 1];
        float* out = s == 0 ? dfake : (float*)(ws + L.off_dy[s]);
        const dim3 grid((unsigned)L.bw_tiles[s], (unsigned)planes);
        if (s == SCALES - 1)
            msssim_grad_kernel<true><<<grid, BW_THREADS, 0, st>>>(plane_x(s), plane_y(s), g.H[s], g.W[s], g.H[s] - HALO, g.W[s] - HALO, L.bw_tiles_x[s], win, S,
                                                                  e, coef + s, dc, Hc, Wc, out);
        else
            msssim_grad_kernel<false><<<grid, BW_THREADS, 0, st>>>(plane_x(s), plane_y(s), g.H[s], g.W[s], g.H[s] - HALO, g.W[s] - HALO, L.bw_tiles_x[s], win, S,
                                                                   e, coef + s, dc, Hc, Wc, out);
        DCVIC_CHECK_LAUNCH("msssim_loss_grad");
    }
    return DCVIC_OK;
}

extern "C" long long dcvic_abs_err_workspace_bytes(int N, long long n_per_image) {
    return N > 0 ? (long long)N * abs_err_blocks(n_per_image) * (long long)sizeof(double) : 0;
}

extern "C" int dcvic_abs_err_f32(const float* a, const float* b, long long n_per_image, int N, double scale, double* loss, float* da, void* workspace,
                                 long long workspace_bytes, void* stream) {
    DCVIC_CHECK_ARG(a && b && loss && workspace, "abs_err: null pointer (a %p, b %p, loss %p, workspace %p)", (const void*)a, (const void*)b, (void*)loss,
                    workspace);
    DCVIC_CHECK_ARG(N > 0 && n_per_image > 0, "abs_err: empty tensor N=%d n_per_image=%lld", N, n_per_image);
    DCVIC_CHECK_ARG(scale - scale == 0.0, "abs_err: scale %g is not finite", scale);
    const int per = (int)abs_err_blocks(n_per_image);
    DCVIC_CHECK_ARG((long long)N * per <= 0x3fffffff && n_per_image <= (1LL << 40), "abs_err: N=%d n_per_image=%lld too large", N, n_per_image);
    const long long need = dcvic_abs_err_workspace_bytes(N, n_per_image);
    DCVIC_CHECK_ARG(workspace_bytes >= need, "abs_err: workspace of %lld bytes, need %lld", workspace_bytes, need);
    abs_err_kernel<<<(unsigned)(N * per), AE_THREADS, 0, (hipStream_t)stream>>>(a, b, (float)scale, da, (double*)workspace, n_per_image, per);
    DCVIC_CHECK_LAUNCH("abs_err");
    abs_err_total_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const double*)workspace, per, N, scale, loss);
    DCVIC_CHECK_LAUNCH("abs_err_total");
    return DCVIC_OK;
}
