// rate_train.hip -- the differentiable rate term: the training-mode (additive uniform noise) forward of the two entropy models and
// the gradients of the rate loss, restated from CompressAI 1.2.4 (the reference drives them from
// ste_gaussian_conditional.py:16-23 and entropy_bottleneck.py:19-28), and EntropyBottleneck.loss().  include/dcvic_rate.h states
// the formulae; this file follows rate.hip and chan_ce.hip: fp32 data, fp64 sums in a fixed order, no atomics, no output that
// depends on what a buffer held before (bits, loss and the parameter gradients ACCUMULATE by contract).
//
// The value path is written with explicit roundings (__fmul_rn / __fsub_rn / fmaf) and is the same code whether or not gradients
// are requested, so the bits of lik / bits / loss cannot depend on the gradient outputs.
//
// dcvic_gaussian_rate_train_f32: rate.hip's decomposition -- block b of image n owns the span [b*span, (b+1)*span) of C*HW, fp64
//   partials per block, a finishing kernel adds them in ascending order.  One pass: value and gradients from the same registers.
// dcvic_eb_rate_train_f32: one workgroup per channel, lanes over the flat (n, hw) index.  The channel's 58 parameters
//   (softplus / tanh applied here) sit in LDS; a lane runs the 5-layer cumulative forward twice (zt -/+ 0.5), then its reverse
//   pass, and keeps the 58 parameter gradients as fp64 accumulators; a shuffle tree and a 4-wave LDS pass add them in a fixed
//   order, the chain factors of softplus / tanh are applied once per channel, and the sums are += into the caller's buffers.
//   ln p per element goes to the workspace; a span kernel and the finishing kernel form bits[n] exactly as above (an order that
//   depends on C*HW only, channels ascending).
#include "common.h"
#include "dcvic_rate.h"

namespace {

constexpr float LIK_BOUND = 1e-9f, SCALE_BOUND = 0.11f;
constexpr double LN2 = 0.693147180559945309417;
constexpr float INV_LN2 = 1.44269504088896340736f, INV_SQRT_2PI = 0.39894228040143267794f;

__device__ __forceinline__ double block_sum4_d(double v, double* red) {      // 256 threads
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float std_cumulative(float x) { return __fmul_rn(0.5f, erfcf(__fmul_rn(-0.70710678118654752440f, x))); }
__device__ __forceinline__ float std_density(float x) { return INV_SQRT_2PI * expf(-0.5f * x * x); }

// ------------------------------------------------------------------------------------------------ Gaussian conditional
struct GrOut { float yh, p, dy, ds; };

// gw = scale * w[n]
__device__ __forceinline__ float gr_train_element(float y, float m, float sg, float u, float gw, bool want_grad, GrOut& o) {
    o.yh = __fadd_rn(rintf(__fsub_rn(y, m)), m);
    const float d = __fsub_rn(__fadd_rn(y, u), m);
    const float v = fabsf(d);
    const float s = fmaxf(sg, SCALE_BOUND);
    const float a = __fsub_rn(0.5f, v) / s, b = __fsub_rn(-0.5f, v) / s;
    const float p_raw = __fsub_rn(std_cumulative(a), std_cumulative(b));
    o.p = fmaxf(p_raw, LIK_BOUND);
    o.dy = 0.f;
    o.ds = 0.f;
    if (want_grad) {
        const float g_p = -gw * INV_LN2 / o.p;
        const float g_raw = (p_raw >= LIK_BOUND || g_p < 0.f) ? g_p : 0.f;       // LowerBound backward, likelihood bound
        const float fa = std_density(a), fb = std_density(b);
        const float sign = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        o.dy = g_raw * (-sign * (fa - fb) / s);
        const float g_s = g_raw * (-(a * fa - b * fb) / s);
        o.ds = (sg >= SCALE_BOUND || g_s < 0.f) ? g_s : 0.f;                     // LowerBound backward, scale bound
    }
    return logf(o.p);
}

struct GrArgs {
    const float *y, *mu, *sigma, *noise, *w;
    float *y_hat, *lik, *dy, *dmu, *dsigma;
    long long y_bs, ms_bs, noise_bs, yh_bs, lik_bs, dy_bs, dms_bs, CHW;
    double* partial;
    float scale;
};

// VEC: every stream is 16-B aligned and the block spans are multiples of 4 -> float4 accesses, four elements per lane and iteration
template <bool VEC>
__global__ __launch_bounds__(256) void gaussian_rate_train_kernel(GrArgs A) {
    __shared__ double red[4];
    const int n = blockIdx.y;
    const long long CHW = A.CHW;
    long long span = (CHW + gridDim.x - 1) / gridDim.x;
    if (VEC) span = (span + 3) & ~3ll;
    const long long i_end = min(CHW, (long long)(blockIdx.x + 1) * span);
    const float gw = A.scale * (A.w ? A.w[n] : 1.f);
    const bool want_grad = A.dy || A.dmu || A.dsigma;
    double acc = 0.0;
    constexpr int V = VEC ? 4 : 1;
    for (long long i = (long long)blockIdx.x * span + V * threadIdx.x; i < i_end; i += V * blockDim.x) {
        alignas(16) float y[V], m[V], sg[V], u[V], yh[V], p[V], dy[V], dm[V], ds[V];
        if (VEC) {
            *reinterpret_cast<float4*>(y) = *reinterpret_cast<const float4*>(A.y + n * A.y_bs + i);
            *reinterpret_cast<float4*>(m) = *reinterpret_cast<const float4*>(A.mu + n * A.ms_bs + i);
            *reinterpret_cast<float4*>(sg) = *reinterpret_cast<const float4*>(A.sigma + n * A.ms_bs + i);
            *reinterpret_cast<float4*>(u) = *reinterpret_cast<const float4*>(A.noise + n * A.noise_bs + i);
        } else {
            y[0] = A.y[n * A.y_bs + i];
            m[0] = A.mu[n * A.ms_bs + i];
            sg[0] = A.sigma[n * A.ms_bs + i];
            u[0] = A.noise[n * A.noise_bs + i];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            GrOut o;
            acc += (double)gr_train_element(y[j], m[j], sg[j], u[j], gw, want_grad, o);
            yh[j] = o.yh, p[j] = o.p, dy[j] = o.dy, dm[j] = -o.dy, ds[j] = o.ds;
        }
        if (VEC) {
            if (A.y_hat) *reinterpret_cast<float4*>(A.y_hat + n * A.yh_bs + i) = *reinterpret_cast<float4*>(yh);
            if (A.lik) *reinterpret_cast<float4*>(A.lik + n * A.lik_bs + i) = *reinterpret_cast<float4*>(p);
            if (A.dy) *reinterpret_cast<float4*>(A.dy + n * A.dy_bs + i) = *reinterpret_cast<float4*>(dy);
            if (A.dmu) *reinterpret_cast<float4*>(A.dmu + n * A.dms_bs + i) = *reinterpret_cast<float4*>(dm);
            if (A.dsigma) *reinterpret_cast<float4*>(A.dsigma + n * A.dms_bs + i) = *reinterpret_cast<float4*>(ds);
        } else {
            if (A.y_hat) A.y_hat[n * A.yh_bs + i] = yh[0];
            if (A.lik) A.lik[n * A.lik_bs + i] = p[0];
            if (A.dy) A.dy[n * A.dy_bs + i] = dy[0];
            if (A.dmu) A.dmu[n * A.dms_bs + i] = dm[0];
            if (A.dsigma) A.dsigma[n * A.dms_bs + i] = ds[0];
        }
    }
    if (A.partial) {
        const double t = block_sum4_d(acc, red);
        if (threadIdx.x == 0) A.partial[(long long)n * gridDim.x + blockIdx.x] = t;
    }
}

// One workgroup of N threads (N <= 1024): b[n] = -(the image's block partials, ascending) / ln 2; bits[n] += b[n];
// loss[0] += sum_n scale * w[n] * b[n], n ascending
__global__ void rate_train_finish_kernel(const double* __restrict__ partial, int nb, const float* __restrict__ w, double scale,
                                         float* __restrict__ bits, float* __restrict__ loss) {
    __shared__ double term[1024];
    const int n = threadIdx.x;
    double t = 0.0;
    for (int b = 0; b < nb; ++b) t += partial[(long long)n * nb + b];
    const double bn = -t / LN2;
    if (bits) bits[n] += (float)bn;
    if (loss) {
        term[n] = scale * (w ? (double)w[n] : 1.0) * bn;
        __syncthreads();
        if (n == 0) {
            double s = 0.0;
            for (int i = 0; i < (int)blockDim.x; ++i) s += term[i];
            loss[0] += (float)s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entropy bottleneck
// Parameter slot k of a channel, in the pack order of rate.hip: matrices [0, 33) = m0 (3x1), m1..m3 (3x3 row-major), m4 (1x3);
// biases [33, 46) = b0..b3 (3), b4 (1); factors [46, 58) = f0..f3 (3).
constexpr int NPAR = 58, OFF_B = 33, OFF_F = 46;

struct EbPtrs { const float* t[14]; };      // matrix0..4, bias0..4, factor0..3
struct EbGradPtrs { float* t[14]; };

__host__ __device__ constexpr int eb_width(int t) { return t == 0 ? 3 : t < 4 ? 9 : t == 4 ? 3 : t < 9 ? 3 : t == 9 ? 1 : 3; }
__host__ __device__ constexpr int eb_base(int t) {
    return t == 0 ? 0 : t < 5 ? 3 + 9 * (t - 1) : t < 10 ? OFF_B + 3 * (t - 5) : OFF_F + 3 * (t - 10);
}

// the raw value of slot k (every tensor index is a constant after unrolling: no dynamically indexed kernel argument)
__device__ __forceinline__ float eb_raw(const EbPtrs& P, int c, int k) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < 14; ++t)
        if (k >= eb_base(t) && k < eb_base(t) + eb_width(t)) v = P.t[t][(long long)c * eb_width(t) + (k - eb_base(t))];
    return v;
}

__device__ __forceinline__ void eb_grad_add(const EbGradPtrs& G, int c, int k, float g) {
#pragma unroll
    for (int t = 0; t < 14; ++t)
        if (k >= eb_base(t) && k < eb_base(t) + eb_width(t)) G.t[t][(long long)c * eb_width(t) + (k - eb_base(t))] += g;
}

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }       // torch's threshold 20
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// slot k as the forward uses it: softplus(matrix), bias, tanh(factor)
__device__ __forceinline__ float eb_effective(float raw, int k) { return k < OFF_B ? softplus_f(raw) : (k < OFF_F ? raw : tanhf(raw)); }
// d effective / d raw
__device__ __forceinline__ float eb_chain(float raw, int k) {
    if (k < OFF_B) return raw > 20.f ? 1.f : sigmoid_f(raw);
    if (k < OFF_F) return 1.f;
    const float t = tanhf(raw);
    return 1.f - t * t;
}

// the cumulative's forward with every rounding explicit; h[l] = the layer's output, th[l] = tanh of its pre-activation
__device__ __forceinline__ float eb_forward(float x, const float* P, float h[4][3], float th[4][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = fmaf(P[r], x, P[OFF_B + r]);
        th[0][r] = tanhf(a);
        h[0][r] = fmaf(P[OFF_F + r], th[0][r], a);
    }
#pragma unroll
    for (int l = 1; l < 4; ++l) {
        const float* m = P + 3 + (l - 1) * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float a = fmaf(m[r * 3 + 2], h[l - 1][2], fmaf(m[r * 3 + 1], h[l - 1][1], fmaf(m[r * 3], h[l - 1][0], P[OFF_B + l * 3 + r])));
            th[l][r] = tanhf(a);
            h[l][r] = fmaf(P[OFF_F + l * 3 + r], th[l][r], a);
        }
    }
    return fmaf(P[32], h[3][2], fmaf(P[31], h[3][1], fmaf(P[30], h[3][0], P[OFF_B + 12])));
}

// reverse pass of eb_forward for d loss / d logit = g: returns d loss / d x; with PG adds the gradients w.r.t. the 58 effective
// parameters to acc
template <bool PG>
__device__ __forceinline__ float eb_reverse(float x, float g, const float* P, const float h[4][3], const float th[4][3], double* acc) {
    float gh[3], ga[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gh[j] = g * P[30 + j];
        if (PG) acc[30 + j] += (double)(g * h[3][j]);
    }
    if (PG) acc[OFF_B + 12] += (double)g;
#pragma unroll
    for (int l = 3; l >= 1; --l) {
        const float* m = P + 3 + (l - 1) * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float t = th[l][r];
            ga[r] = gh[r] * fmaf(P[OFF_F + l * 3 + r], 1.f - t * t, 1.f);
            if (PG) {
                acc[OFF_F + l * 3 + r] += (double)(gh[r] * t);
                acc[OFF_B + l * 3 + r] += (double)ga[r];
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[3 + (l - 1) * 9 + r * 3 + j] += (double)(ga[r] * h[l - 1][j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) gh[j] = ga[0] * m[j] + ga[1] * m[3 + j] + ga[2] * m[6 + j];
    }
    float gx = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float t = th[0][r];
        const float a = gh[r] * fmaf(P[OFF_F + r], 1.f - t * t, 1.f);
        if (PG) {
            acc[OFF_F + r] += (double)(gh[r] * t);
            acc[OFF_B + r] += (double)a;
            acc[r] += (double)(a * x);
        }
        gx += a * P[r];
    }
    return gx;
}

__global__ __launch_bounds__(256) void eb_rate_train_kernel(const float* __restrict__ z, const float* __restrict__ noise, EbPtrs raw,
                                                            const float* __restrict__ medians, int med_stride,
                                                            const float* __restrict__ w, float scale, float* __restrict__ z_hat,
                                                            float* __restrict__ lik, float* __restrict__ dz, EbGradPtrs grads,
                                                            int want_pg, double* __restrict__ lnp, int N, int C, int HW) {
    __shared__ float P[NPAR];
    __shared__ double red[4][NPAR];
    const int c = blockIdx.x;
    if (threadIdx.x < NPAR) P[threadIdx.x] = eb_effective(eb_raw(raw, c, threadIdx.x), threadIdx.x);
    __syncthreads();
    const float med = medians[(long long)c * med_stride];
    const long long CHW = (long long)C * HW, M = (long long)N * HW;
    const bool want_grad = dz || want_pg;
    double acc[NPAR];
#pragma unroll
    for (int k = 0; k < NPAR; ++k) acc[k] = 0.0;
    for (long long i = threadIdx.x; i < M; i += blockDim.x) {
        const int n = (int)(i / HW);
        const long long idx = n * CHW + (long long)c * HW + (i - (long long)n * HW);
        const float zv = z[idx];
        if (z_hat) z_hat[idx] = __fadd_rn(rintf(__fsub_rn(zv, med)), med);
        const float zt = __fadd_rn(zv, noise[idx]);
        const float xl = __fsub_rn(zt, 0.5f), xu = __fadd_rn(zt, 0.5f);
        float hl[4][3], tl[4][3], hu[4][3], tu[4][3];
        const float lower = eb_forward(xl, P, hl, tl), upper = eb_forward(xu, P, hu, tu);
        const float t = __fadd_rn(lower, upper);
        const float sg = t > 0.f ? -1.f : (t < 0.f ? 1.f : 0.f);
        const float su = 1.f / __fadd_rn(1.f, expf(-sg * upper)), sl = 1.f / __fadd_rn(1.f, expf(-sg * lower));
        const float D = __fsub_rn(su, sl);
        const float p_raw = fabsf(D), p = fmaxf(p_raw, LIK_BOUND);
        if (lik) lik[idx] = p;
        if (lnp) lnp[idx] = (double)logf(p);
        if (want_grad) {
            const float g_p = -(scale * (w ? w[n] : 1.f)) * INV_LN2 / p;
            const float g_raw = (p_raw >= LIK_BOUND || g_p < 0.f) ? g_p : 0.f;       // LowerBound backward
            const float g_D = g_raw * (D > 0.f ? 1.f : (D < 0.f ? -1.f : 0.f));
            const float g_u = g_D * sg * su * (1.f - su), g_l = -g_D * sg * sl * (1.f - sl);
            float gz;
            if (want_pg) gz = eb_reverse<true>(xu, g_u, P, hu, tu, acc) + eb_reverse<true>(xl, g_l, P, hl, tl, acc);
            else gz = eb_reverse<false>(xu, g_u, P, hu, tu, acc) + eb_reverse<false>(xl, g_l, P, hl, tl, acc);
            if (dz) dz[idx] = gz;
        }
    }
    if (want_pg) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < NPAR; ++k) {
            double v = acc[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) red[wv][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < NPAR) {
            const int k = threadIdx.x;
            const double s = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
            eb_grad_add(grads, c, k, (float)(s * (double)eb_chain(eb_raw(raw, c, k), k)));
        }
    }
}

// block b of image n adds its span of the per-element ln p (doubles, [N][C*HW]) in a fixed order
__global__ __launch_bounds__(256) void lnp_partial_kernel(const double* __restrict__ lnp, double* __restrict__ partial, long long CHW) {
    __shared__ double red[4];
    const int n = blockIdx.y;
    const long long span = (CHW + gridDim.x - 1) / gridDim.x;
    const long long i_end = min(CHW, (long long)(blockIdx.x + 1) * span);
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * span + threadIdx.x; i < i_end; i += blockDim.x) acc += lnp[n * CHW + i];
    const double t = block_sum4_d(acc, red);
    if (threadIdx.x == 0) partial[(long long)n * gridDim.x + blockIdx.x] = t;
}

// ------------------------------------------------------------------------------------------------ auxiliary loss
// one workgroup; item (c, k) = quantile k of channel c: forward-mode derivative of the cumulative beside its value
__global__ __launch_bounds__(256) void eb_aux_loss_kernel(EbPtrs raw, const float* __restrict__ quantiles, const float* __restrict__ target,
                                                          float* __restrict__ aux, float* __restrict__ dq, int accumulate, int C) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) {
        const int c = i / 3, k = i - 3 * c;
        float P[NPAR];
#pragma unroll
        for (int s = 0; s < NPAR; ++s) P[s] = eb_effective(eb_raw(raw, c, s), s);
        const float x = quantiles[i];
        float h[4][3], th[4][3];
        const float logit = eb_forward(x, P, h, th);
        const float diff = logit - target[k];
        acc += (double)fabsf(diff);
        if (dq) {
            const float g = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
            const float gx = eb_reverse<false>(x, g, P, h, th, nullptr);
            dq[i] = accumulate ? dq[i] + gx : gx;
        }
    }
    const double t = block_sum4_d(acc, red);
    if (aux && threadIdx.x == 0) aux[0] = (float)t;
}

bool eb_ptrs(const dcvic_eb_params* p, EbPtrs& out) {
    if (!p) return false;
    for (int i = 0; i < 5; ++i) out.t[i] = p->matrix[i], out.t[5 + i] = p->bias[i];
    for (int i = 0; i < 4; ++i) out.t[10 + i] = p->factor[i];
    for (int i = 0; i < 14; ++i)
        if (!out.t[i]) return false;
    return true;
}

}  // namespace

extern "C" int dcvic_gaussian_rate_train_f32(const float* y, long long y_bs, const float* mu, const float* sigma, long long ms_bs,
                                             const float* noise, long long noise_bs, const float* sample_weight, double scale,
                                             float* y_hat, long long yh_bs, float* lik, long long lik_bs, float* bits, float* loss,
                                             float* dy, long long dy_bs, float* dmu, float* dsigma, long long dms_bs,
                                             double* workspace, int N, int C, int HW, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && C > 0 && HW > 0, "dcvic_gaussian_rate_train_f32: empty tensor N=%d C=%d HW=%d", N, C, HW);
    DCVIC_CHECK_ARG(y && mu && sigma && noise, "dcvic_gaussian_rate_train_f32: null pointer (y %p, mu %p, sigma %p, noise %p)", (const void*)y,
                    (const void*)mu, (const void*)sigma, (const void*)noise);
    DCVIC_CHECK_ARG(y_hat || lik || bits || loss || dy || dmu || dsigma, "dcvic_gaussian_rate_train_f32: no output requested");
    const long long CHW = (long long)C * HW;
    DCVIC_CHECK_ARG(y_bs >= CHW && ms_bs >= CHW && noise_bs >= CHW && (!y_hat || yh_bs >= CHW) && (!lik || lik_bs >= CHW) &&
                        (!dy || dy_bs >= CHW) && (!(dmu || dsigma) || dms_bs >= CHW),
                    "dcvic_gaussian_rate_train_f32: batch stride too small (below C*HW = %lld)", CHW);
    const bool sums = bits || loss;
    DCVIC_CHECK_ARG(N <= 65535 && (!sums || N <= 1024), "dcvic_gaussian_rate_train_f32: batch too large, N=%d (bits / loss: <= 1024 images per call)", N);
    DCVIC_CHECK_ARG(!sums || workspace, "dcvic_gaussian_rate_train_f32: bits / loss need a workspace of N * dcvic_rate_blocks(C*HW) doubles");
    const int nb = dcvic_rate_blocks(CHW);
    GrArgs A;
    A.y = y, A.mu = mu, A.sigma = sigma, A.noise = noise, A.w = sample_weight;
    A.y_hat = y_hat, A.lik = lik, A.dy = dy, A.dmu = dmu, A.dsigma = dsigma;
    A.y_bs = y_bs, A.ms_bs = ms_bs, A.noise_bs = noise_bs, A.yh_bs = yh_bs, A.lik_bs = lik_bs, A.dy_bs = dy_bs, A.dms_bs = dms_bs, A.CHW = CHW;
    A.partial = sums ? workspace : nullptr;
    A.scale = (float)scale;
    auto al16 = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    auto m4 = [](const void* p, long long bs) { return p == nullptr || (bs & 3) == 0; };
    // NOTE chosen from CHW, strides and alignment only (never N): the reduction order of bits[n] is the same for every batch size
    const bool vec = (CHW & 3) == 0 && ((y_bs | ms_bs | noise_bs) & 3) == 0 && m4(y_hat, yh_bs) && m4(lik, lik_bs) && m4(dy, dy_bs) &&
                     m4(dmu, dms_bs) && m4(dsigma, dms_bs) && al16(y) && al16(mu) && al16(sigma) && al16(noise) && al16(y_hat) && al16(lik) &&
                     al16(dy) && al16(dmu) && al16(dsigma);
    dim3 grid(nb, N);
    if (vec) gaussian_rate_train_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(A);
    else gaussian_rate_train_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(A);
    DCVIC_CHECK_LAUNCH("dcvic_gaussian_rate_train_f32");
    if (sums) {
        rate_train_finish_kernel<<<1, N, 0, (hipStream_t)stream>>>(workspace, nb, sample_weight, scale, bits, loss);
        DCVIC_CHECK_LAUNCH("dcvic_gaussian_rate_train_f32: finish");
    }
    return DCVIC_OK;
}

extern "C" long long dcvic_eb_rate_train_workspace_doubles(int N, int C, int HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    const long long CHW = (long long)C * HW;
    return (long long)N * CHW + (long long)N * dcvic_rate_blocks(CHW);
}

extern "C" int dcvic_eb_rate_train_f32(const float* z, const float* noise, const dcvic_eb_params* params, const float* medians, int med_stride,
                                       const float* sample_weight, double scale, float* z_hat, float* lik, float* bits, float* loss,
                                       float* dz, const dcvic_eb_grads* grads, double* workspace, int N, int C, int HW, void* stream) {
    DCVIC_CHECK_ARG(N > 0 && C > 0 && HW > 0, "dcvic_eb_rate_train_f32: empty tensor N=%d C=%d HW=%d", N, C, HW);
    EbPtrs raw;
    DCVIC_CHECK_ARG(z && noise && medians && eb_ptrs(params, raw), "dcvic_eb_rate_train_f32: null pointer (z %p, noise %p, medians %p, params %p or one of its 14)",
                    (const void*)z, (const void*)noise, (const void*)medians, (const void*)params);
    DCVIC_CHECK_ARG(med_stride > 0, "dcvic_eb_rate_train_f32: med_stride=%d", med_stride);
    EbGradPtrs G;
    for (int i = 0; i < 14; ++i) G.t[i] = nullptr;
    if (grads) {
        for (int i = 0; i < 5; ++i) G.t[i] = grads->matrix[i], G.t[5 + i] = grads->bias[i];
        for (int i = 0; i < 4; ++i) G.t[10 + i] = grads->factor[i];
        for (int i = 0; i < 14; ++i) DCVIC_CHECK_ARG(G.t[i], "dcvic_eb_rate_train_f32: null pointer in grads (tensor %d of 14)", i);
    }
    DCVIC_CHECK_ARG(z_hat || lik || bits || loss || dz || grads, "dcvic_eb_rate_train_f32: no output requested");
    const bool sums = bits || loss;
    DCVIC_CHECK_ARG(C <= 0x7fffffff / 9 && (!sums || N <= 1024), "dcvic_eb_rate_train_f32: too large, N=%d C=%d (bits / loss: <= 1024 images per call)", N, C);
    DCVIC_CHECK_ARG(!sums || workspace, "dcvic_eb_rate_train_f32: bits / loss need a workspace of dcvic_eb_rate_train_workspace_doubles(N, C, HW) doubles");
    const long long CHW = (long long)C * HW;
    eb_rate_train_kernel<<<C, 256, 0, (hipStream_t)stream>>>(z, noise, raw, medians, med_stride, sample_weight, (float)scale, z_hat, lik, dz, G,
                                                            grads ? 1 : 0, sums ? workspace : nullptr, N, C, HW);
    DCVIC_CHECK_LAUNCH("dcvic_eb_rate_train_f32");
    if (sums) {
        const int nb = dcvic_rate_blocks(CHW);
        double* partial = workspace + (long long)N * CHW;
        lnp_partial_kernel<<<dim3(nb, N), 256, 0, (hipStream_t)stream>>>(workspace, partial, CHW);
        DCVIC_CHECK_LAUNCH("dcvic_eb_rate_train_f32: partial");
        rate_train_finish_kernel<<<1, N, 0, (hipStream_t)stream>>>(partial, nb, sample_weight, scale, bits, loss);
        DCVIC_CHECK_LAUNCH("dcvic_eb_rate_train_f32: finish");
    }
    return DCVIC_OK;
}

extern "C" int dcvic_eb_aux_loss_f32(const dcvic_eb_params* params, const float* quantiles, const float* target, float* aux, float* dquantiles,
                                     int accumulate, int C, void* stream) {
    DCVIC_CHECK_ARG(C > 0 && C <= 0x7fffffff / 9, "dcvic_eb_aux_loss_f32: C=%d", C);
    EbPtrs raw;
    DCVIC_CHECK_ARG(quantiles && target && eb_ptrs(params, raw), "dcvic_eb_aux_loss_f32: null pointer (quantiles %p, target %p, params %p or one of its 14)",
                    (const void*)quantiles, (const void*)target, (const void*)params);
    DCVIC_CHECK_ARG(aux || dquantiles, "dcvic_eb_aux_loss_f32: no output requested");
    eb_aux_loss_kernel<<<1, 256, 0, (hipStream_t)stream>>>(raw, quantiles, target, aux, dquantiles, accumulate ? 1 : 0, C);
    DCVIC_CHECK_LAUNCH("dcvic_eb_aux_loss_f32");
    return DCVIC_OK;
}
