// bn_train.hip -- per-channel batch statistics over (N, H, W) with their backward (include/dcvic_bn.h): torch.nn.BatchNorm2d in
// training mode and taming's ActNorm (reference: taming/modules/util.py:10-69), the normalisation layers of the GAN discriminators
// (src/models/discriminator/taming_nlayer_discriminator.py:11-26 `get_norm_layer`).
//
// Layout of the work.  Tensors are [N][C][HW] with a batch stride each.  A plane (n, c) is cut into S = ceil(HW / CHUNK) chunks of
// CHUNK = 4096 values; workgroup (c * S + s, n) of 256 threads owns one chunk.  Thread t owns the values 4 t .. 4 t + 3 of every
// 1024-value step of its chunk, ascending: one 16-byte load where the plane bases are 16-byte aligned (HW and every batch stride a
// multiple of 4), four 4-byte loads of the SAME values otherwise -- so which thread adds what, and in which order, depends on
// (N, C, HW) alone, not on the strides.  All three kinds of pass use this one assignment:
//   sum pass      two fp64 sums per thread (x and x^2; or g' and g' * u), a lane tree per wave, the four waves added in order, one
//                 pair of doubles per workgroup into the workspace at [(c * N + n) * S + s];
//   final pass    one wave per channel: lane i adds the channel's N * S partial pairs i, i + 64, ... in ascending order, a lane tree
//                 adds the 64; lane 0 forms mean / rstd / the running statistics (forward) or the parameter gradients and the three
//                 per-channel factors of dx (backward);
//   apply pass    elementwise, y = act(((x + p0) * p1) * a + b) or dx = k1 * (g' - k2 - u * k3).
// BatchNorm is p0 = -mean, p1 = rstd, a = gamma, b = beta; ActNorm is p0 = loc, p1 = 1, a = scale, b = 0: u = (x + p0) * p1 is xhat
// for the one and x + loc for the other, and the two share every kernel.  No atomics, nothing read before it is written.
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "dcvic_bn.h"

namespace {

constexpr int THREADS = 256, CHUNK = 4096, STEP = THREADS * 4;
static_assert(CHUNK % STEP == 0, "a chunk is a whole number of steps");

__device__ __forceinline__ double wsum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the values i .. i + 3 of a plane of HW values (i a multiple of 4, i < HW); past the plane's end: 0, never read
template <bool VEC>
__device__ __forceinline__ void load4(const float* p, int i, int HW, float (&v)[4]) {
    if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < HW ? p[i + j] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, int i, int HW, const float (&v)[4]) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < HW) p[i + j] = v[j];
    }
}

__device__ __forceinline__ float act_grad(float g, float y, int act) { return act == DCVIC_ACT_LRELU02 ? (y > 0.f ? g : 0.2f * g) : g; }

// the per-channel pair (p0, p1) of u = (x + p0) * p1
struct Shift {
    const float* shift;     // save_mean (neg) or loc
    const float* mul;       // save_rstd, or null: 1
    int neg;
    __device__ __forceinline__ void get(int c, float& p0, float& p1) const {
        p0 = neg ? -shift[c] : shift[c];
        p1 = mul ? mul[c] : 1.f;
    }
};

// BWD false: the sums of x and x^2.  BWD true: of g' and g' * u.
template <bool VEC, bool BWD>
__global__ __launch_bounds__(THREADS) void bn_sum_kernel(const float* x, long long x_bs, const float* g, long long g_bs, const float* y,
                                                         long long y_bs, Shift sh, int act, double* __restrict__ part, int N, int HW,
                                                         int S) {
    __shared__ double red[2][THREADS / 64];
    const int c = blockIdx.x / S, s = blockIdx.x % S, n = blockIdx.y;
    const long long po = (long long)c * HW;
    const float* xp = x + (long long)n * x_bs + po;
    const float* gp = BWD ? g + (long long)n * g_bs + po : nullptr;
    const float* yp = BWD && act != DCVIC_ACT_NONE ? y + (long long)n * y_bs + po : nullptr;
    float p0 = 0.f, p1 = 1.f;
    if constexpr (BWD) sh.get(c, p0, p1);
    const int lo = s * CHUNK, hi = min(HW, lo + CHUNK);
    double a = 0.0, b = 0.0;
    for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += STEP) {
        float xv[4], gv[4], yv[4];
        load4<VEC>(xp, i, HW, xv);
        if constexpr (BWD) {
            load4<VEC>(gp, i, HW, gv);
            if (yp) load4<VEC>(yp, i, HW, yv);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (VEC || i + j < HW) {
                if constexpr (BWD) {
                    const float gg = yp ? act_grad(gv[j], yv[j], act) : gv[j];
                    const float u = (xv[j] + p0) * p1;
                    a += (double)gg;
                    b = fma((double)gg, (double)u, b);
                } else {
                    const double xd = (double)xv[j];
                    a += xd;
                    b = fma(xd, xd, b);
                }
            }
        }
    }
    a = wsum_d(a);
    b = wsum_d(b);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = a, red[1][threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = part + 2 * (((long long)c * N + n) * S + s);
        dst[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        dst[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// one wave per channel: the channel's P partial pairs, lane i the pairs i, i + 64, ... ascending, then the lane tree
__device__ __forceinline__ void channel_sums(const double* __restrict__ part, int c, int P, double& a, double& b) {
    const double* pc = part + 2 * (long long)c * P;
    a = 0.0, b = 0.0;
    for (int i = threadIdx.x & 63; i < P; i += 64) a += pc[2 * (long long)i], b += pc[2 * (long long)i + 1];
    a = wsum_d(a);
    b = wsum_d(b);
}

// std_out given: the statistics-only form (mean_out, unbiased std).  Else save_mean / save_rstd and, when given, the running pair.
__global__ __launch_bounds__(THREADS) void bn_fwd_final_kernel(const double* __restrict__ part, int P, double M, int C, double eps, double momentum,
                                                               float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                               float* __restrict__ std_out, float* __restrict__ rmean, float* __restrict__ rvar) {
    const int c = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (c >= C) return;
    double s1, s2;
    channel_sums(part, c, P, s1, s2);
    if ((threadIdx.x & 63) != 0) return;
    const double mean = s1 / M;
    double var = s2 / M - mean * mean;
    var = var > 0.0 ? var : (var == var ? 0.0 : var);        // clamped at 0; a NaN stays one
    const double unbiased = var * (M / (M - 1.0));
    mean_out[c] = (float)mean;
    if (std_out) {
        std_out[c] = (float)sqrt(unbiased);
        return;
    }
    rstd_out[c] = (float)(1.0 / sqrt(var + eps));
    if (rmean) {
        rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
        rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * unbiased);
    }
}

// dmul[c] (+)= sum g' u, dadd[c] (+)= fac[c] * sum g' (fac: ActNorm's scale; null: 1); coef (BatchNorm only): [3][C] = gamma * rstd,
// sum g' / M, sum g' u / M
__global__ __launch_bounds__(THREADS) void bn_bwd_final_kernel(const double* __restrict__ part, int P, double M, int C, const float* __restrict__ gamma,
                                                               const float* __restrict__ rstd, const float* __restrict__ fac,
                                                               float* __restrict__ dmul, float* __restrict__ dadd, int accumulate,
                                                               float* __restrict__ coef) {
    const int c = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (c >= C) return;
    double sg, sgu;
    channel_sums(part, c, P, sg, sgu);
    if ((threadIdx.x & 63) != 0) return;
    if (dmul) {
        const double add = fac ? (double)fac[c] * sg : sg;
        dmul[c] = accumulate ? (float)((double)dmul[c] + sgu) : (float)sgu;
        dadd[c] = accumulate ? (float)((double)dadd[c] + add) : (float)add;
    }
    if (coef) {
        coef[c] = gamma[c] * rstd[c];
        coef[C + c] = (float)(sg / M);
        coef[2 * C + c] = (float)(sgu / M);
    }
}

// y = act(((x + p0) * p1) * a[c] + b[c])   (b null: 0)
template <bool VEC>
__global__ __launch_bounds__(THREADS) void bn_apply_kernel(const float* x, long long x_bs, float* y, long long y_bs, Shift sh,
                                                           const float* __restrict__ A, const float* __restrict__ B, int act, int HW, int S) {
    const int c = blockIdx.x / S, s = blockIdx.x % S, n = blockIdx.y;
    const long long po = (long long)c * HW;
    const float* xp = x + (long long)n * x_bs + po;
    float* yp = y + (long long)n * y_bs + po;
    float p0, p1;
    sh.get(c, p0, p1);
    const float a = A[c], b = B ? B[c] : 0.f;
    const int lo = s * CHUNK, hi = min(HW, lo + CHUNK);
    for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += STEP) {
        float v[4];
        load4<VEC>(xp, i, HW, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = fmaf((v[j] + p0) * p1, a, b);
            v[j] = act == DCVIC_ACT_LRELU02 ? (t > 0.f ? t : 0.2f * t) : t;
        }
        store4<VEC>(yp, i, HW, v);
    }
}

// dx = k1[c] * ((g' - k2[c]) - u * k3[c]); k3 null (ActNorm): dx = k1[c] * g', x is not read
template <bool VEC>
__global__ __launch_bounds__(THREADS) void bn_dx_kernel(const float* x, long long x_bs, const float* g, long long g_bs, const float* y,
                                                        long long y_bs, float* dx, long long dx_bs, Shift sh, const float* __restrict__ k1,
                                                        const float* __restrict__ k2, const float* __restrict__ k3, int act, int HW, int S) {
    const int c = blockIdx.x / S, s = blockIdx.x % S, n = blockIdx.y;
    const long long po = (long long)c * HW;
    const float* xp = x + (long long)n * x_bs + po;
    const float* gp = g + (long long)n * g_bs + po;
    const float* yp = act != DCVIC_ACT_NONE ? y + (long long)n * y_bs + po : nullptr;
    float* dp = dx + (long long)n * dx_bs + po;
    float p0 = 0.f, p1 = 1.f;
    if (k3) sh.get(c, p0, p1);
    const float f1 = k1[c], f2 = k3 ? k2[c] : 0.f, f3 = k3 ? k3[c] : 0.f;
    const int lo = s * CHUNK, hi = min(HW, lo + CHUNK);
    for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += STEP) {
        float xv[4], gv[4], yv[4];
        load4<VEC>(gp, i, HW, gv);
        if (k3) load4<VEC>(xp, i, HW, xv);
        if (yp) load4<VEC>(yp, i, HW, yv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gg = yp ? act_grad(gv[j], yv[j], act) : gv[j];
            gv[j] = k3 ? f1 * ((gg - f2) - ((xv[j] + p0) * p1) * f3) : f1 * gg;
        }
        store4<VEC>(dp, i, HW, gv);
    }
}

long long chunks(int HW) { return ((long long)HW + CHUNK - 1) / CHUNK; }

long long coef_offset(int N, int C, int HW) { return 16LL * C * N * chunks(HW); }

long long workspace_bytes(int N, int C, int HW) {
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    return coef_offset(N, C, HW) + (12LL * C + 15) / 16 * 16;
}

bool vec_ok(const void* p, long long bs) { return p == nullptr || (((uintptr_t)p & 15) == 0 && bs % 4 == 0); }

// the checks every entry point shares; `reduces`: it sums over the batch (M >= 2, a workspace)
int check_common(const char* name, int N, int C, int HW, bool reduces, const void* ws, long long ws_bytes, int act) {
    DCVIC_CHECK_ARG(N > 0 && C > 0 && HW > 0, "%s: empty tensor N=%d C=%d HW=%d", name, N, C, HW);
    DCVIC_CHECK_ARG(N <= 65535, "%s: N=%d, at most 65535 images", name, N);
    DCVIC_CHECK_ARG(HW <= (1 << 30) && (long long)C * chunks(HW) <= 0x7fffffffLL && (long long)N * chunks(HW) <= 0x7fffffffLL &&
                        (long long)C * N * chunks(HW) <= (1LL << 40),
                    "%s: N=%d C=%d HW=%d too large", name, N, C, HW);
    DCVIC_CHECK_ARG(act == DCVIC_ACT_NONE || act == DCVIC_ACT_LRELU02, "%s: act=%d, only none (0) and LeakyReLU(0.2) (%d) are fused", name, act,
                    DCVIC_ACT_LRELU02);
    if (reduces) {
        DCVIC_CHECK_ARG((long long)N * HW >= 2, "%s: M = N * HW = %lld, batch statistics need at least 2 values per channel", name, (long long)N * HW);
        DCVIC_CHECK_ARG(ws != nullptr, "%s: null pointer (workspace)", name);
        DCVIC_CHECK_ARG(((uintptr_t)ws & 7) == 0, "%s: workspace %p is not 8-byte aligned", name, ws);
        DCVIC_CHECK_ARG(ws_bytes >= workspace_bytes(N, C, HW), "%s: workspace of %lld bytes, needs %lld (dcvic_bn_workspace_bytes)", name, ws_bytes,
                        workspace_bytes(N, C, HW));
    }
    return DCVIC_OK;
}

int check_stride(const char* name, const char* what, long long bs, int C, int HW) {
    DCVIC_CHECK_ARG(bs >= (long long)C * HW, "%s: batch stride %lld of %s below its %lld values per image", name, bs, what, (long long)C * HW);
    return DCVIC_OK;
}

#define BN_TRY(expr)                    \
    do {                                \
        if (int rc__ = (expr)) return rc__; \
    } while (0)

int launch_sum_fwd(const char* name, const float* x, long long x_bs, double* part, int N, int C, int HW, hipStream_t st) {
    const int S = (int)chunks(HW);
    const dim3 grid((unsigned)(C * S), (unsigned)N);
    auto k = vec_ok(x, x_bs) && HW % 4 == 0 ? bn_sum_kernel<true, false> : bn_sum_kernel<false, false>;
    k<<<grid, THREADS, 0, st>>>(x, x_bs, nullptr, 0, nullptr, 0, Shift{nullptr, nullptr, 0}, DCVIC_ACT_NONE, part, N, HW, S);
    DCVIC_CHECK_LAUNCH(name);
    return DCVIC_OK;
}

// what both backwards share: the sum pass, the final pass, the dx pass
int launch_bwd(const char* name, const float* x, long long x_bs, const float* g, long long g_bs, const float* y, long long y_bs, Shift sh,
               const float* gamma, const float* rstd, const float* fac, float* dx, long long dx_bs, float* dmul, float* dadd, int accumulate,
               int act, bool batchnorm, void* ws, int N, int C, int HW, hipStream_t st) {
    const int S = (int)chunks(HW);
    const dim3 grid((unsigned)(C * S), (unsigned)N);
    double* part = (double*)ws;
    float* coef = batchnorm ? (float*)((char*)ws + coef_offset(N, C, HW)) : nullptr;
    const bool vec = HW % 4 == 0 && vec_ok(x, x_bs) && vec_ok(g, g_bs) && vec_ok(act != DCVIC_ACT_NONE ? y : nullptr, y_bs) && vec_ok(dx, dx_bs);
    if (batchnorm || dmul) {
        auto ks = vec ? bn_sum_kernel<true, true> : bn_sum_kernel<false, true>;
        ks<<<grid, THREADS, 0, st>>>(x, x_bs, g, g_bs, y, y_bs, sh, act, part, N, HW, S);
        DCVIC_CHECK_LAUNCH(name);
        bn_bwd_final_kernel<<<dcvic_cdiv(C, THREADS / 64), THREADS, 0, st>>>(part, N * S, (double)N * (double)HW, C, gamma, rstd, fac, dmul, dadd,
                                                                             accumulate, coef);
        DCVIC_CHECK_LAUNCH(name);
    }
    auto kd = vec ? bn_dx_kernel<true> : bn_dx_kernel<false>;
    if (batchnorm)
        kd<<<grid, THREADS, 0, st>>>(x, x_bs, g, g_bs, y, y_bs, dx, dx_bs, sh, coef, coef + C, coef + 2 * C, act, HW, S);
    else
        kd<<<grid, THREADS, 0, st>>>(x, x_bs, g, g_bs, y, y_bs, dx, dx_bs, sh, fac, nullptr, nullptr, act, HW, S);
    DCVIC_CHECK_LAUNCH(name);
    return DCVIC_OK;
}

}  // namespace

extern "C" long long dcvic_bn_workspace_bytes(int N, int C, int HW) { return workspace_bytes(N, C, HW); }

extern "C" int dcvic_bn_stats_f32(const float* x, long long x_bs, float* mean, float* std_unbiased, void* workspace, long long workspace_bytes_,
                                  int N, int C, int HW, void* stream) {
    const char* name = "bn_stats";
    BN_TRY(check_common(name, N, C, HW, true, workspace, workspace_bytes_, DCVIC_ACT_NONE));
    DCVIC_CHECK_ARG(x && mean && std_unbiased, "%s: null pointer (x %p, mean %p, std %p)", name, (const void*)x, (void*)mean, (void*)std_unbiased);
    BN_TRY(check_stride(name, "x", x_bs, C, HW));
    BN_TRY(launch_sum_fwd(name, x, x_bs, (double*)workspace, N, C, HW, (hipStream_t)stream));
    bn_fwd_final_kernel<<<dcvic_cdiv(C, THREADS / 64), THREADS, 0, (hipStream_t)stream>>>((const double*)workspace, N * (int)chunks(HW),
                                                                                         (double)N * (double)HW, C, 0.0, 0.0, mean, nullptr,
                                                                                         std_unbiased, nullptr, nullptr);
    DCVIC_CHECK_LAUNCH(name);
    return DCVIC_OK;
}

extern "C" int dcvic_bn_train_fwd_f32(const float* x, long long x_bs, float* y, long long y_bs, const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, double momentum, double eps, float* save_mean, float* save_rstd,
                                      int act, void* workspace, long long workspace_bytes_, int N, int C, int HW, void* stream) {
    const char* name = "bn_train_fwd";
    BN_TRY(check_common(name, N, C, HW, true, workspace, workspace_bytes_, act));
    DCVIC_CHECK_ARG(x && y && gamma && beta && save_mean && save_rstd, "%s: null pointer (x %p, y %p, gamma %p, beta %p, save_mean %p, save_rstd %p)",
                    name, (const void*)x, (void*)y, (const void*)gamma, (const void*)beta, (void*)save_mean, (void*)save_rstd);
    DCVIC_CHECK_ARG(!running_mean == !running_var, "%s: null pointer (running_mean %p, running_var %p: both or neither)", name, (void*)running_mean,
                    (void*)running_var);
    DCVIC_CHECK_ARG(eps > 0.0 && eps < (double)INFINITY,"%s: eps=%g, needs a finite positive value", name, eps);
    DCVIC_CHECK_ARG(momentum >= 0.0 && momentum <= 1.0, "%s: momentum=%g outside [0, 1]", name, momentum);
    BN_TRY(check_stride(name, "x", x_bs, C, HW));
    BN_TRY(check_stride(name, "y", y_bs, C, HW));
    hipStream_t st = (hipStream_t)stream;
    const int S = (int)chunks(HW);
    BN_TRY(launch_sum_fwd(name, x, x_bs, (double*)workspace, N, C, HW, st));
    bn_fwd_final_kernel<<<dcvic_cdiv(C, THREADS / 64), THREADS, 0, st>>>((const double*)workspace, N * S, (double)N * (double)HW, C, eps, momentum,
                                                                         save_mean, save_rstd, nullptr, running_mean, running_var);
    DCVIC_CHECK_LAUNCH(name);
    auto k = HW % 4 == 0 && vec_ok(x, x_bs) && vec_ok(y, y_bs) ? bn_apply_kernel<true> : bn_apply_kernel<false>;
    k<<<dim3((unsigned)(C * S), (unsigned)N), THREADS, 0, st>>>(x, x_bs, y, y_bs, Shift{save_mean, save_rstd, 1}, gamma, beta, act, HW, S);
    DCVIC_CHECK_LAUNCH(name);
    return DCVIC_OK;
}

extern "C" int dcvic_bn_train_bwd_f32(const float* x, long long x_bs, const float* g, long long g_bs, const float* y, long long y_bs,
                                      const float* save_mean, const float* save_rstd, const float* gamma, float* dx, long long dx_bs,
                                      float* dgamma, float* dbeta, int accumulate, int act, void* workspace, long long workspace_bytes_, int N,
                                      int C, int HW, void* stream) {
    const char* name = "bn_train_bwd";
    BN_TRY(check_common(name, N, C, HW, true, workspace, workspace_bytes_, act));
    DCVIC_CHECK_ARG(x && g && save_mean && save_rstd && gamma && dx, "%s: null pointer (x %p, g %p, save_mean %p, save_rstd %p, gamma %p, dx %p)", name,
                    (const void*)x, (const void*)g, (const void*)save_mean, (const void*)save_rstd, (const void*)gamma, (void*)dx);
    DCVIC_CHECK_ARG(y || act == DCVIC_ACT_NONE, "%s: null pointer (y, which a fused activation's derivative reads)", name);
    DCVIC_CHECK_ARG(!dgamma == !dbeta, "%s: null pointer (dgamma %p, dbeta %p: both or neither)", name, (void*)dgamma, (void*)dbeta);
    BN_TRY(check_stride(name, "x", x_bs, C, HW));
    BN_TRY(check_stride(name, "g", g_bs, C, HW));
    if (act != DCVIC_ACT_NONE) BN_TRY(check_stride(name, "y", y_bs, C, HW));
    BN_TRY(check_stride(name, "dx", dx_bs, C, HW));
    return launch_bwd(name, x, x_bs, g, g_bs, y, y_bs, Shift{save_mean, save_rstd, 1}, gamma, save_rstd, nullptr, dx, dx_bs, dgamma, dbeta,
                      accumulate ? 1 : 0, act, true, workspace, N, C, HW, (hipStream_t)stream);
}

extern "C" int dcvic_actnorm_fwd_f32(const float* x, long long x_bs, float* y, long long y_bs, const float* loc, const float* scale, int act, int N,
                                     int C, int HW, void* stream) {
    const char* name = "actnorm_fwd";
    BN_TRY(check_common(name, N, C, HW, false, nullptr, 0, act));
    DCVIC_CHECK_ARG(x && y && loc && scale, "%s: null pointer (x %p, y %p, loc %p, scale %p)", name, (const void*)x, (void*)y, (const void*)loc,
                    (const void*)scale);
    BN_TRY(check_stride(name, "x", x_bs, C, HW));
    BN_TRY(check_stride(name, "y", y_bs, C, HW));
    const int S = (int)chunks(HW);
    auto k = HW % 4 == 0 && vec_ok(x, x_bs) && vec_ok(y, y_bs) ? bn_apply_kernel<true> : bn_apply_kernel<false>;
    k<<<dim3((unsigned)(C * S), (unsigned)N), THREADS, 0, (hipStream_t)stream>>>(x, x_bs, y, y_bs, Shift{loc, nullptr, 0}, scale, nullptr, act, HW, S);
    DCVIC_CHECK_LAUNCH(name);
    return DCVIC_OK;
}

extern "C" int dcvic_actnorm_bwd_f32(const float* x, long long x_bs, const float* g, long long g_bs, const float* y, long long y_bs,
                                     const float* loc, const float* scale, float* dx, long long dx_bs, float* dloc, float* dscale, int accumulate,
                                     int act, void* workspace, long long workspace_bytes_, int N, int C, int HW, void* stream) {
    const char* name = "actnorm_bwd";
    BN_TRY(check_common(name, N, C, HW, true, workspace, workspace_bytes_, act));
    DCVIC_CHECK_ARG(x && g && loc && scale && dx, "%s: null pointer (x %p, g %p, loc %p, scale %p, dx %p)", name, (const void*)x, (const void*)g,
                    (const void*)loc, (const void*)scale, (void*)dx);
    DCVIC_CHECK_ARG(y || act == DCVIC_ACT_NONE, "%s: null pointer (y, which a fused activation's derivative reads)", name);
    DCVIC_CHECK_ARG(!dloc == !dscale, "%s: null pointer (dloc %p, dscale %p: both or neither)", name, (void*)dloc, (void*)dscale);
    BN_TRY(check_stride(name, "x", x_bs, C, HW));
    BN_TRY(check_stride(name, "g", g_bs, C, HW));
    if (act != DCVIC_ACT_NONE) BN_TRY(check_stride(name, "y", y_bs, C, HW));
    BN_TRY(check_stride(name, "dx", dx_bs, C, HW));
    return launch_bwd(name, x, x_bs, g, g_bs, y, y_bs, Shift{loc, nullptr, 0}, nullptr, nullptr, scale, dx, dx_bs, dscale, dloc, accumulate ? 1 : 0,
                      act, false, workspace, N, C, HW, (hipStream_t)stream);
}
