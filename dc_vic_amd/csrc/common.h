// Shared host/device helpers for libdcvic_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <type_traits>

#include "dcvic.h"

void dcvic_set_error(const char* fmt, ...);

#define DCVIC_CHECK_ARG(cond, ...)            \
    do {                                      \
        if (!(cond)) {                        \
            dcvic_set_error(__VA_ARGS__);     \
            return DCVIC_EINVAL;              \
        }                                     \
    } while (0)

#define DCVIC_CHECK_LAUNCH(what)                                                   \
    do {                                                                           \
        hipError_t e__ = hipGetLastError();                                        \
        if (e__ != hipSuccess) {                                                   \
            dcvic_set_error("%s: %s", what, hipGetErrorString(e__));               \
            return DCVIC_ELAUNCH;                                                  \
        }                                                                          \
    } while (0)

// The activation as a compile-time choice: the one place the expressions are written.  Any other ACT is the identity.
// CAUTION: the same expression can round differently as straight-line code and behind dcvic_act's switch.  hipcc contracts a * b + c
// across statements, so with the switch gone the activation's last multiply can presumably fuse with what the caller adds next (a residual, an
// affine map), and the transcendental forms (GELU, swish, sigmoid, tanh) are where it showed: conv1x1_dma_kernel with a compiled-in GELU
// body no longer gave the bits of the other convolution kernels on the same layer.  none / ReLU / leaky ReLU have no rounding of their
// own and are safe.  groupnorm_kernel uses the transcendental forms straight-line; it stores the activation's result as is, and
// tests/test_gpu_act_paths.py pins its bits.  Before using dcvic_act_c<transcendental> in a kernel whose results must equal another
// kernel's, compare the two bit for bit.
template <int ACT>
__device__ __forceinline__ float dcvic_act_c(float v) {
    if constexpr (ACT == DCVIC_ACT_RELU) return fmaxf(v, 0.f);
    else if constexpr (ACT == DCVIC_ACT_LRELU02) return v > 0.f ? v : 0.2f * v;
    else if constexpr (ACT == DCVIC_ACT_SWISH) return v / (1.f + expf(-v));
    else if constexpr (ACT == DCVIC_ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    else if constexpr (ACT == DCVIC_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
    else if constexpr (ACT == DCVIC_ACT_HALF_TANH) return 0.5f * tanhf(v);
    else return v;
}

// calls f(std::integral_constant<int, ACT>{}) for the launch's activation from ONE switch: a kernel whose `act` is uniform over the
// launch runs its per-value loops inside f, where the activation is straight-line code (the switch per value put every expf in a
// basic block of its own and kept the scheduler from overlapping the values of an unrolled loop)
template <class F>
__device__ __forceinline__ void dcvic_act_dispatch(int act, F&& f) {
    switch (act) {
        case DCVIC_ACT_RELU: f(std::integral_constant<int, DCVIC_ACT_RELU>{}); break;
        case DCVIC_ACT_LRELU02: f(std::integral_constant<int, DCVIC_ACT_LRELU02>{}); break;
        case DCVIC_ACT_SWISH: f(std::integral_constant<int, DCVIC_ACT_SWISH>{}); break;
        case DCVIC_ACT_GELU: f(std::integral_constant<int, DCVIC_ACT_GELU>{}); break;
        case DCVIC_ACT_SIGMOID: f(std::integral_constant<int, DCVIC_ACT_SIGMOID>{}); break;
        case DCVIC_ACT_HALF_TANH: f(std::integral_constant<int, DCVIC_ACT_HALF_TANH>{}); break;
        default: f(std::integral_constant<int, DCVIC_ACT_NONE>{}); break;
    }
}

// the activation chosen at run time, per value
__device__ __forceinline__ float dcvic_act(float v, int act) {
    float r;
    dcvic_act_dispatch(act, [&](auto a) { r = dcvic_act_c<decltype(a)::value>(v); });
    return r;
}

// A kernel that compiles a body of its own only for SOME activations (the ones its layers launch it with) names every other launch
// DCVIC_ACT_ANY: dcvic_act_of<DCVIC_ACT_ANY>(v, act) keeps the per-value switch, dcvic_act_of<ACT>(v, act) is dcvic_act_c<ACT>(v).
#define DCVIC_ACT_ANY (-1)
template <int ACT>
__device__ __forceinline__ float dcvic_act_of(float v, int act) {
    if constexpr (ACT == DCVIC_ACT_ANY) return dcvic_act(v, act);
    else return dcvic_act_c<ACT>(v);
}
// calls f(std::integral_constant<int, A>{}) with A = act when act is one of ACTS, else with A = DCVIC_ACT_ANY
template <int... ACTS, class F>
__device__ __forceinline__ void dcvic_act_dispatch_some(int act, F&& f) {
    const bool hit = ((act == ACTS ? (f(std::integral_constant<int, ACTS>{}), true) : false) || ...);
    if (!hit) f(std::integral_constant<int, DCVIC_ACT_ANY>{});
}

// Function attributes (dynamic-LDS limit) are per device.  `if (DcvicAttrOnce once{mask}) { hipFuncSetAttribute(...); }` runs the
// body until it has COMPLETED once on the current HIP device: the device's bit in the site-local mask is set by the destructor,
// i.e. after the attribute calls -- a second thread arriving meanwhile applies the (idempotent) attribute itself instead of
// launching a > 64 KiB-LDS kernel before it is in effect.  Devices >= 32 re-apply on every call.
struct DcvicAttrOnce {
    std::atomic<unsigned>& mask;
    unsigned bit = 0;
    bool need = true;
    explicit DcvicAttrOnce(std::atomic<unsigned>& m) : mask(m) {
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 32) {
            bit = 1u << dev;
            need = (mask.load(std::memory_order_acquire) & bit) == 0;
        }
    }
    ~DcvicAttrOnce() { if (need && bit) mask.fetch_or(bit, std::memory_order_release); }
    explicit operator bool() const { return need; }
    DcvicAttrOnce(const DcvicAttrOnce&) = delete;
    DcvicAttrOnce& operator=(const DcvicAttrOnce&) = delete;
};
// Compute units of the current HIP device (cached per ordinal).
int dcvic_num_cu();

static inline int dcvic_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
