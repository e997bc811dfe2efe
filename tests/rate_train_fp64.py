"""The rate term restated in plain torch (no test in here; shared by test_rate_train_host.py and test_gpu_rate_train.py).

PARITY UNPINNED: CompressAI 1.2.4 is neither in the reference tree nor importable, so this restates its
GaussianConditional.forward(training=True), EntropyBottleneck.forward(training=True), EntropyBottleneck.loss() and LowerBound from
SURVEY App-B, as the reference drives them (ste_gaussian_conditional.py:16-23, entropy_bottleneck.py:19-28), in the dtype it is given:
fp64 is the yardstick, the same code in fp32 on the CPU is the reference's own arithmetic and gives the error the bounds start from.
The two bounds are the fp32 numbers the fp32 reference holds (0.11f, 1e-9f), in every dtype."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SCALE_BOUND = float(np.float32(0.11))
LIK_BOUND = float(np.float32(1e-9))
LN2 = math.log(2.0)
EB_NAMES = tuple(f"_matrix{i}" for i in range(5)) + tuple(f"_bias{i}" for i in range(5)) + tuple(f"_factor{i}" for i in range(4))


class LowerBound(torch.autograd.Function):
    """CompressAI's LowerBound: max(x, bound); the gradient passes when x >= bound or when it is negative."""

    @staticmethod
    def forward(ctx, x, bound):
        b = torch.tensor(bound, dtype=x.dtype)
        ctx.save_for_backward(x, b)
        return torch.max(x, b)

    @staticmethod
    def backward(ctx, g):
        x, b = ctx.saved_tensors
        return ((x >= b) | (g < 0)).to(g.dtype) * g, None


def std_cumulative(x):
    return 0.5 * torch.erfc(-(2 ** -0.5) * x)


def gaussian_likelihood(y, mu, sigma, noise):
    v = torch.abs(y + noise - mu)
    s = LowerBound.apply(sigma, SCALE_BOUND)
    p_raw = std_cumulative((0.5 - v) / s) - std_cumulative((-0.5 - v) / s)
    return LowerBound.apply(p_raw, LIK_BOUND), p_raw


def image_bits(lik):
    return -torch.log(lik).flatten(1).sum(1) / LN2


def gaussian_rate(y, mu, sigma, noise, w, scale, dtype=torch.float64):
    """dict(lik, p_raw, bits [N], loss, dy, dmu, dsigma) of loss = sum_n scale * w[n] * bits[n]; inputs are CPU tensors of any
    float dtype (views welcome), w None for 1."""
    y, mu, sigma = (t.detach().to(dtype).clone().requires_grad_(True) for t in (y, mu, sigma))
    lik, p_raw = gaussian_likelihood(y, mu, sigma, noise.to(dtype))
    bits = image_bits(lik)
    wv = torch.ones(y.shape[0], dtype=dtype) if w is None else w.to(dtype)
    loss = (scale * wv * bits).sum()
    loss.backward()
    return dict(lik=lik.detach(), p_raw=p_raw.detach(), bits=bits.detach(), loss=loss.detach(), dy=y.grad, dmu=mu.grad, dsigma=sigma.grad)


def eb_logits(x, P, detach=False):
    """EntropyBottleneck._logits_cumulative on x [C, 1, M]."""
    g = (lambda t: t.detach()) if detach else (lambda t: t)
    logits = x
    for i in range(5):
        logits = torch.matmul(F.softplus(g(P[f"_matrix{i}"])), logits) + g(P[f"_bias{i}"])
        if i < 4:
            logits = logits + torch.tanh(g(P[f"_factor{i}"])) * torch.tanh(logits)
    return logits


def eb_likelihood(z, noise, P):
    N, C = z.shape[:2]
    v = (z + noise).permute(1, 0, 2, 3).reshape(C, 1, -1)
    lower, upper = eb_logits(v - 0.5, P), eb_logits(v + 0.5, P)
    sign = -torch.sign(lower + upper).detach()
    p_raw = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))
    back = lambda t: t.reshape(C, N, *z.shape[2:]).permute(1, 0, 2, 3)
    return back(LowerBound.apply(p_raw, LIK_BOUND)), back(p_raw)


def eb_params(sd, prefix, dtype, requires_grad=True):
    return {k: sd[f"{prefix}.{k}"].detach().to(dtype).clone().requires_grad_(requires_grad) for k in EB_NAMES + ("quantiles",)}


def eb_rate(z, noise, sd, prefix, w, scale, dtype=torch.float64):
    """dict(lik, p_raw, bits, loss, dz, grads {name: gradient w.r.t. the raw parameter}) of loss = sum_n scale * w[n] * bits[n]."""
    P = eb_params(sd, prefix, dtype)
    z = z.detach().to(dtype).clone().requires_grad_(True)
    lik, p_raw = eb_likelihood(z, noise.to(dtype), P)
    bits = image_bits(lik)
    wv = torch.ones(z.shape[0], dtype=dtype) if w is None else w.to(dtype)
    loss = (scale * wv * bits).sum()
    loss.backward()
    return dict(lik=lik.detach(), p_raw=p_raw.detach(), bits=bits.detach(), loss=loss.detach(), dz=z.grad, grads={k: P[k].grad for k in EB_NAMES})


def eb_aux(sd, prefix, tail_mass=1e-9, dtype=torch.float64):
    """EntropyBottleneck.loss(): (value, gradient w.r.t. quantiles [C, 1, 3]); the parameters are stop-gradient."""
    P = eb_params(sd, prefix, dtype)
    t = math.log(2 / tail_mass - 1)
    target = torch.tensor([-t, 0.0, t], dtype=torch.float32).to(dtype)       # the module's fp32 buffer
    aux = torch.abs(eb_logits(P["quantiles"], P, detach=True) - target).sum()
    aux.backward()
    assert all(P[k].grad is None for k in EB_NAMES)
    return aux.detach(), P["quantiles"].grad


# ---------------------------------------------------------------------------------------------------- inputs
# planted elements of the Gaussian cases, as (y, u, mu, sigma) at flat indexes 0.. of image 0 (as many as the shape holds):
#   sigma 0.05 (below the scale bound) where the gradient w.r.t. s is positive (v = 0: blocked) and negative (v = 0.625: passes);
#   |y + u - mu| = 12 at sigma = 0.11f: p_raw < 1e-9;  y + u == mu exactly: sign(0) = 0
PLANTED = ((1.25, 0.25, 1.5, 0.05), (1.0, 0.125, 0.5, 0.05), (3.0, 0.25, -8.75, SCALE_BOUND), (1.25, 0.25, 1.5, 1.0))


def gaussian_inputs(shape, seed, plant=True):
    """y ~ 3 N(0, 1), sigma log-uniform in [0.05, 8], mu = y + 1.5 max(sigma, 0.11) N(0, 1), u ~ U(-0.5, 0.5): fp32 CPU tensors,
    plus per-sample weights that include a 0 when N > 1."""
    g = torch.Generator().manual_seed(seed)
    y = 3 * torch.randn(shape, generator=g)
    sigma = torch.exp(torch.rand(shape, generator=g) * (math.log(8.0) - math.log(0.05)) + math.log(0.05))
    mu = y + 1.5 * torch.clamp(sigma, min=0.11) * torch.randn(shape, generator=g)
    u = torch.rand(shape, generator=g) - 0.5
    if plant:
        for i, (a, b, c, d) in enumerate(PLANTED[:y[0].numel()]):
            y[0].view(-1)[i], u[0].view(-1)[i], mu[0].view(-1)[i], sigma[0].view(-1)[i] = a, b, c, d
    w = torch.tensor([0.7, 0.0, 1.3, 0.4, 2.0, 0.9, 0.0, 1.1][:shape[0]], dtype=torch.float32) if shape[0] <= 8 else torch.rand(shape[0], generator=g)
    return y, mu, sigma, u, w


def eb_inputs(shape, seed):
    """z ~ 4 N(0, 1), u ~ U(-0.5, 0.5), weights as above; the parameters come from oracle.entropy_oracle.synth_entropy_bottleneck."""
    g = torch.Generator().manual_seed(seed)
    z = 4 * torch.randn(shape, generator=g)
    u = torch.rand(shape, generator=g) - 0.5
    w = torch.tensor([0.7, 0.0, 1.3, 0.4, 2.0, 0.9, 0.0, 1.1][:shape[0]], dtype=torch.float32)
    return z, u, w


# ---------------------------------------------------------------------------------------------------- bounds
VALUE_FLOOR, GRAD_FLOOR, LIK_FLOOR = 1e-6, 1e-5, 1e-5


def value_err(got, want):
    """relative error of a value (vector: the largest, relative to the largest magnitude)"""
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def grad_err(got, want):
    """largest error of a gradient tensor, relative to the tensor's largest magnitude"""
    got, want = got.double(), want.double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def lik_err(got, want):
    return float((got.double() - want.double()).abs().max())


def bound(fp32_err, floor):
    """4 x the error of the fp32 restatement on the same inputs (the device's erfcf / expf / tanhf differ from the host's by a few
    ulp), or the project's floor, whichever is larger"""
    return max(4.0 * fp32_err, floor)
