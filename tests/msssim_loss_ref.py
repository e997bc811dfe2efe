"""MSSSIMLoss and L1Loss of the reference's src/losses/distortion_loss.py restated in plain torch (no test in here; used by
test_msssim_loss_host.py, test_gpu_msssim_loss.py and msssim_step_ref.py).

MSSSIMLoss is loss_weight * (1 - MS_SSIM(data_range=1, size_average=True, channel=3)(real, fake)) of pytorch-msssim 0.2.1, which is
neither in the reference tree nor importable here: restated from the package's source as tests/test_ssim_host.py restates it for the
validation metric (same window, same pools, same weights), but on the float images as they are and with C1 = 0.01^2, C2 = 0.03^2.
`dtype` is the precision of every tensor on the way (the window and the weights are the package's fp32 values, widened for fp64);
torch autograd gives the gradient."""
import functools

import torch
import torch.nn.functional as F

from test_ssim_host import WEIGHTS, ssim_window

C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
MIN_SIDE = 160
REGIMES = ("near", "far", "unclamped", "anticorrelated", "identical")


def _filter(X, win):
    C = X.shape[1]
    out = F.conv2d(X, win.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(out, win.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)


def _ssim(X, Y, win):
    mu1, mu2 = _filter(X, win), _filter(Y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = _filter(X * X, win) - mu1_sq
    s2 = _filter(Y * Y, win) - mu2_sq
    s12 = _filter(X * Y, win) - mu1_mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def factors(real, fake, dtype=torch.float64):
    """[5, N, C]: the per-plane means cs_0 .. cs_3, ssim_4 before the relu."""
    X, Y = real.to(dtype), fake.to(dtype)
    assert min(X.shape[-2:]) > MIN_SIDE, "pytorch-msssim asserts min(H, W) > (11 - 1) * 2^4"
    win = ssim_window().to(device=X.device, dtype=dtype)
    f = []
    for i in range(5):
        ssim_pc, cs = _ssim(X, Y, win)
        if i < 4:
            f.append(cs)
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    return torch.stack(f + [ssim_pc], dim=0)


def ms_ssim_planes(real, fake, dtype=torch.float64):
    """[N, C]: prod_s relu(f_s)^w_s."""
    f = factors(real, fake, dtype)
    w = torch.tensor(WEIGHTS, dtype=torch.float32).to(device=f.device, dtype=dtype)
    return torch.prod(torch.relu(f) ** w.view(-1, 1, 1), dim=0)


def ms_ssim_loss(real, fake, loss_weight, dtype=torch.float64):
    return loss_weight * (1 - ms_ssim_planes(real, fake, dtype).mean())


def l1_loss(real, fake, loss_weight, dtype=torch.float64):
    return loss_weight * F.l1_loss(real.to(dtype), fake.to(dtype))


def value_and_grad(fn, real, fake, loss_weight, dtype):
    """(loss, d loss / d fake) of fn in `dtype`, both as fp64 CPU tensors."""
    y = fake.detach().to(dtype).clone().requires_grad_(True)
    v = fn(real.detach().to(dtype), y, loss_weight, dtype)
    v.backward()
    return v.detach().double(), y.grad.detach().double()


# ---------------------------------------------------------------------------------------------------- the GPU tests' inputs
def smooth(shape, seed):
    """Bicubic-smoothed uniform noise in [-1, 1] (fp32), a textured image."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((N, C, H // 6 + 2, W // 6 + 2), generator=g, dtype=torch.float64) * 2.4 - 1.2
    return F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(-1, 1).float()


@functools.lru_cache(maxsize=None)
def pair(shape, regime, seed=0):
    """(real, fake) fp32 CPU tensors of `shape` for one of REGIMES."""
    real = smooth(shape, 100 + seed)
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(200 + seed), dtype=torch.float64).float()
    if regime == "near":
        real = real.clone()
        real[:, :, 60:100, 70:120] = 0.25                   # a constant 40 x 50 patch, shared: zero variance, zero covariance
        fake = real + 0.03 * noise
        fake[:, :, 60:100, 70:120] = 0.25
    elif regime == "far":
        fake = real + 0.3 * noise
    elif regime == "unclamped":
        fake = 1.5 * real + 0.1 * noise
    elif regime == "anticorrelated":
        fake = -real
    elif regime == "identical":
        fake = real.clone()
    else:
        raise KeyError(regime)
    return real.contiguous(), fake.contiguous()


@functools.lru_cache(maxsize=None)
def reference(shape, regime, loss_weight, seed=0):
    """dict(loss64, grad64, loss32, grad32, factors) for pair(shape, regime): the fp64 restatement, the fp32 one (both as fp64 tensors)
    and the fp64 factors [5, N, C].  Computed once per case; callers leave it unchanged."""
    real, fake = pair(shape, regime, seed)
    l64, g64 = value_and_grad(ms_ssim_loss, real, fake, loss_weight, torch.float64)
    l32, g32 = value_and_grad(ms_ssim_loss, real, fake, loss_weight, torch.float32)
    return dict(loss64=l64, grad64=g64, loss32=l32, grad32=g32, factors=factors(real, fake, torch.float64))
