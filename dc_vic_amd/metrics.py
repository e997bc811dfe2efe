"""Full-reference perceptual metrics on HIP kernels: DISTS and LPIPS(alex), one value per image pair, as the reference's
scripts/calc_metrics.py:174-215 reports them (batch size 1, full resolution, mean over images of the per-image value).

PARITY UNPINNED: neither the `DISTS_pytorch` nor the `lpips` package is in the reference tree, and neither they nor their weights can
be fetched.  Both metrics are restated from the published packages and load their state dicts by key (`DISTSVGG.from_files`,
`load_lpips`); `tests/test_metrics_host.py` pins the restatement as a plain-torch fp64 function, which the GPU tests compare against.

DISTS (Ding et al. 2020): taps [x, relu1_2, relu2_2, relu3_3, relu4_3, relu5_3] of a VGG16 whose max pools are L2 pools
(csrc/metrics.hip), on (x - mean) / std for the convolutions and on the raw [0, 1] input for tap 0; per-channel fp64 moments of the
two images' taps; 1 - sum alpha S1 + beta S2.  The 3x3 convolutions may run as Winograd F(2x2, 3x3) (layers.allow_winograd: no
integer decision follows them), which re-associates each sum and lands closer to fp64 than the direct fmaf chain.

x and y run through the network as ONE batch of 2N images.  The conv, pool and moments kernels are batch-invariant, so every image's
value has the same bits whichever images share its batch.  No torch compute op touches the data: torch allocates and takes views."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import check, lib
from .layers import Conv2d, allow_winograd
from .ops import _chk4, _p, _stream

Tensor = torch.Tensor

DISTS_CHNS = (3, 64, 128, 256, 512, 512)
DISTS_MEAN = (0.485, 0.456, 0.406)
DISTS_STD = (0.229, 0.224, 0.225)
# torchvision vgg16().features indices of the convs of each DISTS stage, and the index of the L2 pool opening stages 2-5
VGG16_STAGES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
POOL_INDEX = (None, 4, 9, 16, 23)
_CONV_CH = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))


def hann_filter() -> Tensor:
    """The L2 pool's 3x3 kernel: outer(a, a) / sum with a = hanning(5)[1:-1] = [.5, 1, .5]  ->  [[1,2,1],[2,4,2],[1,2,1]] / 16."""
    a = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    g = a[:, None] * a[None, :]
    return (g / g.sum()).float()


class L2Pool(nn.Module):
    """L2pooling(channels): holds the package's `filter` buffer [C, 1, 3, 3] (so a DISTS state dict loads by key); the pool itself is
    dcvic_l2pool_f32, whose kernel is the fixed Hann filter -- a state dict whose filter differs is rejected on load."""

    def __init__(self, channels: int):
        super().__init__()
        self.register_buffer("filter", hann_filter()[None, None].repeat(channels, 1, 1, 1))

    def forward(self, x: Tensor) -> Tensor:
        return l2pool(x)


class DISTSVGG(nn.Module):
    """DISTS() of DISTS_pytorch: stage1..stage5 with the package's sub-module indices (stage2.4 is the first L2 pool, stage2.5 the
    first conv of stage 2, ...), the mean / std buffers and alpha / beta [1, 1475, 1, 1].  Use `from_files` for real weights."""

    def __init__(self):
        super().__init__()
        it = iter(_CONV_CH)
        for s, idxs in enumerate(VGG16_STAGES):
            st = nn.Sequential()
            if POOL_INDEX[s] is not None:
                st.add_module(str(POOL_INDEX[s]), L2Pool(DISTS_CHNS[s]))
            for i in idxs:
                ci, co = next(it)
                st.add_module(str(i), Conv2d(ci, co, 3, 1, 1))
            setattr(self, f"stage{s + 1}", st)
        self.register_buffer("mean", torch.tensor(DISTS_MEAN).view(1, -1, 1, 1))
        self.register_buffer("std", torch.tensor(DISTS_STD).view(1, -1, 1, 1))
        self.alpha = nn.Parameter(torch.full((1, sum(DISTS_CHNS), 1, 1), 0.1), requires_grad=False)
        self.beta = nn.Parameter(torch.full((1, sum(DISTS_CHNS), 1, 1), 0.1), requires_grad=False)
        allow_winograd(self)
        self._prep = None
        self._prep_key = None

    def stages(self) -> List[Tuple[Optional[L2Pool], List[Conv2d]]]:
        out = []
        for s in range(5):
            st = getattr(self, f"stage{s + 1}")
            pool = st[0] if isinstance(st[0], L2Pool) else None
            out.append((pool, [m for m in st if isinstance(m, Conv2d)]))
        return out

    def convs(self) -> List[Conv2d]:
        return [m for _, cs in self.stages() for m in cs]

    # ------------------------------------------------------------------------------------------ constructors
    @classmethod
    def synthetic(cls, seed: int = 0) -> "DISTSVGG":
        """Deterministic synthetic weights (tests and benchmarks only): He-normal convs, small biases, alpha / beta ~ N(0.1, 0.01)
        as the package initialises them."""
        m = cls()
        g = torch.Generator().manual_seed(2000 + seed)
        for c in m.convs():
            fan_in = c.weight.shape[1] * 9
            c.weight.data.copy_(torch.randn(c.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            c.bias.data.copy_(torch.randn(c.bias.shape, generator=g) * 0.01)
        m.alpha.data.copy_(0.1 + 0.01 * torch.randn(m.alpha.shape, generator=g))
        m.beta.data.copy_(0.1 + 0.01 * torch.randn(m.beta.shape, generator=g))
        return m

    @classmethod
    def from_state_dicts(cls, vgg16: Optional[Dict[str, Tensor]], dists: Dict[str, Tensor]) -> "DISTSVGG":
        """`dists` is either a complete DISTS() state dict (then `vgg16` must be None) or the package's weights.pt, {alpha, beta}, with
        `vgg16` a torchvision vgg16 state dict (features.<i>.weight / bias; classifier keys ignored)."""
        if not isinstance(dists, dict):
            raise ValueError(f"DISTS weights: expected a dict, got {type(dists).__name__}")
        m = cls()
        full = any(k.startswith("stage") for k in dists)
        if full:
            if vgg16 is not None:
                raise ValueError("DISTS weights: a complete DISTS state dict holds the VGG16 convs already; do not pass a VGG16 file too")
            m._load_full(dists)
        else:
            if vgg16 is None:
                raise ValueError("DISTS weights: an alpha / beta file needs the torchvision VGG16 state dict too (--vgg16_path)")
            if not isinstance(vgg16, dict):
                raise ValueError(f"VGG16 weights: expected a dict, got {type(vgg16).__name__}")
            convs = m.convs()
            for c, i in zip(convs, [i for idxs in VGG16_STAGES for i in idxs]):
                _copy(c.weight, vgg16, f"features.{i}.weight", "VGG16")
                _copy(c.bias, vgg16, f"features.{i}.bias", "VGG16")
        _copy(m.alpha, dists, "alpha", "DISTS")
        _copy(m.beta, dists, "beta", "DISTS")
        return m

    @classmethod
    def from_files(cls, vgg16_path: Optional[str] = None, dists_path: str = "") -> "DISTSVGG":
        """Load with torch.load(weights_only=True): `dists_path` a complete DISTS() state dict, or the package's weights.pt (alpha,
        beta) together with `vgg16_path`, torchvision's VGG16 ImageNet state dict."""
        if not dists_path:
            raise ValueError("DISTS weights: dists_path is required")
        dists = torch.load(dists_path, map_location="cpu", weights_only=True)
        vgg = torch.load(vgg16_path, map_location="cpu", weights_only=True) if vgg16_path else None
        return cls.from_state_dicts(vgg, dists)

    def _load_full(self, sd: Dict[str, Tensor]) -> None:
        """Convs mapped by their order inside each stage (the sub-module indices themselves do not matter); filters checked."""
        for s, (pool, convs) in enumerate(self.stages()):
            pre = f"stage{s + 1}."
            idx = sorted({int(k[len(pre):].split(".")[0]) for k in sd
                          if k.startswith(pre) and k.endswith(".weight") and k[len(pre):].split(".")[0].isdigit()
                          and getattr(sd[k], "dim", lambda: 0)() == 4})
            if len(idx) != len(convs):
                raise ValueError(f"DISTS state dict: {pre}* holds {len(idx)} conv weights, expected {len(convs)}")
            for c, i in zip(convs, idx):
                _copy(c.weight, sd, f"{pre}{i}.weight", "DISTS")
                _copy(c.bias, sd, f"{pre}{i}.bias", "DISTS")
            filt = sorted(k for k in sd if k.startswith(pre) and k.endswith(".filter"))
            if (pool is None) != (not filt) or len(filt) > 1:
                raise ValueError(f"DISTS state dict: {pre}* has {len(filt)} L2 pool filters, expected {0 if pool is None else 1}")
            if pool is not None:
                f = sd[filt[0]]
                if tuple(f.shape) != tuple(pool.filter.shape):
                    raise ValueError(f"DISTS state dict: {filt[0]} has shape {tuple(f.shape)}, expected {tuple(pool.filter.shape)}")
                if not torch.allclose(f.double(), pool.filter.double(), rtol=0, atol=1e-7):
                    raise ValueError(f"DISTS state dict: {filt[0]} is not the Hann 3x3 filter [[1,2,1],[2,4,2],[1,2,1]]/16 of L2pooling")
        _copy(self.mean, sd, "mean", "DISTS")
        _copy(self.std, sd, "std", "DISTS")

    # ------------------------------------------------------------------------------------------ derived constants
    def prepared(self) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """(scale, shift) of the input normalisation as chan_affine vectors [1, 3] -- x * (1 + scale) + shift = (x - mean) / std -- and
        alpha / w_sum, beta / w_sum (fp64 [1475], w_sum = sum alpha + sum beta) on the module's device.  Weight preparation, cached."""
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in (self.alpha, self.beta, self.mean, self.std))
        if self._prep is None or self._prep_key != key:
            a, b = self.alpha.detach().double().reshape(-1), self.beta.detach().double().reshape(-1)
            w_sum = a.sum() + b.sum()
            mean, std = self.mean.detach().reshape(1, 3), self.std.detach().reshape(1, 3)
            self._prep = ((1.0 / std - 1.0).float().contiguous(), (-mean / std).float().contiguous(), (a / w_sum).contiguous(),
                          (b / w_sum).contiguous())
            self._prep_key = key
        return self._prep


def _copy(dst: Tensor, sd: Dict[str, Tensor], key: str, what: str) -> None:
    if key not in sd:
        raise ValueError(f"{what} state dict lacks {key!r}")
    v = sd[key]
    if not isinstance(v, torch.Tensor) or tuple(v.shape) != tuple(dst.shape):
        shape = tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__
        raise ValueError(f"{what} state dict: {key} has shape {shape}, expected {tuple(dst.shape)}")
    dst.data.copy_(v.to(dst.device, dtype=dst.dtype))


def load_lpips(state: Optional[Dict[str, Tensor]] = None, seed: int = 0):
    """LPIPSAlex (train/lpips.py) with an `lpips.LPIPS(net='alex')` state dict loaded strictly by key and shape; synthetic weights of
    `seed` when `state` is None (tests and benchmarks only)."""
    from .train.lpips import LPIPSAlex
    m = LPIPSAlex(seed)
    if state is not None:
        if not isinstance(state, dict):
            raise ValueError(f"LPIPS weights: expected a dict, got {type(state).__name__}")
        for k, v in m.state_dict().items():
            _copy(v, state, k, "lpips")
    return m


# ------------------------------------------------------------------------------------------------ kernels
def l2pool(x: Tensor) -> Tensor:
    """DISTS L2pooling: sqrt(conv2d(x^2, hann3x3, stride 2, pad 1, groups=C) + 1e-12) -> [N, C, (H-1)//2+1, (W-1)//2+1]."""
    N, Cc, H, W = _chk4(x, "l2pool x")
    if not x.is_contiguous():
        raise ValueError("l2pool: x must be contiguous")
    y = torch.empty((N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    check(lib().dcvic_l2pool_f32(_p(x), _p(y), N * Cc, H, W, _stream()), "l2pool")
    return y


def pair_moments(f0: Tensor, f1: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Per (n, c) of two same-shape dense maps: [mu_x, mu_y, var_x, var_y, cov_xy] in fp64 -> [N, C, 5] (or written into `out`, a
    [N, >= C, 5] fp64 view with unit strides inside each image, e.g. a channel slice of the DISTS moments buffer)."""
    N, Cc, H, W = _chk4(f0, "moments f0")
    if tuple(f1.shape) != tuple(f0.shape):
        raise ValueError(f"pair_moments: shapes differ {tuple(f0.shape)} vs {tuple(f1.shape)}")
    _chk4(f1, "moments f1")
    for t, nm in ((f0, "f0"), (f1, "f1")):
        if N > 1 and t.stride(0) != Cc * H * W:
            raise ValueError(f"pair_moments: {nm} must be dense over the batch")
    if out is None:
        out = torch.empty((N, Cc, 5), dtype=torch.float64, device=f0.device)
    if out.dtype != torch.float64 or out.device != f0.device or out.dim() != 3 or out.shape[0] != N or out.shape[1] != Cc \
            or out.shape[2] != 5 or out.stride(2) != 1 or (Cc > 1 and out.stride(1) != 5):
        raise ValueError("pair_moments: out must be an fp64 [N, C, 5] view with unit strides inside each image")
    ws = torch.empty(max(1, lib().dcvic_pair_moments_workspace_doubles(N * Cc, H * W)), dtype=torch.float64, device=f0.device)
    out_bs = out.stride(0) if N > 1 else max(out.stride(0), 5 * Cc)
    check(lib().dcvic_pair_moments_f64(_p(f0), _p(f1), N, Cc, H * W, _p(out), out_bs, _p(ws), _stream()), "pair_moments")
    return out


def _pair_batch(x: Tensor, y: Tensor, what: str) -> Tuple[Tensor, int]:
    """[x; y] as one dense batch of 2N (copied by the plane-copy kernel)."""
    N, Cc, H, W = _chk4(x, f"{what} x")
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError(f"{what}: x and y differ in shape {tuple(x.shape)} vs {tuple(y.shape)}")
    _chk4(y, f"{what} y")
    if Cc != 3:
        raise ValueError(f"{what}: need RGB images [N, 3, H, W], got {tuple(x.shape)}")
    xy = torch.empty((2 * N, 3, H, W), dtype=torch.float32, device=x.device)
    ops.copy_planes(xy[:N], x, H, W)
    ops.copy_planes(xy[N:], y, H, W)
    return xy, N


@torch.no_grad()
def dists(model: DISTSVGG, x: Tensor, y: Tensor) -> Tensor:
    """DISTS(x_n, y_n) for each n: x, y fp32 [N, 3, H, W] RGB in [0, 1] on the current device -> fp64 [N] on the device."""
    xy, N = _pair_batch(x, y, "dists")
    scale, shift, alpha, beta = model.prepared()
    mom = torch.empty((N, sum(DISTS_CHNS), 5), dtype=torch.float64, device=x.device)
    pair_moments(xy[:N], xy[N:], out=mom[:, 0:3])
    h = ops.chan_affine(xy, scale, shift)
    off = 3
    for s, (pool, convs) in enumerate(model.stages()):
        if pool is not None:
            h = l2pool(h)
        for c in convs:
            h = c(h, act=ops.ACT_RELU)
        cs = DISTS_CHNS[s + 1]
        pair_moments(h[:N], h[N:], out=mom[:, off:off + cs])
        off += cs
    out = torch.empty(N, dtype=torch.float64, device=x.device)
    check(lib().dcvic_dists_score_f64(_p(mom), mom.stride(0), _p(alpha), _p(beta), N, off, _p(out), _stream()), "dists_score")
    return out


@torch.no_grad()
def lpips(model, x: Tensor, y: Tensor) -> Tensor:
    """LPIPS(x_n, y_n) for each n (lpips v0.1, alex, linear heads, spatial mean, summed over the 5 taps): x, y fp32 [N, 3, H, W] RGB
    in [-1, 1] on the current device -> fp64 [N] on the device.  `model`: a LPIPSAlex (load_lpips)."""
    from .train import autograd as A
    from .train.lpips import CHNS, features
    xy, N = _pair_batch(x, y, "lpips")
    feats = [f.data for f in features(A.Ctx([]), model, A.const(xy))]
    taps = len(feats)
    mom = torch.empty((N, taps, 5), dtype=torch.float64, device=x.device)
    for k, f in enumerate(feats):
        _, Cc, H, W = f.shape
        assert Cc == CHNS[k]
        w = getattr(model, f"lin{k}").model[1].weight.detach().reshape(-1).contiguous()
        pix = torch.empty((N, 1, H, W), dtype=torch.float32, device=x.device)
        f = f if f.is_contiguous() else A._dense(f)
        check(lib().dcvic_lpips_tap_f32(_p(f[:N]), _p(f[N:]), _p(w), _p(pix), None, N, Cc, H * W, 0.0, _stream()), "lpips_tap")
        pair_moments(pix, pix, out=mom[:, k:k + 1])           # spatial mean = mu_x of the map with itself (read once)
    out = torch.empty(N, dtype=torch.float64, device=x.device)
    check(lib().dcvic_lpips_score_f64(_p(mom), N, taps, _p(out), _stream()), "lpips_score")
    return out


# ------------------------------------------------------------------------------------------------ MS-SSIM and PSNR
MSSSIM_MIN_SIDE = 161          # pytorch-msssim 0.2.1 asserts min(H, W) > (win_size - 1) * 2**4


def msssim_psnr_sse(x: Tensor, y: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(ms_ssim [N], psnr [N], sse [N]) fp64 on the device for x, y contiguous fp32 [N, 3, H, W] in [-1, 1] (csrc/ssim.hip): the
    reference's calc_ms_ssim (pytorch-msssim 0.2.1 on trunc((v + 1) / 2 * 255), -1 where min(H, W) <= 160, which the package refuses
    and the reference reports as -1) and calc_psnr (10 log10(255^2 / mse) on the same integers; inf for identical images); sse is the
    exact squared-error sum of the integer planes."""
    N, Cc, H, W = _chk4(x, "ms_ssim x")
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError(f"ms_ssim_psnr: x and y differ in shape {tuple(x.shape)} vs {tuple(y.shape)}")
    _chk4(y, "ms_ssim y")
    if Cc != 3:
        raise ValueError(f"ms_ssim_psnr: need RGB images [N, 3, H, W], got {tuple(x.shape)}")
    if not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("ms_ssim_psnr: x and y must be contiguous")
    if y.device != x.device:
        raise ValueError(f"ms_ssim_psnr: x on {x.device}, y on {y.device}")
    full = min(H, W) >= MSSSIM_MIN_SIDE
    psnr = torch.empty(N, dtype=torch.float64, device=x.device)
    sse = torch.empty(N, dtype=torch.float64, device=x.device)
    ms = torch.empty(N, dtype=torch.float64, device=x.device) if full else torch.full((N,), -1.0, dtype=torch.float64, device=x.device)
    nb = int(lib().dcvic_msssim_workspace_bytes(N, Cc, H, W))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=x.device)
    check(lib().dcvic_msssim_psnr_f64(_p(x), _p(y), N, Cc, H, W, _p(ms) if full else None, _p(psnr), _p(sse), _p(ws), nb,
                                      _stream()), "msssim_psnr")
    return ms, psnr, sse


@torch.no_grad()
def ms_ssim_psnr(x: Tensor, y: Tensor) -> Tuple[Tensor, Tensor]:
    """(ms_ssim [N], psnr [N]) fp64 on the device; see msssim_psnr_sse."""
    ms, psnr, _ = msssim_psnr_sse(x, y)
    return ms, psnr
