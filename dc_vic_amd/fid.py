"""HiFiC patch FID on HIP kernels: the FID of the reference's scripts/calc_metrics.py:220-320 (FIDMetric) and
scripts/beta_selection.py (Eq. 13: score = alpha * PSNR - FID).

PARITY UNPINNED: the `pytorch_fid` package is not in the reference tree and can be neither fetched nor its weights downloaded.  Its
FIDInceptionV3 (`InceptionV3(output_blocks=[3])`: pool3, 2048-d) is restated here with torchvision's Inception3 module and parameter
names, so pytorch-fid's `pt_inception-2015-12-05-6726825d.pth` loads by key (`FIDInception.from_file`); `tests/test_fid_host.py` pins
the restatement as a plain-torch fp64 function with unfolded BatchNorm, which the GPU tests compare against.

Per patch (csrc/fid.hip, dcvic_fid_patch_resize_f32): ToTensor, F.interpolate(size=(299, 299), bilinear, align_corners=False), 2 x - 1.
Every BasicConv2d (conv without bias, BatchNorm2d(eps=0.001), ReLU) runs as one ConvPlan convolution whose weights and bias hold the
BatchNorm, folded in fp64 at load time and rounded to fp32, with the ReLU in the epilogue; each branch writes straight into its channel
slice of the block's concatenated output.  The pools are dcvic_fid_pool3_f32 / dcvic_fid_mean_hw_f32; the statistics (per-feature sums
and F^T F) accumulate in fp64 on the device (dcvic_fid_stats_accum_f64), so features never leave it.  A patch's features have the same
bits whichever patches share its batch.  The Frechet distance is pytorch-fid's calculate_frechet_distance (scipy, fp64, host)."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import check, lib
from .ops import _bs, _chk4, _p, _stream

Tensor = torch.Tensor

FID_DIMS = 2048
INCEPTION_SIZE = 299
BN_EPS = 0.001
POOL_MAX_S2, POOL_AVG, POOL_MAX_S1 = 0, 1, 2     # dcvic_fid_pool3_f32 modes
# keys of pytorch-fid's / torchvision's Inception3 state dict that FID-Inception does not use
OPTIONAL_PREFIXES = ("fc.", "AuxLogits.")
OPTIONAL_SUFFIX = "num_batches_tracked"


def _pair(v) -> Tuple[int, int]:
    return (v, v) if isinstance(v, int) else tuple(v)


class BasicConv2d(nn.Module):
    """torchvision's BasicConv2d: Conv2d(bias=False) -> BatchNorm2d(eps=0.001) -> ReLU, run as one fused convolution."""

    def __init__(self, in_ch: int, out_ch: int, kernel_size, stride: int = 1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(in_ch, out_ch, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_ch, eps=BN_EPS)
        self.conv.weight.requires_grad_(False)
        self.bn.weight.requires_grad_(False)
        self.bn.bias.requires_grad_(False)
        self.stride, self.pad = stride, _pair(padding)
        self._plan = None
        self._plan_key = None

    def folded(self) -> Tuple[Tensor, Tensor]:
        """(weight, bias) of conv -> BN as one convolution, on the module's device: scale = gamma / sqrt(var + eps) applied to the weight
        and beta - mean * scale as the bias, computed in fp64 and rounded to fp32 once."""
        bn = self.bn
        scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        w = self.conv.weight.detach().double() * scale.view(-1, 1, 1, 1)
        b = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
        return w.float().contiguous(), b.float().contiguous()

    def _key(self):
        ts = (self.conv.weight, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var)
        return tuple((t.data_ptr(), t._version, str(t.device)) for t in ts)

    def plan(self) -> ops.ConvPlan:
        k = self._key()
        if self._plan is None or self._plan_key != k:
            w, b = self.folded()
            self._plan = ops.ConvPlan(w, b, "conv", stride=self.stride, pad=self.pad)
            # Winograd where eligible (mostly not at these map sizes): no integer decision follows these layers
            self._plan.wino = tuple(w.shape[2:]) == (3, 3) and self.stride == 1 and self.pad == (1, 1)
            self._plan_key = k
        return self._plan

    def forward(self, x: Tensor, out: Optional[Tensor] = None) -> Tensor:
        return self.plan()(x, out=out, act=ops.ACT_RELU)


def _new(N: int, Cc: int, H: int, W: int, like: Tensor) -> Tensor:
    return torch.empty((N, Cc, H, W), dtype=torch.float32, device=like.device)


class InceptionA(nn.Module):
    """FIDInceptionA (Mixed_5b/5c/5d): [1x1 64, 5x5 64, 3x3dbl 96, avg pool (count_include_pad=False) + 1x1 pool_features]."""

    def __init__(self, in_ch: int, pool_features: int):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_ch, 64, 1)
        self.branch5x5_1 = BasicConv2d(in_ch, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_ch, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(in_ch, pool_features, 1)
        self.out_channels = 224 + pool_features

    def forward(self, x: Tensor) -> Tensor:
        N, _, H, W = x.shape
        out = _new(N, self.out_channels, H, W, x)
        self.branch1x1(x, out[:, 0:64])
        self.branch5x5_2(self.branch5x5_1(x), out[:, 64:128])
        self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)), out[:, 128:224])
        self.branch_pool(pool3(x, POOL_AVG), out[:, 224:])
        return out


class InceptionB(nn.Module):
    """InceptionB (Mixed_6a): [3x3 / s2 384, 3x3dbl (.. 3x3 / s2) 96, max pool 3 / s2]."""

    def __init__(self, in_ch: int):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_ch, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_ch, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)
        self.out_channels = 480 + in_ch

    def forward(self, x: Tensor) -> Tensor:
        N, Cc, H, W = x.shape
        out = _new(N, self.out_channels, (H - 3) // 2 + 1, (W - 3) // 2 + 1, x)
        self.branch3x3(x, out[:, 0:384])
        self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)), out[:, 384:480])
        pool3(x, POOL_MAX_S2, out=out[:, 480:])
        return out


class InceptionC(nn.Module):
    """FIDInceptionC (Mixed_6b..6e): [1x1 192, 7x7 (1x7, 7x1) 192, 7x7dbl (7x1, 1x7, 7x1, 1x7) 192, avg pool + 1x1 192]."""

    def __init__(self, in_ch: int, channels_7x7: int):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_ch, 192, 1)
        self.branch7x7_1 = BasicConv2d(in_ch, c7, 1)
        self.branch7x7_2 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_ch, c7, 1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_ch, 192, 1)
        self.out_channels = 768

    def forward(self, x: Tensor) -> Tensor:
        N, _, H, W = x.shape
        out = _new(N, 768, H, W, x)
        self.branch1x1(x, out[:, 0:192])
        self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)), out[:, 192:384])
        t = self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))
        self.branch7x7dbl_5(self.branch7x7dbl_4(t), out[:, 384:576])
        self.branch_pool(pool3(x, POOL_AVG), out[:, 576:768])
        return out


class InceptionD(nn.Module):
    """InceptionD (Mixed_7a): [1x1 192 -> 3x3 / s2 320, 1x1 192 -> 1x7 -> 7x1 -> 3x3 / s2 192, max pool 3 / s2]."""

    def __init__(self, in_ch: int):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_ch, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_ch, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)
        self.out_channels = 512 + in_ch

    def forward(self, x: Tensor) -> Tensor:
        N, Cc, H, W = x.shape
        out = _new(N, self.out_channels, (H - 3) // 2 + 1, (W - 3) // 2 + 1, x)
        self.branch3x3_2(self.branch3x3_1(x), out[:, 0:320])
        self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))), out[:, 320:512])
        pool3(x, POOL_MAX_S2, out=out[:, 512:])
        return out


class InceptionE(nn.Module):
    """FIDInceptionE_1 (Mixed_7b, avg pool with count_include_pad=False) / FIDInceptionE_2 (Mixed_7c, max pool 3 / s1 / p1):
    [1x1 320, 3x3 (1x3 | 3x1) 768, 3x3dbl (3x3, then 1x3 | 3x1) 768, pool + 1x1 192]."""

    def __init__(self, in_ch: int, max_pool: bool):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_ch, 320, 1)
        self.branch3x3_1 = BasicConv2d(in_ch, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_ch, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_ch, 192, 1)
        self.max_pool = max_pool
        self.out_channels = 2048

    def forward(self, x: Tensor) -> Tensor:
        N, _, H, W = x.shape
        out = _new(N, 2048, H, W, x)
        self.branch1x1(x, out[:, 0:320])
        t = self.branch3x3_1(x)
        self.branch3x3_2a(t, out[:, 320:704])
        self.branch3x3_2b(t, out[:, 704:1088])
        t = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        self.branch3x3dbl_3a(t, out[:, 1088:1472])
        self.branch3x3dbl_3b(t, out[:, 1472:1856])
        self.branch_pool(pool3(x, POOL_MAX_S1 if self.max_pool else POOL_AVG), out[:, 1856:2048])
        return out


class FIDInception(nn.Module):
    """pytorch-fid's FIDInceptionV3 up to pool3 (blocks 0-3 of InceptionV3(output_blocks=[3])), with torchvision Inception3 names."""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, 3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, 3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, 1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, 3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, max_pool=False)
        self.Mixed_7c = InceptionE(2048, max_pool=True)

    def convs(self) -> "OrderedDict[str, BasicConv2d]":
        return OrderedDict((n, m) for n, m in self.named_modules() if isinstance(m, BasicConv2d))

    @staticmethod
    def manifest() -> "OrderedDict[str, Tuple[int, ...]]":
        """The keys and shapes FID-Inception needs from a state dict (num_batches_tracked, fc.* and AuxLogits.* are optional)."""
        return OrderedDict((k, tuple(v.shape)) for k, v in FIDInception().state_dict().items() if not k.endswith(OPTIONAL_SUFFIX))

    # ------------------------------------------------------------------------------------------ constructors
    @classmethod
    def from_state_dict(cls, sd: Dict[str, Tensor]) -> "FIDInception":
        """Strict load by key and shape: any key outside the manifest except fc.*, AuxLogits.* and *.num_batches_tracked, any missing
        key and any shape mismatch raises ValueError naming the key."""
        if not isinstance(sd, dict):
            raise ValueError(f"Inception weights: expected a state dict, got {type(sd).__name__}")
        m = cls()
        want = m.manifest()
        for k in sd:
            if k not in want and not k.startswith(OPTIONAL_PREFIXES) and not k.endswith(OPTIONAL_SUFFIX):
                raise ValueError(f"Inception state dict: unexpected key {k!r}")
        own = m.state_dict()
        for k, shape in want.items():
            if k not in sd:
                raise ValueError(f"Inception state dict lacks {k!r}")
            v = sd[k]
            if not isinstance(v, torch.Tensor) or tuple(v.shape) != shape:
                got = tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__
                raise ValueError(f"Inception state dict: {k} has shape {got}, expected {shape}")
            own[k].copy_(v.to(dtype=own[k].dtype))
        return m

    @classmethod
    def from_file(cls, path: str) -> "FIDInception":
        """pytorch-fid's pt_inception-2015-12-05-6726825d.pth (or any Inception3-named state dict), torch.load(weights_only=True)."""
        return cls.from_state_dict(torch.load(path, map_location="cpu", weights_only=True))

    @classmethod
    def synthetic(cls, seed: int = 0) -> "FIDInception":
        """Deterministic synthetic weights (tests and benchmarks only): He-normal convs, and BatchNorm statistics with
        gamma / sqrt(var + eps) ~ 1 and small shifts, so the activations stay O(1) through all 94 convolutions."""
        m = cls()
        g = torch.Generator().manual_seed(3000 + seed)
        for c in m.convs().values():
            w = c.conv.weight
            fan_in = w.shape[1] * w.shape[2] * w.shape[3]
            w.data.copy_(torch.randn(w.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            n = w.shape[0]
            var = 0.5 + torch.rand(n, generator=g)
            c.bn.running_var.copy_(var)
            c.bn.running_mean.copy_(0.05 * torch.randn(n, generator=g))
            c.bn.weight.data.copy_(torch.sqrt(var + BN_EPS) * (0.9 + 0.2 * torch.rand(n, generator=g)))
            c.bn.bias.data.copy_(0.05 * torch.randn(n, generator=g))
        return m

    # ------------------------------------------------------------------------------------------ forward
    @torch.no_grad()
    def features(self, x: Tensor, out: Optional[Tensor] = None) -> Tensor:
        """pool3 features [N, 2048] (fp32, on the device) of network inputs x [N, 3, 299, 299] (already resized and in [-1, 1])."""
        N, Cc, H, W = _chk4(x, "fid features x")
        if Cc != 3:
            raise ValueError(f"fid features: need [N, 3, H, W] inputs, got {tuple(x.shape)}")
        h = self.Conv2d_1a_3x3(x)
        h = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(h))
        h = pool3(h, POOL_MAX_S2)
        h = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(h))
        h = pool3(h, POOL_MAX_S2)
        for blk in (self.Mixed_5b, self.Mixed_5c, self.Mixed_5d, self.Mixed_6a, self.Mixed_6b, self.Mixed_6c, self.Mixed_6d,
                    self.Mixed_6e, self.Mixed_7a, self.Mixed_7b, self.Mixed_7c):
            h = blk(h)
        return mean_hw(h, out=out)


def conv_layer_shapes(size: int = INCEPTION_SIZE):
    """(name, Cin, Cout, KH, KW, stride, H_in, H_out) of every convolution at a size x size input, in execution order.  Inside a block every
    conv reads the block's input size (the stride-2 convs end their branches); the stem convs and the two max pools chain."""
    m = FIDInception()
    rows = []

    def add(name: str, c: BasicConv2d, H: int) -> int:
        kh, kw = c.conv.kernel_size
        Ho = (H + 2 * c.pad[0] - kh) // c.stride + 1
        rows.append((name, c.conv.in_channels, c.conv.out_channels, kh, kw, c.stride, H, Ho))
        return Ho

    H = size
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", None, "Conv2d_3b_1x1", "Conv2d_4a_3x3", None):
        H = (H - 3) // 2 + 1 if name is None else add(name, getattr(m, name), H)
    for bname, blk in m.named_children():
        if not bname.startswith("Mixed_"):
            continue
        Ho = H
        for cname, c in blk.named_children():
            r = add(f"{bname}.{cname}", c, H)
            Ho = r if c.stride == 2 else Ho
        H = Ho
    return rows


# ------------------------------------------------------------------------------------------------ kernels
def pool3(x: Tensor, mode: int, out: Optional[Tensor] = None) -> Tensor:
    """The Inception pools (dcvic_fid_pool3_f32): POOL_MAX_S2 = MaxPool2d(3, 2), POOL_AVG = avg_pool2d(3, 1, 1, count_include_pad=False),
    POOL_MAX_S1 = max_pool2d(3, 1, 1).  x and `out` may be channel-slice views (dense planes, any batch stride)."""
    N, Cc, H, W = _chk4(x, "fid pool x")
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == POOL_MAX_S2 else (H, W)
    if out is None:
        out = _new(N, Cc, Ho, Wo, x)
    if tuple(_chk4(out, "fid pool out")) != (N, Cc, Ho, Wo):
        raise ValueError(f"fid pool: out shape {tuple(out.shape)} != {(N, Cc, Ho, Wo)}")
    check(lib().dcvic_fid_pool3_f32(mode, _p(x), _bs(x), N, Cc, H, W, _p(out), _bs(out), _stream()), "fid_pool3")
    return out


def mean_hw(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Global average pool: [N, C, H, W] -> [N, C] (dcvic_fid_mean_hw_f32); `out` may be a row-strided [N, C] view."""
    N, Cc, H, W = _chk4(x, "fid mean x")
    if out is None:
        out = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    if out.dtype != torch.float32 or out.device != x.device or tuple(out.shape) != (N, Cc) or (Cc > 1 and out.stride(1) != 1):
        raise ValueError(f"fid mean: out must be an fp32 [{N}, {Cc}] view with unit column stride on {x.device}")
    ys = out.stride(0) if N > 1 else Cc
    check(lib().dcvic_fid_mean_hw_f32(_p(x), _bs(x), N, Cc, H * W, _p(out), ys, _stream()), "fid_mean_hw")
    return out


def patch_inputs(img: Tensor, origins: Tensor, ph: int, pw: Optional[int] = None, out: Optional[Tensor] = None,
                 size: int = INCEPTION_SIZE) -> Tensor:
    """Network inputs [B, 3, size, size] of the ph x pw patches of `img` (u8 [H, W, 3] on the device) at `origins` (int32 [B, 2] of
    (y0, x0) on the device, checked against the image by the caller: see `check_origins`), as pytorch-fid sees them:
    ToTensor, F.interpolate(size, bilinear, align_corners=False), 2 x - 1.  `out` may be a batch slice of a larger input buffer."""
    pw = ph if pw is None else pw
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous() or not img.is_cuda:
        raise ValueError(f"fid patch_inputs: img must be a contiguous u8 [H, W, 3] device tensor, got {img.dtype} {tuple(img.shape)}")
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or not origins.is_contiguous() \
            or origins.device != img.device:
        raise ValueError("fid patch_inputs: origins must be a contiguous int32 [B, 2] tensor on the image's device")
    B = origins.shape[0]
    H, W = img.shape[:2]
    if out is None:
        out = torch.empty((B, 3, size, size), dtype=torch.float32, device=img.device)
    if tuple(_chk4(out, "fid patch out")) != (B, 3, size, size):
        raise ValueError(f"fid patch_inputs: out shape {tuple(out.shape)} != {(B, 3, size, size)}")
    check(lib().dcvic_fid_patch_resize_f32(_p(img), H, W, _p(origins), B, ph, pw, size, _p(out), _bs(out), _stream()), "fid_patch_resize")
    return out


def check_origins(origins: np.ndarray, H: int, W: int, ph: int, pw: int) -> np.ndarray:
    """The (y0, x0) rows as a contiguous int32 array, after checking that every patch lies inside the H x W image."""
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.int64).reshape(-1, 2))
    if len(o) and (o.min() < 0 or (o[:, 0] + ph).max() > H or (o[:, 1] + pw).max() > W):
        raise ValueError(f"fid: a {ph} x {pw} patch origin lies outside the {H} x {W} image")
    return o.astype(np.int32)


class FIDStats:
    """Running fp64 feature statistics on the device: n, sum_b f_b and the upper triangle of sum_b f_b f_b^T."""

    def __init__(self, device, dims: int = FID_DIMS):
        self.dims = dims
        self.n = 0
        self.sum = torch.zeros(dims, dtype=torch.float64, device=device)
        self.gram = torch.zeros((dims, dims), dtype=torch.float64, device=device)

    def add(self, feats: Tensor) -> None:
        """Accumulate a batch of fp32 features [B, dims] (row-strided views allowed)."""
        if feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.dims or feats.device != self.sum.device \
                or (self.dims > 1 and feats.stride(1) != 1):
            raise ValueError(f"FIDStats.add: need fp32 [B, {self.dims}] features with unit column stride on {self.sum.device}")
        B = feats.shape[0]
        if B == 0:
            return
        check(lib().dcvic_fid_stats_accum_f64(_p(feats), feats.stride(0) if B > 1 else self.dims, B, self.dims, _p(self.sum),
                                              _p(self.gram), _stream()), "fid_stats_accum")
        self.n += B

    def mu_sigma(self) -> Tuple[np.ndarray, np.ndarray]:
        """(mu, sigma) as np.mean / np.cov(rowvar=False) define them: mu = sum / n, sigma = (G - n mu mu^T) / (n - 1), in fp64."""
        if self.n < 2:
            raise ValueError(f"FID statistics need at least 2 patches, got {self.n}")
        s = self.sum.cpu().numpy()
        g = np.triu(self.gram.cpu().numpy())
        g = g + np.triu(g, 1).T
        mu = s / self.n
        sigma = (g - self.n * np.outer(mu, mu)) / (self.n - 1)
        return mu, sigma


def frechet_distance(mu1: np.ndarray, sigma1: np.ndarray, mu2: np.ndarray, sigma2: np.ndarray, eps: float = 1e-6) -> float:
    """pytorch-fid's calculate_frechet_distance, step for step: ||mu1 - mu2||^2 + tr(sigma1) + tr(sigma2) - 2 tr sqrtm(sigma1 sigma2),
    retrying with eps * I added to both sigmas when sqrtm is not finite; a complex result with a diagonal imaginary part above 1e-3
    raises ValueError, a smaller one keeps the real part.  scipy (1.15: sqrtm(A, disp=True, blocksize=64)) is imported here only."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError("frechet_distance: the two statistics differ in dimension")
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


class PatchFeatures:
    """Streams patches of device images through the network in batches of up to `batch` patches, filled across images, into an
    FIDStats (or any callable taking [B, 2048] feature batches).  One upload per image; no per-patch host work."""

    def __init__(self, model: FIDInception, device, batch: int = 100, patch: int = 256):
        self.model, self.device, self.batch, self.patch = model, torch.device(device), batch, patch
        self.buf = torch.empty((batch, 3, INCEPTION_SIZE, INCEPTION_SIZE), dtype=torch.float32, device=self.device)
        self.feats = torch.empty((batch, FID_DIMS), dtype=torch.float32, device=self.device)
        self.fill = 0
        self.sink = None

    def _flush(self) -> None:
        if self.fill:
            f = self.model.features(self.buf[:self.fill], out=self.feats[:self.fill])
            self.sink(f)
            self.fill = 0

    def run(self, images: Iterable[Tuple[np.ndarray, np.ndarray]], sink) -> int:
        """images: (u8 [H, W, 3] host array, (y0, x0) origins [n, 2]) pairs.  Returns the number of patches."""
        self.sink, total = sink, 0
        p = self.patch
        for img, origins in images:
            H, W = img.shape[:2]
            o = check_origins(origins, H, W, p, p)
            if not len(o):
                continue
            dimg = torch.from_numpy(np.require(img, np.uint8, ["C", "W"])).to(self.device)
            dorg = torch.from_numpy(o).to(self.device)
            i = 0
            while i < len(o):
                k = min(len(o) - i, self.batch - self.fill)
                patch_inputs(dimg, dorg[i:i + k], p, out=self.buf[self.fill:self.fill + k])
                self.fill += k
                i += k
                if self.fill == self.batch:
                    self._flush()
            total += len(o)
        self._flush()
        return total

    def statistics(self, images: Iterable[Tuple[np.ndarray, np.ndarray]]) -> FIDStats:
        st = FIDStats(self.device)
        self.run(images, st.add)
        return st
