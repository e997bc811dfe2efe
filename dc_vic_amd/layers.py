"""Parameter-holding building blocks whose forward passes are HIP kernels.

Each class keeps the parameter names / shapes of the torch.nn layer it stands in for (so the
reference's checkpoints load by key), but `forward` dispatches to the C ABI through dc_vic_amd.ops.
Weights are packed into the MFMA tile layout lazily and re-packed if a parameter changes
(load_state_dict, .to(device)).  Inference only: no autograd graph is built.
"""
from __future__ import annotations

import math
import operator
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops

Tensor = torch.Tensor
_VERSION = operator.attrgetter("_version")


class WeightFingerprint:
    """Identity of the weights under some modules: (tensor object, storage address, version) of every parameter and buffer.  It moves
    when torch can see the change -- load_state_dict, an in-place op on the parameter (p.copy_, p.add_, an optimiser step), a parameter
    replaced by a new one, .to(device), `p.data = other` -- and does NOT move under a write torch cannot see: `p.data.copy_()` or a
    raw-pointer write (a HIP kernel on p.data_ptr()) leave p._version where it was.  Those routes need invalidate_weight_caches().
    The modules' parameter / buffer dicts are gathered once (a replaced submodule is not followed) and read again by every call; the
    tensors of the last call are held, so a freed parameter's address cannot come back under a new one.  ~0.3 us per tensor."""

    def __init__(self, modules: Sequence[nn.Module]):
        seen, self._dicts = set(), []
        for root in modules:
            for m in root.modules():
                if id(m) not in seen:
                    seen.add(id(m))
                    self._dicts += [d for d in (m._parameters, m._buffers) if d]
        self._held = []

    def __call__(self) -> tuple:
        ts = self._held = [t for d in self._dicts for t in d.values() if t is not None]
        return tuple(map(id, ts)), tuple(map(Tensor.data_ptr, ts)), tuple(map(_VERSION, ts))


# Every cache in the package that holds a copy of (or a pointer into a copy of) some weights, by the attribute it lives in on its module,
# with the value that means "empty".  A new cache goes in here: invalidate_weight_caches is the one place that drops them all.
WEIGHT_CACHE_ATTRS = {
    "_plan": None,          # _Packed: the packed ConvPlan (also fid.FrozenConv)
    "_plain_plan": None,    # train/autograd.conv: the fp32 plan of a frozen layer
    "_dgrad": None,         # train/autograd.conv: the data-gradient plan (flipped / transposed copy)
    "_qkv_plan": None,      # vqgan.AttnBlock: q/k/v as one convolution
    "_rest_key": None,      # charm.SliceTransform: first conv without its hyperprior channels
    "_rest": None,
    "_hp_key": None,        # charm.Minnen20CharmContextModel: stacked hyperprior partial convolutions
    "_hp_mean": None,
    "_hp_scale": None,
    "_packs": None,         # entropy.EntropyBottleneck: softplus / tanh'd matrices
}


def invalidate_weight_caches(module: nn.Module) -> None:
    """Drop everything derived from the weights under `module`: packed convolution plans, fused q/k/v packs, CHARM's split plans, the
    entropy bottleneck's packs, cached beta vectors (`_vec_cache`) and captured hipGraphs (`_graphs`).  Needed after a write torch does
    not version (`p.data` / raw pointer, e.g. the fused Adam kernel); every torch-visible route is detected without it
    (WeightFingerprint).  The integer CDF tables of the entropy models are state, not cache: they are rebuilt by codec_setup()."""
    for m in module.modules():
        d = m.__dict__
        for name, empty in WEIGHT_CACHE_ATTRS.items():
            if d.get(name, empty) is not empty:
                d[name] = empty
        if "_vec_cache" in d:
            m.invalidate_caches()
        if "_graphs" in d:
            m._graphs.clear()


def copy_kernel_flags(plan, layer, wino: bool = True, bf16: bool = False):
    """The kernel families `layer` opted into (allow_winograd, allow_bf16), copied to a plan made from its weights -- the one place that
    does it.  `wino=False`: the plan is not a Conv2d(k3, s1, p1); `bf16` is passed by inference only.  (F(4x4) counts only where F(2x2)
    does: ConvPlan never looks at wino44 without wino.)"""
    plan.wino = wino and bool(getattr(layer, "wino", False))
    plan.wino44 = plan.wino and bool(getattr(layer, "wino44", False))
    plan.bf16 = bf16 and bool(getattr(layer, "bf16", False)) and not getattr(layer, "bf16_keep_fp32", False)
    return plan


class _Packed(nn.Module):
    def __init__(self):
        super().__init__()
        self._plan = None
        self._plan_key = None

    def _key(self):
        return tuple((p.data_ptr(), p._version, str(p.device)) for p in self.parameters(recurse=False))

    def _get_plan(self, bf16: bool = True):
        """`bf16=False`: the plan runs fp32 whatever allow_bf16 set (training: train/autograd.conv)."""
        k = self._key()
        if self._plan is None or self._plan_key != k:
            self._plan = self._build_plan()
            self._plan_key = k
        return copy_kernel_flags(self._plan, self, bf16=bf16)

    def _build_plan(self):
        raise NotImplementedError


class Conv2d(_Packed):
    """torch.nn.Conv2d(in, out, k, stride, padding) stand-in (weight [out, in, k, k], bias [out]).

    `asym_pad`: ldm Downsample semantics -- F.pad(x, (0,1,0,1)) then a pad-0 stride-2 conv (model.py:72-76).
    `upsample`: ldm Upsample semantics -- nearest x2 before the conv (model.py:53-57), fused in the loader.
    """

    def __init__(self, in_ch: int, out_ch: int, kernel_size: int, stride: int = 1, padding: int = 0, bias: bool = True,
                 asym_pad: bool = False, upsample: bool = False):
        super().__init__()
        self.in_channels, self.out_channels = in_ch, out_ch
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.asym_pad, self.upsample = asym_pad, upsample
        self.wino = False     # allow_winograd(): set only where no integer decision depends on this layer's exact bits
        self.wino44 = False   # allow_winograd(f44=True): F(4x4, 3x3) too -- only AFTER the path's last integer decision
        self.bf16 = False     # allow_bf16(): the bf16-MFMA kernel (decoder precision "bf16"), same layers as wino44
        self.bf16_keep_fp32 = False   # set by the owner: a marked layer whose bf16 rounding costs too much fidelity stays fp32
        self.weight = nn.Parameter(torch.empty(out_ch, in_ch, kernel_size, kernel_size), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_ch), requires_grad=False) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1 / math.sqrt(in_ch * kernel_size * kernel_size)
            nn.init.uniform_(self.bias, -bound, bound)

    def _build_plan(self):
        pad = (0, 0) if self.asym_pad else (self.padding, self.padding)
        return ops.ConvPlan(self.weight, self.bias, "conv", stride=self.stride, pad=pad, upsample=self.upsample)

    def forward(self, x, act: int = ops.ACT_NONE, res: Optional[Tensor] = None, affine=None, out: Optional[Tensor] = None,
                gn_stats: bool = False) -> Tensor:
        """`gn_stats`: a GroupNorm over exactly this output follows; its statistics come out of this launch's epilogue when it runs on the
        F(4x4) kernel (take them with `take_gn_part()`, None otherwise -- the GroupNorm then makes its own pass)."""
        plan = self._get_plan()
        out_hw = None
        if self.asym_pad:
            src0 = x if isinstance(x, Tensor) else x[0]
            H, W = src0.shape[2:]
            out_hw = ((H + 1 - self.kernel_size) // self.stride + 1, (W + 1 - self.kernel_size) // self.stride + 1)
        y = plan(x, out=out, act=act, res=res, affine=affine, out_hw=out_hw, gn_stats=gn_stats)
        self._gn_part = plan.last_gn_part
        return y

    def take_gn_part(self):
        p, self._gn_part = getattr(self, "_gn_part", None), None
        return p


def allow_winograd(module: nn.Module, on: bool = True, f44: bool = False) -> nn.Module:
    """Let every Conv2d(k3, s1, p1) under `module` run as Winograd F(2x2, 3x3) (csrc/wino.hip) when the launch is eligible; with
    `f44` also as F(4x4, 3x3) (csrc/wino44.hip: 2.25 instead of 4 multiplies per output, ~3x the rounding error -- 1.5e-6 rms relative
    per layer).  `f44` is passed ONLY by the frozen VQGAN decoder and the SFT fusion blocks, the layers after the estimator's argmax,
    where nothing but the reconstruction's fp tolerance (contract 1e-3, measured in tests/parity_util.py) depends on the bits; never by
    the encoder side, whose bits feed the VQ argmin and the symbol rounding.  `DCVIC_WINO44=0` keeps those layers on F(2x2).

    Winograd re-associates the sum (1e-6 relative against the direct fmaf chain; closer to fp64 than the direct chain).  Callers:
      * the frozen VQGAN decoder and the SFT fusion blocks -- the layers after the path's last integer decision (the estimator
        argmax): bitstreams and indices cannot change, only the reconstruction at the 1e-5 level;
      * the VQGAN ENCODER (vqgan.Encoder, default on, `DCVIC_WINO_ENCODER=0` for the direct kernels) -- upstream of the VQ argmin
        and, through the one-hot feature, of the y symbols.  Deterministic and batch-invariant, so encoder and decoder of THIS
        build always agree; against the oracle / reference it can move a VQ index or a symbol that sits on an fp32 near-tie
        (as any other fp32 summation order would): the parity tests itemise and bound such near-ties, and measured on the test
        set it adds none over the direct kernels.  Its 4-channel conv_out stays direct.
    Hyperprior, CHARM, both ELIC networks and the estimator keep the layer-defined reduction order (never called for them)."""
    for m in module.modules():
        if isinstance(m, Conv2d) and m.kernel_size == 3 and m.stride == 1 and m.padding == 1 and not m.asym_pad:   # (incl. the Upsample convs)
            m.wino = on
            m.wino44 = bool(on and f44)
    return module


def allow_bf16(module: nn.Module, on: bool = True) -> nn.Module:
    """Let every Conv2d(k3, s1, p1) under `module`, the Upsample convs included, run on the bf16-MFMA kernel (csrc/conv_bf16.hip: bf16
    operands, fp32 accumulation) when the launch is eligible -- the layers allow_winograd(f44=True) marks.  Called ONLY through
    set_decoder_precision for the frozen VQGAN decoder and the SFT fusion blocks, after the estimator's argmax: bitstreams, indices,
    symbols and logits cannot move, only the reconstruction (contract: >= 50 dB PSNR against the fp32 reconstruction).  Never for the
    encoder, the hyperprior, CHARM, the ELIC decoder or the estimator.  A launch the kernel does not take stays on the fp32 kernels."""
    for m in module.modules():
        if isinstance(m, Conv2d) and m.kernel_size == 3 and m.stride == 1 and m.padding == 1 and not m.asym_pad:
            m.bf16 = bool(on)
    return module


class ConvTranspose2d(_Packed):
    """torch.nn.ConvTranspose2d stand-in for the two shapes on the path (weight [in, out, k, k]):
    (k5, s2, p2, output_padding 1) -- elic_autoencoder.py:21-28, minnen20_hyperprior.py:46-48 -- and (k3, s1, p1)."""

    def __init__(self, in_ch: int, out_ch: int, kernel_size: int, stride: int, padding: int, output_padding: int = 0):
        super().__init__()
        if (kernel_size, stride, padding, output_padding) not in ((5, 2, 2, 1), (3, 1, 1, 0)):
            raise NotImplementedError("ConvTranspose2d: only (k5,s2,p2,op1) and (k3,s1,p1) are on the DC-VIC path")
        self.in_channels, self.out_channels, self.kernel_size = in_ch, out_ch, kernel_size
        self.weight = nn.Parameter(torch.empty(in_ch, out_ch, kernel_size, kernel_size), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_ch), requires_grad=False)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        nn.init.zeros_(self.bias)

    def _build_plan(self):
        return ops.ConvPlan(self.weight, self.bias, "convT")

    def forward(self, x, act: int = ops.ACT_NONE, out: Optional[Tensor] = None) -> Tensor:
        return self._get_plan()(x, out=out, act=act)


class Linear(_Packed):
    """torch.nn.Linear stand-in applied to NCHW maps as a 1x1 convolution (weight [out, in])."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_features), requires_grad=False) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            nn.init.zeros_(self.bias)

    def _build_plan(self):
        return ops.ConvPlan(self.weight, self.bias, "conv")

    def forward(self, x: Tensor, act: int = ops.ACT_NONE, res: Optional[Tensor] = None) -> Tensor:
        """x: [N, in, H, W] map (a [B, in] matrix is passed as [B, in, 1, 1])."""
        return self._get_plan()(x, act=act, res=res)


class GroupNorm(nn.Module):
    """GroupNorm(32, C, eps 1e-6, affine) (+ fused activation)."""

    def __init__(self, num_channels: int, num_groups: int = 32, eps: float = 1e-6):
        super().__init__()
        self.num_groups, self.eps = num_groups, eps
        self.weight = nn.Parameter(torch.ones(num_channels), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(num_channels), requires_grad=False)

    def forward(self, x: Tensor, act: int = ops.ACT_NONE, out: Optional[Tensor] = None, part=None) -> Tensor:
        return ops.groupnorm(x, self.weight, self.bias, self.num_groups, self.eps, act, out, part=part)


class LayerNormC(nn.Module):
    """nn.LayerNorm(C) of the token view, evaluated on the NCHW map."""

    def __init__(self, dim: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(dim), requires_grad=False)

    def forward(self, x: Tensor) -> Tensor:
        return ops.layernorm_c(x, self.weight, self.bias, self.eps)


class BatchNorm2d(nn.Module):
    """torch.nn.BatchNorm2d(num_features, eps, momentum) stand-in with torch's state-dict entries (weight, bias, running_mean,
    running_var, int64 num_batches_tracked).  It has a training forward only, on the tape (train/autograd.batch_norm, csrc/bn_train.hip):
    the normalised GAN discriminators never run in eval mode."""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = int(num_features), float(eps), float(momentum)
        self.weight = nn.Parameter(torch.ones(num_features), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(num_features), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        raise RuntimeError("BatchNorm2d runs on the training tape only (train/autograd.batch_norm)")


class ActNorm(nn.Module):
    """taming's ActNorm(num_features) stand-in (taming/modules/util.py:10-69, logdet not built): loc and scale [1, C, 1, 1] and the
    uint8 buffer `initialized`.  The first training call sets loc = -mean and scale = 1 / (std_unbiased + 1e-6) from its batch
    (train/autograd.act_norm).  The flag lives on the device for the state dict; the host reads it once, and again after a
    load_state_dict, never per step."""

    def __init__(self, num_features: int):
        super().__init__()
        self.num_features = int(num_features)
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1), requires_grad=False)
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1), requires_grad=False)
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))
        self._initialized_host: Optional[bool] = None
        self.flag_reads = 0          # device reads of the flag so far (tests)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._initialized_host = None

    def is_initialized(self) -> bool:
        if self._initialized_host is None:
            self._initialized_host = bool(self.initialized.item())
            self.flag_reads += 1
        return self._initialized_host

    def mark_initialized(self) -> None:
        self.initialized.fill_(1)
        self._initialized_host = True

    def forward(self, x):
        raise RuntimeError("ActNorm runs on the training tape only (train/autograd.act_norm)")


class Act(nn.Module):
    """Placeholder that keeps nn.Sequential indices aligned with the reference (activations are fused)."""

    def forward(self, x):
        raise RuntimeError("activation placeholders are fused into the neighbouring kernel")
