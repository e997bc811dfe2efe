"""The initialisation a stage 1-1 run starts from: every trainable tensor of the unconditioned model redrawn by the rule the reference's
constructors apply to it, from one seeded generator.

The constructors of dc_vic_amd/layers.py are stand-ins for checkpoints to be loaded into: they zero some biases torch draws, and other
code draws from the same stream, so they stay as they are and reference_init_ runs after build_comp_model.  Rules, per module:
  Conv2d, ConvTranspose2d, Linear   torch's defaults: weight kaiming_uniform_(a=sqrt(5)) = U(-1/sqrt(fan_in), 1/sqrt(fan_in)), bias from the
                                    same interval; fan_in = weight.shape[1] x kernel area (for ConvTranspose2d that is out_ch x k x k)
  GroupNorm, LayerNorm              weight 1, bias 0
  relative_position_bias_table      trunc_normal_(std=.02)                                   (swinir_layers.py:114)
  encoder.projection                with proj_init: trunc_normal_(std=proj_init_std), bias 0 (elic_insert_encoder.py:74-76)
  fusion_module                     with weight_init: trunc_normal_(std=weight_init_std), bias 0 on every convolution (vq_fusion_module.py:55-68)
  EntropyBottleneck                 its own values: matrices log(expm1(1 / scale / filters)), biases U(-0.5, 0.5), factors 0,
                                    quantiles (-init_scale, 0, init_scale)
The estimator is built from RSTB blocks directly, not through the SwinIR class whose `_init_weights` (swinir_layers.py:769-776) would give
its Linear layers trunc_normal_(.02) and zero biases: they keep torch's defaults, as in the reference; LayerNorm is 1 / 0 either way.
The truncated normals are cut at +-2 std.  (timm's trunc_normal_ takes its cut-offs a = -2, b = 2 in absolute units, which at std .02
never bind; the cut at two standard deviations is the documented rule, and only the Swin bias tables use it with the shipped config.)
`vq_model.*` is frozen and left alone."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from ..entropy import EntropyBottleneck
from ..layers import Conv2d, ConvTranspose2d, GroupNorm, LayerNormC, Linear

TRUNC_STD_CUT = 2.0      # the truncated normals' cut-off, in standard deviations


def _uniform_(p: torch.Tensor, bound: float, g: torch.Generator) -> None:
    p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound)


def _trunc_normal_(p: torch.Tensor, std: float, g: torch.Generator) -> None:
    t = torch.empty(p.shape, dtype=torch.float32)
    nn.init.trunc_normal_(t, 0.0, std, -TRUNC_STD_CUT * std, TRUNC_STD_CUT * std, generator=g)
    p.copy_(t)


def init_rule(model, name: str, module: nn.Module) -> str:
    """The rule for the parameters `module` (named `name` in `model`) owns directly: "torch", "trunc:<std>", "norm", "table",
    "bottleneck", or "" for a module that owns none."""
    if isinstance(module, EntropyBottleneck):
        return "bottleneck"
    if isinstance(module, (GroupNorm, LayerNormC)):
        return "norm"
    if hasattr(module, "relative_position_bias_table"):
        return "table"
    if isinstance(module, (Conv2d, ConvTranspose2d, Linear)):
        enc = model.encoder
        if name == "encoder.projection" and getattr(enc, "proj_init", False):
            return f"trunc:{enc.proj_init_std!r}"
        fm = model.fusion_module
        if name.startswith("fusion_module.") and getattr(fm, "weight_init", False):
            return f"trunc:{fm.weight_init_std!r}"
        return "torch"
    return ""


@torch.no_grad()
def reference_init_(model, generator: torch.Generator) -> Dict[str, str]:
    """Redraw every trainable tensor of the unconditioned `model` (everything but `vq_model.*`) in place, in named_modules order, from
    the CPU `generator` -> {parameter name: rule}.  Two calls with generators in equal states give equal bits.  ValueError for a
    beta-conditioned model (its conditioning modules have initialisation rules of their own, not restated here) and for a parameter
    no rule covers."""
    if hasattr(model.encoder, "beta_ft_list") or hasattr(model.decoder, "beta_ft_list"):
        raise ValueError(f"reference_init_ initialises the unconditioned model of stage 1-1, not {type(model).__name__}")
    done: Dict[str, str] = {}
    for name, mod in model.named_modules():
        if name == "vq_model" or name.startswith("vq_model."):
            continue
        rule = init_rule(model, name, mod)
        own = {k: p for k, p in mod.named_parameters(recurse=False)}
        if not rule:
            if own:
                raise ValueError(f"reference_init_: no rule for {name} ({type(mod).__name__}: {sorted(own)})")
            continue
        if rule == "bottleneck":
            f = (1,) + mod.filters + (1,)
            scale = mod.init_scale ** (1 / (len(mod.filters) + 1))
            for i in range(len(mod.filters) + 1):
                own[f"_matrix{i}"].fill_(float(np.log(np.expm1(1 / scale / f[i + 1]))))
                _uniform_(own[f"_bias{i}"], 0.5, generator)
                if i < len(mod.filters):
                    own[f"_factor{i}"].zero_()
            own["quantiles"].copy_(torch.tensor([-mod.init_scale, 0.0, mod.init_scale]).repeat(mod.channels, 1, 1))
        elif rule == "norm":
            own["weight"].fill_(1.0); own["bias"].zero_()
        elif rule == "table":
            _trunc_normal_(own["relative_position_bias_table"], 0.02, generator)
        else:
            w = own["weight"]
            fan_in = w.shape[1] * (w[0, 0].numel() if w.dim() > 2 else 1)
            if rule == "torch":
                _uniform_(w, 1.0 / math.sqrt(fan_in), generator)
            else:
                _trunc_normal_(w, float(rule.split(":", 1)[1]), generator)
            if own.get("bias") is not None:
                if rule == "torch":
                    _uniform_(own["bias"], 1.0 / math.sqrt(fan_in), generator)
                else:
                    own["bias"].zero_()
        for k in own:
            done[f"{name}.{k}"] = rule
    model.invalidate_weight_caches()
    return done
