"""The code losses of the reference's `loss` section (src/losses/cross_entropy_loss.py) on the training tape, and the host-side
reading of that section (config/exp1_stage1_3.yaml:61-79): every entry's `type` and keywords are either honoured or refused
with the YAML key and the value -- none is read and dropped.  `read_loss_section` is pure: no GPU, no model."""
from __future__ import annotations

from typing import Any, Dict, Optional

from ..registry import LOSS_REGISTRY
from . import autograd as A

Tensor = Any


def check_focal_gamma(gamma) -> float:
    """gamma is 0 (plain cross entropy) or >= 1: for 0 < gamma < 1 the derivative of (1 - p_t)^gamma is unbounded at p_t = 1
    (torch's autograd returns NaN there), a negative gamma is unbounded in value."""
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"gamma: {gamma!r} is not a number")
    if not (g == 0.0 or g >= 1.0) or g == float("inf"):
        raise ValueError(f"gamma: {gamma} is not supported, it must be 0 or >= 1 (the gradient is unbounded at p_t = 1 for 0 < gamma < 1)")
    return g


@LOSS_REGISTRY.register()
class CrossEntropyLoss:
    """cross_entropy_loss.py:11-29: loss_weight * nn.CrossEntropyLoss()(logits [N, C, H, W], target [N, H, W]).  The value and the
    gradient come from dcvic_cross_entropy_f32 + reduce_loss, as the trainer's code loss always did."""

    def __init__(self, loss_weight: float, ce_kwargs: Optional[dict] = None, **extra):
        if extra:
            raise ValueError(f"CrossEntropyLoss: unknown keyword(s) {sorted(extra)}")
        if ce_kwargs:
            raise ValueError(f"ce_kwargs: {dict(ce_kwargs)} is not supported (class weights, ignore_index and label smoothing are not built): leave it empty")
        self.loss_weight = float(loss_weight)

    def __call__(self, ctx: A.Ctx, logits: A.Var, target: Tensor) -> Tensor:
        return A.cross_entropy_loss(ctx, logits, target, self.loss_weight)


@LOSS_REGISTRY.register()
class FocalCrossEntropyLoss:
    """cross_entropy_loss.py:32-53: loss_weight * reduce((1 - p_t)^gamma * CE) with reduction mean or sum, one pass of csrc/chan_ce.hip.
    `reduction: none` returns a per-position map for the per-sample beta weighting of the rate-distortion trainers: this class, which
    returns one value, refuses it -- train/rd_trainer.py forms that loss with A.focal_cross_entropy_loss_weighted and
    sample_loss_weights below.  The reference forwards further keywords to nn.CrossEntropyLoss, none of which is built."""

    def __init__(self, loss_weight: float, gamma: float, reduction: str = "mean", **kwargs):
        if kwargs:
            raise ValueError(f"FocalCrossEntropyLoss: unknown keyword(s) {sorted(kwargs)} (nn.CrossEntropyLoss options are not built)")
        if reduction not in ("mean", "sum"):
            why = "needs the per-sample weighting of the rate-distortion trainers, which are not built" if reduction == "none" else "is unknown"
            raise ValueError(f"reduction: {reduction} {why}; use mean or sum")
        self.loss_weight, self.gamma, self.reduction = float(loss_weight), check_focal_gamma(gamma), reduction

    def __call__(self, ctx: A.Ctx, logits: A.Var, target: Tensor) -> Tensor:
        return A.focal_cross_entropy_loss(ctx, logits, target, self.loss_weight, self.gamma, self.reduction)


@LOSS_REGISTRY.register()
class RateLoss:
    """rate_loss.py:11-24: loss_weight * reduce(bpp).  The rate kernels (csrc/rate_train.hip) form sum_n scale * w[n] * bits[n]
    themselves, so this class states the trainers' expressions as the per-sample weight vector w (with scale = 1):
      RateDistortionVqCodeTrainer: bpp is the scalar sum(bits) / (N * num_pixel), every reduction leaves it as it is:
        loss_weight * sum(bits) / (N * num_pixel)
      DualBetaCondRateDistortionVqCodeTrainer with sample_beta_batch (dual_cond_rate_distortion_vq_code_trainer.py:92-108,167-175):
        bpp[n] = bits[n] / num_pixel (_calc_batch_bpp), then apply_loss_weight's (loss * beta_weight).mean() with
        beta_weight = exp(beta_rate) or beta_rate + offset:
          none: mean_n(loss_weight * bpp[n] * beta_weight[n]);  mean / sum: loss_weight * mean(bpp) or sum(bpp), times mean(beta_weight)
    `target_rate` is accepted and unused, as in the reference."""

    def __init__(self, loss_weight: float, target_rate: float = 0.0, reduction: str = "mean", **extra):
        if extra:
            raise ValueError(f"RateLoss: unknown keyword(s) {sorted(extra)}")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction: {reduction} is unknown; use mean, sum or none")
        self.loss_weight, self.target_rate, self.reduction = float(loss_weight), float(target_rate), reduction

    def sample_weights(self, N: int, num_pixel: int, beta_weight: Optional[Tensor] = None, device=None) -> Tensor:
        """The fp32 [N] vector w with sum_n w[n] * bits[n] equal to the trainer's rate loss (on `device`, default beta_weight's)."""
        import torch
        if beta_weight is None:
            return torch.full((N,), self.loss_weight / (N * num_pixel), dtype=torch.float32, device=device)
        if beta_weight.dim() != 1 or beta_weight.numel() != N:
            raise ValueError(f"beta_weight: a vector of {N} per-sample weights, got {tuple(beta_weight.shape)}")
        b = beta_weight.to(device=device if device is not None else beta_weight.device, dtype=torch.float64)
        if self.reduction == "none":
            w = b * (self.loss_weight / (N * num_pixel))
        else:
            w = (b.mean() * (self.loss_weight / (num_pixel * (N if self.reduction == "mean" else 1)))).expand(N)
        return w.to(torch.float32).contiguous()


def sample_loss_weights(loss_weight: float, reduction: str, N: int, elems_per_image: int, beta_weight: Tensor, device=None) -> Tensor:
    """The fp32 [N] vector w with sum_n w[n] * S[n] equal to apply_loss_weight(code_loss(...), beta_weight) of
    DualBetaCondRateDistortionVqCodeTrainer (dual_cond_rate_distortion_vq_code_trainer.py:92-98,189-198), where S[n] is image n's own
    sum of the per-element terms (focal cross entropy per position, squared error per element: A.focal_cross_entropy_loss_weighted,
    A.mse_loss_weighted) and the code loss carries `loss_weight` and `reduction` (cross_entropy_loss.py:32-53, distortion_loss.py:43-51):
      none: the map's mean over every axis but the batch, then (loss * beta_weight).mean():  w[n] = loss_weight * beta_weight[n] / (N * elems)
      mean: the scalar times mean(beta_weight):                                              w[n] = loss_weight * mean(beta_weight) / (N * elems)
      sum:                                                                                   w[n] = loss_weight * mean(beta_weight)
    beta_weight is exp(beta_vq) or beta_vq + offset, of length N or -- sample_beta_batch: false -- 1, which broadcasts.  Formed in fp64,
    rounded once."""
    import torch
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction: {reduction} is unknown; use mean, sum or none")
    if N <= 0 or elems_per_image <= 0:
        raise ValueError(f"sample_loss_weights: N={N} images of {elems_per_image} elements")
    if beta_weight.dim() != 1 or beta_weight.numel() not in (1, N):
        raise ValueError(f"beta_weight: a vector of {N} per-sample weights (or of 1, which broadcasts), got {tuple(beta_weight.shape)}")
    b = beta_weight.to(device=device if device is not None else beta_weight.device, dtype=torch.float64)
    if reduction == "none":
        w = (b * (float(loss_weight) / (N * elems_per_image))).expand(N)
    else:
        w = (b.mean() * (float(loss_weight) / (N * elems_per_image if reduction == "mean" else 1))).expand(N)
    return w.to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------------- the YAML's `loss` section
# the reference's trainers with a rate term and per-sample beta weights (config/exp1_stage1_1.yaml, exp1_stage1_2.yaml): the second is
# train/rd_trainer.py, and so is the first, over the unconditioned model (train/build.py's choose_trainer).  Their `rate_loss` entry and
# `reduction: none` are read for them here; in a GAN-stage config both are refused.
RATE_DISTORTION_TRAINERS = ("RateDistortionVqCodeTrainer", "DualBetaCondRateDistortionVqCodeTrainer")
_ENTRIES = ("distortion_loss", "perceptual_loss", "gan_loss", "code_distortion_loss", "code_ce_loss", "rate_loss")
_WEIGHT_NAME = {"distortion_loss": "distortion", "perceptual_loss": "perceptual", "gan_loss": "gan", "code_distortion_loss": "code_distortion",
                "code_ce_loss": "code_ce"}


def mse_distortion_factor(normalize_img: bool, mse_scale: str) -> float:
    """The factor of MSELoss (distortion_loss.py:11-39) on mean((a - b)^2) of the [-1, 1] images: normalised images are mapped to
    [0, 1] or [0, 255] first (alpha 1), un-normalised ones are scaled by alpha = 1/4 or 255^2 / 4000."""
    if mse_scale == "0_1":
        return 0.25
    return (255.0 / 2.0) ** 2 if normalize_img else 255.0 ** 2 / 4000.0


def _refuse(key: str, value, why: str):
    raise SystemExit(f"loss.{key}: {value} {why}")


def _only(entry: dict, name: str, allowed) -> None:
    for k in entry:
        if k not in allowed:
            _refuse(f"{name}.{k}", entry[k], f"is not a keyword of {entry.get('type')} that is built (known: {', '.join(allowed)})")


# distortion_loss types (distortion_loss.py) beside MSELoss: honoured under a rate-distortion trainer only (train/rd_trainer.py)
RD_DISTORTIONS = ("L1Loss", "MSSSIMLoss")


def read_distortion_loss(opt) -> Dict[str, Any]:
    """dict(type, loss_weight) of `opt['loss']['distortion_loss']` for the rate-distortion trainer: `type` is MSELoss (also when the
    entry or its type is absent), L1Loss or MSSSIMLoss; `loss_weight` is None when the YAML gives none.  L1Loss and MSSSIMLoss take
    `loss_weight` only (distortion_loss.py:52-76); another keyword, like another type, is SystemExit with the YAML key and the value.
    MSELoss's own keywords are judged by read_loss_section."""
    try:
        e = dict(opt["loss"]["distortion_loss"] or {})
    except (KeyError, TypeError):
        e = {}
    t = e.get("type")
    if t in RD_DISTORTIONS:
        _only(e, "distortion_loss", ("type", "loss_weight"))
    elif t not in (None, "MSELoss"):
        _refuse("distortion_loss.type", t, f"is not built, expected MSELoss, {' or '.join(RD_DISTORTIONS)}")
    w = e.get("loss_weight")
    if w is not None:
        try:
            w = float(w)
        except (TypeError, ValueError):
            _refuse("distortion_loss.loss_weight", w, "is not a number")
    return dict(type=t or "MSELoss", loss_weight=w)


def read_loss_section(opt) -> Dict[str, Any]:
    """What the GAN-stage trainers need from `opt['loss']`, or SystemExit naming the YAML key and the value.  An absent entry or an
    absent `type` keeps the trainer's defaults (CrossEntropyLoss, MSELoss on [0, 1], VanillaMSELoss mean, LPIPS alex).  Returns
      weights              {trainer weight name: loss_weight} of the entries that give one
      code_ce              dict(type, gamma, reduction) -- `type` None for the default
      distortion_factor    factor on mean((a - b)^2) of the [-1, 1] images (times loss_weight)
      code_distortion_reduction  'mean' or 'sum'
      per_sample           True when `trainer.type` names a rate-distortion trainer (its `reduction: none` entries are kept as read)
      line                 the `[train] losses:` log text
      rate                 under a rate-distortion trainer dict(loss_weight or None, reduction) of `rate_loss`, else None
      distortion_type      MSELoss, or -- under a rate-distortion trainer only -- L1Loss or MSSSIMLoss (read_distortion_loss); the
                           factor is then 1: it belongs to MSELoss
    `gan_loss` is judged by train/build.py's choose_gan_trainer; only its weight is read here."""
    try:
        loss = opt["loss"]
    except (KeyError, TypeError):
        loss = None
    loss = dict(loss) if loss else {}
    try:
        t_type = opt["trainer"]["type"]
    except (KeyError, TypeError):
        t_type = None
    per_sample = t_type in RATE_DISTORTION_TRAINERS
    for k in loss:
        if k not in _ENTRIES:
            _refuse(k, loss[k], f"is not a loss entry of the GAN-stage trainers (known: {', '.join(_ENTRIES)})")
    entries = {k: dict(loss.get(k) or {}) for k in _ENTRIES if k in loss}
    weights = {}
    for k, name in _WEIGHT_NAME.items():
        v = entries.get(k, {}).get("loss_weight")
        if v is not None:
            try:
                weights[name] = float(v)
            except (TypeError, ValueError):
                _refuse(f"{k}.loss_weight", v, "is not a number")

    def reduction_of(name: str, e: dict, allowed=("mean", "sum")) -> str:
        r = e.get("reduction", "mean")
        if r == "none" and per_sample:
            return r
        if r == "none":
            _refuse(f"{name}.reduction", r, "needs the per-sample weighting of the rate-distortion trainers, which are not built; use mean or sum")
        if r not in allowed:
            _refuse(f"{name}.reduction", r, f"is unknown, expected {' or '.join(allowed)}")
        return r

    # rate_loss: no GAN-stage trainer has a rate term (fix_entropy_models)
    if "rate_loss" in entries and not per_sample:
        _refuse("rate_loss", entries["rate_loss"].get("type", entries["rate_loss"]), "has no place in the GAN-stage trainers: they train no rate term")

    # rate_loss under a rate-distortion trainer: RateLoss(loss_weight, target_rate, reduction)
    rate = None
    if per_sample:
        e = entries.get("rate_loss", {})
        if e.get("type", "RateLoss") != "RateLoss":
            _refuse("rate_loss.type", e["type"], "is not built, expected RateLoss")
        _only(e, "rate_loss", ("type", "loss_weight", "target_rate", "reduction"))
        rate = dict(loss_weight=e.get("loss_weight"), reduction=reduction_of("rate_loss", e, ("mean", "sum", "none")))
        if rate["loss_weight"] is not None:
            try:
                rate["loss_weight"] = float(rate["loss_weight"])
            except (TypeError, ValueError):
                _refuse("rate_loss.loss_weight", rate["loss_weight"], "is not a number")

    # code_ce_loss
    e = entries.get("code_ce_loss", {})
    code_ce = dict(type=e.get("type"), gamma=0.0, reduction="mean")
    if e.get("type") == "CrossEntropyLoss":
        _only(e, "code_ce_loss", ("type", "loss_weight", "ce_kwargs"))
        if e.get("ce_kwargs"):
            _refuse("code_ce_loss.ce_kwargs", dict(e["ce_kwargs"]), "is not supported (nn.CrossEntropyLoss options are not built): leave it empty")
    elif e.get("type") == "FocalCrossEntropyLoss":
        _only(e, "code_ce_loss", ("type", "loss_weight", "gamma", "reduction"))
        if "gamma" not in e:
            _refuse("code_ce_loss.gamma", None, "is missing: FocalCrossEntropyLoss has no default gamma")
        try:
            code_ce["gamma"] = check_focal_gamma(e["gamma"])
        except ValueError as err:
            raise SystemExit(f"loss.code_ce_loss.{err}")
        code_ce["reduction"] = reduction_of("code_ce_loss", e)
    elif e.get("type") is not None:
        _refuse("code_ce_loss.type", e["type"], "is not built, expected CrossEntropyLoss or FocalCrossEntropyLoss")

    # distortion_loss
    e = entries.get("distortion_loss", {})
    factor, d_desc, d_type = 0.25, "MSELoss on [0, 1]", "MSELoss"
    if per_sample and e.get("type") in RD_DISTORTIONS:
        d_type = read_distortion_loss(opt)["type"]
        factor = 1.0
        d_desc = f"{d_type} on [-1, 1]" + (" (MS_SSIM data_range=1)" if d_type == "MSSSIMLoss" else "")
    elif e.get("type") == "MSELoss":
        _only(e, "distortion_loss", ("type", "loss_weight", "normalize_img", "mse_scale"))
        norm, scale = e.get("normalize_img", False), e.get("mse_scale", "0_255")
        if not isinstance(norm, bool):
            _refuse("distortion_loss.normalize_img", norm, "is not a boolean")
        if scale not in ("0_255", "0_1"):
            _refuse("distortion_loss.mse_scale", repr(scale), "is unknown, expected '0_255' or '0_1'")
        factor = mse_distortion_factor(norm, scale)
        d_desc = f"MSELoss(normalize_img={norm}, mse_scale={scale})"
    elif e.get("type") is not None:
        _refuse("distortion_loss.type", e["type"], "is not built, expected MSELoss")

    # code_distortion_loss
    e = entries.get("code_distortion_loss", {})
    cd_red = "mean"
    if e.get("type") == "VanillaMSELoss":
        _only(e, "code_distortion_loss", ("type", "loss_weight", "reduction"))
        cd_red = reduction_of("code_distortion_loss", e)
    elif e.get("type") is not None:
        _refuse("code_distortion_loss.type", e["type"], "is not built, expected VanillaMSELoss")

    # perceptual_loss
    e = entries.get("perceptual_loss", {})
    if e.get("type") == "LPIPSLoss":
        _only(e, "perceptual_loss", ("type", "loss_weight", "net", "range_norm"))
        net = e.get("net", "vgg")                      # perceptual_loss.py:12, the reference's default
        if net != "alex":
            _refuse("perceptual_loss.net", net if "net" in e else "vgg (LPIPSLoss's default)", "is not built, expected alex")
        if e.get("range_norm", False):
            _refuse("perceptual_loss.range_norm", e["range_norm"], "is not built: the trainer's images are in [-1, 1] already, set it to false")
    elif e.get("type") is not None:
        _refuse("perceptual_loss.type", e["type"], "is not built, expected LPIPSLoss")

    ce_desc = "CrossEntropyLoss" if code_ce["type"] != "FocalCrossEntropyLoss" else f"FocalCrossEntropyLoss(gamma={code_ce['gamma']:g}, {code_ce['reduction']})"
    line = (f"distortion {d_desc} factor {factor:g}; perceptual LPIPSLoss(net=alex); code_distortion VanillaMSELoss({cd_red}); "
            f"code_ce {ce_desc}")
    return dict(weights=weights, code_ce=code_ce, distortion_factor=factor, code_distortion_reduction=cd_red, per_sample=per_sample, line=line,
                rate=rate, distortion_type=d_type)


def build_code_ce_loss(code_ce: Dict[str, Any], loss_weight: float):
    """The loss object for read_loss_section's `code_ce`, or None for the trainer's default."""
    if code_ce.get("type") is None:
        return None
    cls = LOSS_REGISTRY.get(code_ce["type"])
    if code_ce["type"] == "FocalCrossEntropyLoss":
        return cls(loss_weight, code_ce["gamma"], code_ce["reduction"])
    return cls(loss_weight)
