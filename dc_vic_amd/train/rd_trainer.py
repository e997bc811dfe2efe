"""Stage 1-1 and stage 1-2 rate-distortion training steps of DC-VIC on the HIP kernels.

Mirrors src/trainer/dual_cond_rate_distortion_vq_code_trainer.py:56-200 (`DualBetaCondRateDistortionVqCodeTrainer`, over
rate_distortion_vq_code_trainer.py:61-108 and base_model.py:132-146) with config/exp1_stage1_2.yaml: the whole compression model but the
frozen VQGAN trains with Adam + MultiStepLR on  rate + distortion + perceptual + code_distortion + code_ce, where the rate term and
the two code losses carry one weight per image, exp(beta) or beta + offset (`apply_loss_weight`); the entropy bottleneck's `quantiles`
train apart, with their own Adam on EntropyBottleneck.loss(), AFTER the main step (`optimize_aux_parameters`).

The step runs on the tape: nets.analysis_forward (encoder, hyperprior, CHARM, both entropy models with uniform noise; the rate term's
gradients are seeded by csrc/rate_train.hip), then nets.synthesis_forward on the `Var` y_hat (decoder features, estimator, argmax LUT, fusion
decoder), so the image and code losses reach the analysis side through y_hat's straight-through estimator; the step's pieces are BetaPairTrainerBase's.  The per-image weighting of the
code losses is csrc/sample_loss.hip (A.mse_loss_weighted, A.focal_cross_entropy_loss_weighted, losses.sample_loss_weights).

Stage 1-1 (`RateDistortionVqCodeTrainer`, rate_distortion_vq_code_trainer.py:116-194, config/exp1_stage1_1.yaml) is the same step over the
unconditioned HyperpriorCharmVicModel: no beta pair, the five terms as plain reductions, a LinearWarmupScheduler.  RateDistortionStep
holds the step once; the two trainers differ in where the betas come from and in how the rate and code terms are weighted.

Differences, stated: those of trainer.py (LPIPS weights, data-parallel averaging); the uniform noise comes from a trainer-owned device
torch.Generator, not from torch's global one; `model.gumbel_sampling: true` is refused."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..registry import TRAINER_REGISTRY
from . import autograd as A
from . import nets
from .autograd import Ctx, ParamGroup
from .losses import RateLoss, check_focal_gamma, sample_loss_weights
from .trainer import Adam, BetaPairTrainerBase, LinearWarmupScheduler, MultiStepLR, adam_state, load_adam_state

Tensor = torch.Tensor

# config/exp1_stage1_2.yaml's loss_weight values
DEFAULT_RD_LOSS = dict(rate=0.5, distortion=50.0, perceptual=1.0, code_distortion=0.006, code_ce=0.003)
BETA_POLICIES = ("linear", "exp")
DISTORTION_TYPES = ("MSELoss", "L1Loss", "MSSSIMLoss")
LOG_KEYS = ("rate", "distortion", "perceptual", "code_distortion", "code_ce", "total", "qbpp", "vq_acc", "lr", "aux")


def is_main_parameter(name: str) -> bool:
    """rate_distortion_vq_code_trainer.py:61-73 / base_model.py:132-146: every parameter of the model except the frozen VQGAN's and the
    entropy bottleneck's `quantiles` (which the aux optimizer owns)."""
    return not name.startswith("vq_model.") and not name.endswith(".quantiles")


def beta_loss_weight(policy: str, offset: float, beta: Tensor) -> Tensor:
    """One half of calc_vq_rate_loss_weight (:71-78): beta + offset or exp(beta), fp32 as the reference's."""
    if policy == "linear":
        return beta.float() + offset
    if policy == "exp":
        return torch.exp(beta.float())
    raise ValueError(f"beta_policy: {policy} is unknown, expected linear or exp")


def beta_loss_weights(policy: str, offset: float, beta_vq: Tensor, beta_rate: Tensor) -> Tuple[Tensor, Tensor]:
    """calc_vq_rate_loss_weight (:71-78) -> (vq_weight, rate_weight)."""
    return beta_loss_weight(policy, offset, beta_vq), beta_loss_weight(policy, offset, beta_rate)


class RateDistortionStep(BetaPairTrainerBase):
    """The rate-distortion step both stages share: the parameter groups (everything but the frozen VQGAN; `quantiles` apart), the
    training state, forward and losses on the tape, clip + Adam + scheduler, the aux step.  A subclass says which betas a step trains
    with (step_betas), how the rate term is weighted per image (rate_weights) and how the two code terms are formed (code_terms)."""

    def _setup(self, model, lr: float, aux_lr: float, sched, clip_max_norm: Optional[float], loss_weights: Optional[Dict[str, float]], dist, seed: int,
               lpips_state: Optional[Dict[str, Tensor]], rate_reduction: str, code_ce_gamma: float, code_ce_reduction: str,
               code_distortion_reduction: str, distortion_factor: float, gumbel_sampling: bool, distortion_type: str,
               reductions=("none", "mean", "sum")) -> None:
        if distortion_type not in DISTORTION_TYPES:
            raise ValueError(f"distortion_type: {distortion_type} is unknown, expected {', '.join(DISTORTION_TYPES)}")
        if gumbel_sampling:
            raise ValueError("model.gumbel_sampling: true is not built (the Gumbel-softmax sampling of the VQ indices in training mode): set it to false")
        for what, r in (("rate", rate_reduction), ("code_ce", code_ce_reduction), ("code_distortion", code_distortion_reduction)):
            if r not in reductions:
                raise ValueError(f"{what} reduction: {r} is unknown; use {', '.join(reductions[:-1])} or {reductions[-1]}")
        self.model = model
        dev = next(model.decoder.parameters()).device
        self.device = dev
        self.group = ParamGroup([model], dev, select=is_main_parameter)
        self.aux_group = ParamGroup([model.entropy_model_z], dev, select=lambda name: name == "quantiles")
        self.opt, self.aux_opt = Adam(self.group, lr), Adam(self.aux_group, aux_lr)
        self.sched = sched
        self.clip = clip_max_norm
        self.w = dict(DEFAULT_RD_LOSS)
        if loss_weights:
            self.w.update(loss_weights)
        self.rate_loss = RateLoss(self.w["rate"], reduction=rate_reduction)
        self.code_ce_gamma, self.code_ce_reduction = check_focal_gamma(code_ce_gamma), code_ce_reduction
        self.code_distortion_reduction, self.distortion_factor = code_distortion_reduction, float(distortion_factor)
        self.distortion_type = distortion_type
        self.dist = dist
        self.noise_gen = torch.Generator(device=dev).manual_seed(seed)         # the entropy models' uniform noise
        self._build_lpips(self.w["perceptual"], lpips_state, dev)

    # ---------------------------------------------------------------- training state
    def training_state(self, current_iter: int) -> Dict:
        return {"iter": int(current_iter), "noise_gen": self.noise_gen.get_state().clone(),
                "last_epoch": int(self.sched.last_epoch), "main": adam_state(self.opt), "aux": adam_state(self.aux_opt)}

    def load_training_state(self, st: Dict) -> int:
        load_adam_state(self.opt, st["main"], "main")
        load_adam_state(self.aux_opt, st["aux"], "aux")
        self.sched.last_epoch = int(st["last_epoch"])
        self.noise_gen.set_state(st["noise_gen"])
        return int(st["iter"])

    def resync_parameters(self) -> None:
        """After a state dict was loaded into the model: parameters are views of the flat buffers, so load_state_dict's copy_ already
        wrote them; cached packed weights are stale."""
        self.group.refresh_plans(); self.aux_group.refresh_plans()
        self._drop_inference_graphs()

    def checkpoint_modules(self) -> Dict[str, torch.nn.Module]:
        """{name: module} of what a checkpoint holds beside the training state: no discriminator here."""
        return {"comp_model": self.model}

    # ---------------------------------------------------------------- what a subclass states
    def step_betas(self, data_dict: Dict, n: int):
        raise NotImplementedError()

    def rate_weights(self, N: int, num_pixel: int, beta_rate) -> Tensor:
        raise NotImplementedError()

    def code_terms(self, ctx: Ctx, s: Dict, gt_lat: Tensor, gt_idx: Tensor, beta_vq) -> Tuple[Tensor, Tensor]:
        raise NotImplementedError()

    # ---------------------------------------------------------------- one step
    def forward_losses(self, ctx: Ctx, real: Tensor, vq_indices: Optional[Tensor], beta_rate=None, beta_vq=None,
                       noise_y: Optional[Tensor] = None, noise_z: Optional[Tensor] = None):
        """run_comp_model (:80-90, is_train, fix_entropy_models=False) and calc_g_loss (:153-200) on the tape: every term's gradient is
        seeded (the rate term's at forward time).  -> (loss terms as 1-element device tensors, outputs)."""
        m = self.model
        x = real.to(self.device, dtype=torch.float32).contiguous()
        N, _, H, W = x.shape
        w_rate = self.rate_weights(N, H * W, beta_rate)
        out = nets.analysis_forward(ctx, m, x, beta_rate, beta_vq, vq_indices=vq_indices, noise_y=noise_y, noise_z=noise_z, generator=self.noise_gen,
                                    weights=w_rate, scale=1.0)
        s = nets.synthesis_forward(ctx, m, out["quantized_code"]["y"], beta_rate, beta_vq)
        fake = s["fake"]
        L = {"rate": out["loss"]}
        if self.distortion_type == "MSSSIMLoss":           # raises, naming the size, when min(H, W) <= 160
            L["distortion"] = A.ms_ssim_loss(ctx, fake, x, self.w["distortion"])
        elif self.distortion_type == "L1Loss":
            L["distortion"] = A.l1_loss(ctx, fake, x, self.w["distortion"])
        else:
            L["distortion"] = A.mse_loss(ctx, fake, x, self.w["distortion"] * self.distortion_factor)
        L["perceptual"] = self.perceptual_term(ctx, x, fake)
        L["code_distortion"], L["code_ce"] = self.code_terms(ctx, s, out["gt_vq_latent"], out["gt_vq_indices"], beta_vq)
        out.update(s, real=x, qbpp=self.qbpp(out["q_bits_y"], out["q_bits_z"], x))
        return L, out

    def optimize_aux_parameters(self) -> float:
        """rate_distortion_vq_code_trainer.py `optimize_aux_parameters`: EntropyBottleneck.loss() on the parameters as they are NOW
        (after the main step), its gradient w.r.t. `quantiles`, averaged over the ranks, one Adam step."""
        self.aux_group.zero_grad()
        aux = A.eb_aux_loss(Ctx([self.aux_group]), self.model.entropy_model_z)     # writes the gradient itself: no tape to run, no clip
        self.apply_gradients(None, self.aux_opt)
        return float(aux.item())

    def optimize_parameters(self, current_iter: int, data_dict: Dict) -> Optional[Dict[str, float]]:
        real = data_dict["real_images"]
        beta_rate, beta_vq = self.step_betas(data_dict, real.shape[0])
        self.group.zero_grad()
        ctx = Ctx([self.group])
        L, o = self.forward_losses(ctx, real, data_dict.get("vq_indices"), beta_rate, beta_vq, data_dict.get("noise_y"), data_dict.get("noise_z"))
        log = {k: float(v.item()) for k, v in L.items()}
        total = sum(log.values())
        if self.skip_step(total, ctx):
            return None
        lr_now = self.sched.lr()
        self.apply_gradients(ctx, self.opt, lr_now, self.clip)     # clip_grad_norm_ over comp_model.parameters(): `quantiles` has no gradient yet
        self.sched.step()
        aux = self.optimize_aux_parameters()
        self._drop_inference_graphs()
        log.update(total=total, qbpp=o["qbpp"], vq_acc=self.vq_acc(o), lr=lr_now, aux=aux)
        return log


@TRAINER_REGISTRY.register()
class DualBetaCondRateDistortionVqCodeTrainer(RateDistortionStep):
    def __init__(self, model, lr: float = 1e-4, aux_lr: float = 1e-3, milestones=(300000,), gamma: float = 0.1,
                 clip_max_norm: Optional[float] = 1.0, loss_weights: Optional[Dict[str, float]] = None, beta_policy: str = "linear",
                 beta_offset: float = 1.0, sample_beta_batch: bool = False, dist=None, seed: int = 0, lpips_state: Optional[Dict[str, Tensor]] = None,
                 rate_reduction: str = "mean", code_ce_gamma: float = 0.0, code_ce_reduction: str = "mean", code_distortion_reduction: str = "mean",
                 distortion_factor: float = 0.25, gumbel_sampling: bool = False, distortion_type: str = "MSELoss"):
        """`loss_weights`: {rate, distortion, perceptual, code_distortion, code_ce} over DEFAULT_RD_LOSS; the three `*_reduction`s are
        none, mean or sum (RateLoss, FocalCrossEntropyLoss, VanillaMSELoss); `code_ce_gamma` 0 is the plain cross entropy;
        `beta_policy` / `beta_offset` / `sample_beta_batch` default as the reference's constructor does; `distortion_type` is MSELoss,
        L1Loss or MSSSIMLoss (distortion_loss.py), `distortion_factor` belongs to MSELoss alone."""
        if beta_policy not in BETA_POLICIES:
            raise ValueError(f"beta_policy: {beta_policy} is unknown, expected linear or exp")
        self._setup(model, lr, aux_lr, MultiStepLR(lr, list(milestones), gamma), clip_max_norm, loss_weights, dist, seed, lpips_state, rate_reduction,
                    code_ce_gamma, code_ce_reduction, code_distortion_reduction, distortion_factor, gumbel_sampling, distortion_type)
        self.beta_policy, self.beta_offset, self.sample_beta_batch = beta_policy, float(beta_offset), bool(sample_beta_batch)
        self.last_beta_rate: Optional[Tensor] = None
        self.last_beta_vq: Optional[Tensor] = None
        self.rng = np.random.RandomState(seed)                                 # the beta samplers

    def training_state(self, current_iter: int) -> Dict:
        return dict(super().training_state(current_iter), rng=self.rng.get_state())

    def load_training_state(self, st: Dict) -> int:
        self.rng.set_state(st["rng"])
        return super().load_training_state(st)

    def step_betas(self, data_dict: Dict, n: int):
        return self.step_beta_pair(data_dict, n)

    def rate_weights(self, N: int, num_pixel: int, beta_rate) -> Tensor:
        rate_w = beta_loss_weight(self.beta_policy, self.beta_offset, beta_rate)
        return self.rate_loss.sample_weights(N, num_pixel, rate_w.expand(N).contiguous(), device=self.device)

    def code_terms(self, ctx: Ctx, s: Dict, gt_lat: Tensor, gt_idx: Tensor, beta_vq) -> Tuple[Tensor, Tensor]:
        """apply_loss_weight of the two code losses: one weight per image, exp(beta_vq) or beta_vq + offset (csrc/sample_loss.hip)."""
        N = gt_lat.shape[0]
        vq_w = beta_loss_weight(self.beta_policy, self.beta_offset, beta_vq)
        w_cd = sample_loss_weights(self.w["code_distortion"], self.code_distortion_reduction, N, gt_lat[0].numel(), vq_w, device=self.device)
        w_ce = sample_loss_weights(self.w["code_ce"], self.code_ce_reduction, N, gt_idx[0].numel(), vq_w, device=self.device)
        return (A.mse_loss_weighted(ctx, s["pred_embed"], gt_lat, w_cd),
                A.focal_cross_entropy_loss_weighted(ctx, s["logits"], gt_idx, w_ce, self.code_ce_gamma))


@TRAINER_REGISTRY.register()
class RateDistortionVqCodeTrainer(RateDistortionStep):
    """rate_distortion_vq_code_trainer.py:116-194 with config/exp1_stage1_1.yaml: stage 1-1, the unconditioned HyperpriorCharmVicModel from
    its initialisation.  No beta pair and no beta RNG; the terms are plain reductions:
      rate = loss_weight * sum(bits) / (N H W)   (RateLoss on the scalar bpp: mean and sum leave it as it is),
      MSELoss x factor, LPIPS, VanillaMSELoss (mean or sum), FocalCrossEntropyLoss(gamma) (mean or sum)."""

    def __init__(self, model, lr: float = 1e-4, aux_lr: float = 1e-3, scheduler: Optional[Dict] = None, clip_max_norm: Optional[float] = 1.0,
                 loss_weights: Optional[Dict[str, float]] = None, dist=None, seed: int = 0, lpips_state: Optional[Dict[str, Tensor]] = None,
                 rate_reduction: str = "mean", code_ce_gamma: float = 0.0, code_ce_reduction: str = "mean", code_distortion_reduction: str = "mean",
                 distortion_factor: float = 0.25, gumbel_sampling: bool = False, distortion_type: str = "MSELoss"):
        """`scheduler`: dict(type="LinearWarmupScheduler", warmup_iters, warmup_factor) or dict(type="MultiStepLR", milestones, gamma)
        (train/build.py read_g_scheduler), None for MultiStepLR([300000], 0.1); `reduction: none` has no meaning without beta weights."""
        if hasattr(model.encoder, "beta_ft_list") or hasattr(model.decoder, "beta_ft_list"):
            raise ValueError(f"RateDistortionVqCodeTrainer trains the unconditioned HyperpriorCharmVicModel, not {type(model).__name__}: "
                             "its encoder or decoder is beta-conditioned and this trainer draws no beta pair")
        self._setup(model, lr, aux_lr, make_scheduler(lr, scheduler), clip_max_norm, loss_weights, dist, seed, lpips_state, rate_reduction,
                    code_ce_gamma, code_ce_reduction, code_distortion_reduction, distortion_factor, gumbel_sampling, distortion_type,
                    reductions=("mean", "sum"))

    def step_betas(self, data_dict: Dict, n: int):
        return None, None

    def rate_weights(self, N: int, num_pixel: int, beta_rate) -> Tensor:
        return self.rate_loss.sample_weights(N, num_pixel, None, device=self.device)

    def code_terms(self, ctx: Ctx, s: Dict, gt_lat: Tensor, gt_idx: Tensor, beta_vq) -> Tuple[Tensor, Tensor]:
        w_cd = self.w["code_distortion"] * (gt_lat.numel() if self.code_distortion_reduction == "sum" else 1)
        return (A.mse_loss(ctx, s["pred_embed"], gt_lat, w_cd),
                A.focal_cross_entropy_loss(ctx, s["logits"], gt_idx, self.w["code_ce"], self.code_ce_gamma, self.code_ce_reduction))

    def validation(self, current_iter: int, images) -> Dict[str, float]:
        """{bpp, psnr, ms_ssim, vq_acc}: the means over `images` (_validation, :177-180), on the weights of `current_iter`."""
        rows = self.model.validation(images, max_sample_size=100)
        return {k: sum(r[k] for r in rows) / len(rows) for k in ("bpp", "psnr", "ms_ssim", "vq_acc")}


def make_scheduler(lr: float, scheduler: Optional[Dict]):
    """The generator-side schedule of read_g_scheduler's dict."""
    kw = dict(scheduler or dict(type="MultiStepLR", milestones=[300000], gamma=0.1))
    t = kw.pop("type")
    if t == "LinearWarmupScheduler":
        return LinearWarmupScheduler(lr, **kw)
    if t == "MultiStepLR":
        return MultiStepLR(lr, list(kw["milestones"]), kw["gamma"])
    raise ValueError(f"g_scheduler.type: {t} is unknown, expected MultiStepLR or LinearWarmupScheduler")
