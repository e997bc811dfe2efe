"""Stage-3 GAN training step of DC-VIC on the HIP kernels, data-parallel over one process per GPU.

Mirrors src/trainer/dual_cond_gan_distortion_vq_code_trainer.py:24-300 (`DualBetaCondGanDistortionVqCodeTrainer`):
`optimize_parameters` = G step (run_comp_model with is_train=True / fix_entropy_models=True / sample_batch_beta, calc_g_loss,
backward, clip_grad_norm_, Adam, MultiStepLR) followed by the D step (run_discriminator, calc_d_loss, backward, Adam).
Loss definitions: config/exp1_stage1_3.yaml:61-79 (MSELoss x50 on [0,1] images, VanillaGANLoss x0.01, VanillaMSELoss x1 on
the predicted code embedding, CrossEntropyLoss x0.5 on the code logits).  Stage 1-3 (config/exp1_stage1_3.yaml) is the same trainer
without `use_selected_beta_pairs`: beta_rate and beta_vq come per sample from `sample_beta_grid`; the code loss may be the
FocalCrossEntropyLoss of train/losses.py.

Differences, stated:
  * LPIPS (perceptual_loss): the `lpips` wheel and its AlexNet / head weights cannot be fetched offline.  The term is computed
    by dc_vic_amd/train/lpips.py (architecture restated, state-dict key names of the package) with deterministic synthetic
    weights unless an `lpips` state dict is loaded into `trainer.lpips` -- parity unpinned.  Pass `loss_weights={'perceptual': 0}`
    to drop the term.
  * the reference is single-process (README.md:64-65, base_trainer.py:158 TODO); here gradients are averaged across ranks
    with bucketed RCCL all-reduces of the flat gradient buffers -- with world size 1 nothing is sent.
Training mode changes nothing numerically on the frozen encoder / entropy side for this trainer: with
fix_entropy_models=True it runs under no_grad and ste_round(y - mu) + mu has the values of round(y - mu) + mu
(ste_gaussian_conditional.py:16-23), so the inference kernels provide y_hat; the noise-quantised likelihoods only feed a
rate loss this trainer does not have (the logged `qbpp` uses the quantised ones, calc_g_loss :199).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..layers import ActNorm, invalidate_weight_caches
from ..registry import LOSS_REGISTRY, TRAINER_REGISTRY
from . import autograd as A
from . import kernels as K
from . import nets
from .autograd import Ctx, ParamGroup

Tensor = torch.Tensor

DEFAULT_LOSS = dict(distortion=50.0, perceptual=1.0, gan=0.01, code_distortion=1.0, code_ce=0.5)


def allreduce_mean_(flat: Tensor, dist, bucket_bytes: int = 64 << 20) -> int:
    """Average a flat gradient buffer over the ranks with bucketed all-reduces (async, joined at the end).  Ring collectives
    over xGMI are per-link bound, so a few large buckets beat many small ones; 64 MiB keeps three or so in flight for the
    134 MB generator gradient.  Returns the number of buckets."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return 0
    n = flat.numel()
    step = max(1, bucket_bytes // 4)
    works = []
    for off in range(0, n, step):
        works.append(dist.all_reduce(flat[off:off + step], op=dist.ReduceOp.SUM, async_op=True))
    for w in works:
        w.wait()
    if flat.is_cuda:
        K.ew(K.EW_SCALE, None, flat, w=1.0 / dist.get_world_size(), out=flat)
    else:
        flat.mul_(1.0 / dist.get_world_size())        # CPU (gloo tests): plumbing only
    return len(works)


def sample_beta_grid(rng: np.random.RandomState, max_beta: float, num_levels: int, n: int) -> Tensor:
    """hyperprior_dc_vic_model.py:91-97 (`_sample_beta`): n draws from the grid max_beta * k / num_levels, k = 0..num_levels (both
    ends reachable), as a float32 tensor [n].  The reference draws from numpy's global state; here the generator is passed in."""
    i = rng.randint(0, num_levels + 1, n)
    beta = np.float32(max_beta) * (i.astype(np.float32) / np.float32(num_levels))
    return torch.from_numpy(np.asarray(beta, dtype=np.float32))


def loss_anomaly(total: float, dist, device=None) -> bool:
    """base_trainer.py:235-245 skips a step whose total loss is non-finite or > 1e4.  With several ranks the decision must be
    COLLECTIVE: a rank that returned early while the others entered the gradient all-reduce would leave them blocked in RCCL
    forever (and let the Adam / scheduler step counts diverge).  One 1-element MAX all-reduce of the local flag: every rank
    skips or none does."""
    bad = (not math.isfinite(total)) or total > 1e4
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return bad
    flag = torch.tensor([1.0 if bad else 0.0], dtype=torch.float32, device=device if device is not None else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    return bool(flag.item() > 0)


def gumbel_tau(gumbel_kwargs: Optional[Dict]) -> float:
    """`tau` of model.gumbel_kwargs (default 1).  The trainer's sample is F.gumbel_softmax(logits, dim=1, hard=True, tau=tau): `tau` is the
    only keyword it can honour (`hard` and `dim` would collide with the reference's own arguments, `eps` is deprecated and unused)."""
    kw = dict(gumbel_kwargs or {})
    tau = kw.pop("tau", 1.0)
    if kw:
        k = sorted(kw)[0]
        raise ValueError(f"model.gumbel_kwargs.{k}: {kw[k]!r} is not built: tau is the only keyword of the Gumbel-softmax sample")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not math.isfinite(tau) or tau <= 0:
        raise ValueError(f"model.gumbel_kwargs.tau: {tau!r} is not a finite number > 0")
    return float(tau)


class MultiStepLR:
    def __init__(self, base_lr: float, milestones: List[int], gamma: float):
        self.base_lr, self.milestones, self.gamma, self.last_epoch = base_lr, sorted(milestones), gamma, 0

    def lr(self) -> float:
        return self.base_lr * self.gamma ** sum(1 for m in self.milestones if m <= self.last_epoch)

    def step(self) -> None:
        self.last_epoch += 1


class LinearWarmupScheduler:
    """build_optimizer_scheduler.py:13-24: lr(k) = base_lr * (warmup_factor * (1 - k / warmup_iters) + k / warmup_iters) for
    k < warmup_iters steps taken, base_lr from then on; the expression is the reference's, operation by operation."""

    def __init__(self, base_lr: float, warmup_iters: int, warmup_factor: float):
        if isinstance(warmup_iters, bool) or not isinstance(warmup_iters, int) or warmup_iters < 0:
            raise ValueError(f"warmup_iters: {warmup_iters!r} is not an integer >= 0")
        self.base_lr, self.warmup_iters, self.warmup_factor, self.last_epoch = base_lr, warmup_iters, float(warmup_factor), 0

    def lr(self) -> float:
        if self.last_epoch < self.warmup_iters:
            alpha = float(self.last_epoch) / self.warmup_iters
            return self.base_lr * (self.warmup_factor * (1 - alpha) + alpha)
        return self.base_lr

    def step(self) -> None:
        self.last_epoch += 1


class Adam:
    """torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8) on a ParamGroup's flat buffers."""

    def __init__(self, group: ParamGroup, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8):
        self.group, self.lr, self.betas, self.eps, self.t = group, lr, betas, eps, 0

    def step(self, lr: Optional[float] = None, gscale: Optional[Tensor] = None) -> None:
        self.t += 1
        g = self.group
        K.adam_step(g.flat, g.grad, g.m, g.v, self.lr if lr is None else lr, self.betas[0], self.betas[1], self.eps, self.t, gscale)
        g.refresh_plans()


def adam_state(opt: Adam) -> Dict:
    """The Adam part of a training state: the group's moments (host copies), the step count and the group's size."""
    g = opt.group
    return {"m": g.m.detach().cpu().clone(), "v": g.v.detach().cpu().clone(), "t": int(opt.t), "numel": int(g.numel())}


def load_adam_state(opt: Adam, s_: Dict, tag: str) -> None:
    """adam_state's entries of the group saved as `tag` back into `opt`; ValueError when the group's size is another."""
    g = opt.group
    if int(s_["numel"]) != g.numel():
        raise ValueError(f"training state: {tag} group has {s_['numel']} parameters, this model {g.numel()}")
    g.m.copy_(s_["m"].to(g.m.device)); g.v.copy_(s_["v"].to(g.v.device))
    opt.t = int(s_["t"])


class BetaPairTrainerBase:
    """What the GAN-stage trainers and the rate-distortion trainer (rd_trainer.py) share: the perceptual network and its weights, the
    beta-pair samplers (drawing from `self.rng`), the pieces of a step (beta pair, anomaly skip, perceptual term, a group's gradient step, the
    logged vq_acc / qbpp), validation, the forgetting of captured graphs.  Expects `self.model`, `rng`, `device`, `dist`, `w`, `sample_beta_batch`."""

    def _build_lpips(self, weight: float, lpips_state: Optional[Dict[str, Tensor]], dev) -> None:
        self.lpips = None
        if weight > 0:
            from .lpips import LPIPSAlex
            self.lpips = LPIPSAlex(seed=0).to(dev)
            self.lpips_is_synthetic = lpips_state is None
            if lpips_state is not None:
                self.load_lpips_state(lpips_state)

    def load_lpips_state(self, sd: Dict[str, Tensor]) -> None:
        """Load a state dict of the `lpips` package (LPIPS(net='alex').state_dict(): net.sliceK.I.weight/bias, linK.model.1.weight,
        scaling_layer.shift/scale) into the perceptual network, strictly by key and shape."""
        own = self.lpips.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError(f"lpips state dict lacks {missing[:4]}{'...' if len(missing) > 4 else ''}")
        for k, v in own.items():
            if tuple(sd[k].shape) != tuple(v.shape):
                raise ValueError(f"lpips state dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(v.shape)}")
            v.copy_(sd[k].to(v.device, dtype=v.dtype))
        invalidate_weight_caches(self.lpips)
        self.lpips_is_synthetic = False

    def _drop_inference_graphs(self) -> None:
        """The generator's weights moved in place: hipGraphs captured by compress_batch / decompress_batch before that replay the old
        packed weights -- forget them (the next inference call re-captures)."""
        g = getattr(self.model, "_graphs", None)
        if g is not None:
            g.clear()

    # dual_cond_rate_distortion_vq_code_trainer.py:202-233 (_validation)
    def validation_beta_pairs(self) -> List[Tuple[float, float, str]]:
        """(beta_rate, beta_vq, label): the first selected pair when the model uses selected pairs, else the four corners."""
        m = self.model
        if getattr(m, "use_selected_beta_pairs", False):
            return [(float(m.selected_beta_rate[0]), float(m.selected_beta_vq[0]), "idx0")]
        br, bv = float(m.max_beta_rate), float(m.max_beta_vq)
        return [(br, 0.0, "rate_max_vq_000"), (br, bv, "rate_max_vq_max"), (0.0, 0.0, "rate_000_vq_000"), (0.0, bv, "rate_000_vq_max")]

    def validation(self, current_iter: int, images: List[Tensor]) -> Dict[str, float]:
        """{<label>_<metric>: mean over `images`} for every validation beta pair, on the weights of `current_iter` (the packed plans
        are refreshed by every optimizer step).  Runs the inference path only -- no graph capture, no draw from the beta sampler, no
        touch of the optimizer, scheduler, discriminator or data state -- so training continues exactly as without it."""
        out: Dict[str, float] = {}
        for beta_rate, beta_vq, label in self.validation_beta_pairs():
            rows = self.model.validation(images, max_sample_size=100, beta_rate=beta_rate, beta_vq=beta_vq)
            for k in ("bpp", "psnr", "ms_ssim", "vq_acc", "vq_mse"):
                out[f"{label}_{k}"] = sum(r[k] for r in rows) / len(rows)
        return out

    # hyperprior_dc_vic_model.py:99-110
    def sample_selected_beta_pair(self, n: int) -> Tuple[Tensor, Tensor]:
        m = self.model
        i = self.rng.randint(0, len(m.selected_beta_rate), n)
        return (torch.Tensor([m.selected_beta_rate[k] for k in i]).float(), torch.Tensor([m.selected_beta_vq[k] for k in i]).float())

    # hyperprior_dc_vic_model.py:143-161 (data_preprocess without selected pairs): beta_rate first, then beta_vq
    def sample_beta_pair(self, n: int) -> Tuple[Tensor, Tensor]:
        m = self.model
        if getattr(m, "use_selected_beta_pairs", False):
            return self.sample_selected_beta_pair(n)
        beta_rate = sample_beta_grid(self.rng, m.max_beta_rate, m.num_beta_levels, n)
        beta_vq = sample_beta_grid(self.rng, m.max_beta_vq, m.num_beta_levels, n)
        return beta_rate, beta_vq

    # ---------------------------------------------------------------- the pieces of optimize_parameters
    def step_beta_pair(self, data_dict: Dict, n: int):
        """The pair this step trains with: the data dict's, else drawn per image (sample_beta_batch) or once; kept as last_beta_*."""
        beta_rate, beta_vq = data_dict.get("beta_rate"), data_dict.get("beta_vq")
        if beta_rate is None or beta_vq is None:
            beta_rate, beta_vq = self.sample_beta_pair(n if self.sample_beta_batch else 1)
        self.last_beta_rate, self.last_beta_vq = beta_rate, beta_vq
        return beta_rate, beta_vq

    def perceptual_term(self, ctx: Ctx, real: Tensor, fake) -> Tensor:
        """LPIPS(real, fake) x w['perceptual'] on the tape, or a zero when the term is off."""
        if self.lpips is None:
            return torch.zeros(1, device=self.device)
        from .lpips import lpips_loss
        return lpips_loss(ctx, self.lpips, real, fake, self.w["perceptual"])

    def skip_step(self, total: float, ctx: Ctx) -> bool:
        """base_trainer.py:235-245: a total loss that is non-finite or > 1e4 skips the step -- on EVERY rank or on none -- and drops its pass."""
        if not loss_anomaly(total, self.dist, self.device):
            return False
        ctx.discard()
        return True

    def apply_gradients(self, ctx: Optional[Ctx], opt: Adam, lr: Optional[float] = None, clip: Optional[float] = None) -> None:
        """A group's step: backward (`ctx` None: the gradient is written already), mean over the ranks, clip_grad_norm_'s scale, Adam at `lr`."""
        if ctx is not None:
            ctx.backward()
        grad = opt.group.grad
        allreduce_mean_(grad, self.dist)
        gscale = K.clip_scale(K.reduce_loss(K.SUM_SQ, grad, None, 1.0), clip) if clip else None
        opt.step(lr, gscale)

    @staticmethod
    def qbpp(bits_y: Tensor, bits_z: Tensor, x: Tensor) -> float:
        """Bits per pixel of the quantised likelihoods over the batch x (the logged `qbpp`, calc_g_loss :199)."""
        return float((bits_y.double().sum() + bits_z.double().sum()).item()) / (x.shape[0] * x.shape[2] * x.shape[3])

    @staticmethod
    def vq_acc(o: Dict) -> float:
        return float((o["out_vq_indices"] == o["gt_vq_indices"]).float().mean().item())


@TRAINER_REGISTRY.register()
class DualBetaCondGanDistortionVqCodeTrainer(BetaPairTrainerBase):
    def __init__(self, model, discriminator, lr_g: float = 1e-4, lr_d: float = 1e-4, milestones=(300000,), gamma: float = 0.1,
                 clip_max_norm: Optional[float] = 1.0, loss_weights: Optional[Dict[str, float]] = None, sample_beta_batch: bool = True,
                 dist=None, seed: int = 0, d_milestones=None, d_gamma: Optional[float] = None, lpips_state: Optional[Dict[str, Tensor]] = None,
                 code_ce_loss=None, distortion_factor: float = 0.25, code_distortion_reduction: str = "mean",
                 gumbel_sampling: Optional[bool] = None, gumbel_kwargs: Optional[Dict] = None):
        """`code_ce_loss`: a loss object of train/losses.py (CrossEntropyLoss / FocalCrossEntropyLoss, carrying its own weight) or None
        for CrossEntropyLoss x loss_weights['code_ce']; `distortion_factor`: MSELoss's factor on mean((a - b)^2) of the [-1, 1] images
        (0.25 = the [0, 1] scale of the shipped configs); `code_distortion_reduction`: VanillaMSELoss's mean or sum;
        `gumbel_sampling` / `gumbel_kwargs` (None: the model's attributes of those names): decode a hard Gumbel-softmax sample of the
        code logits instead of their argmax (hyperprior_dc_vic_model.py:254-260), which lets the image losses reach the estimator; the
        only keyword is `tau` (> 0, default 1).  The draws come from `self.gumbel_gen`, a device generator seeded like the beta sampler."""
        self.model, self.D = model, discriminator
        if dist is not None and dist.get_world_size() > 1 and any(isinstance(m, ActNorm) for m in discriminator.modules()):
            # BatchNorm statistics are per rank, as under DDP without SyncBatchNorm; rank 0's buffers are the ones saved
            raise ValueError("norm_type actnorm cannot train on more than one rank: its data-dependent initialisation (loc and scale from the "
                             "first batch) would differ per rank")
        dev = next(model.decoder.parameters()).device
        self.device = dev
        # only decoder, vq_estimator, fusion_module are trained (:47-52)
        self.g_group = ParamGroup([model.decoder, model.vq_estimator, model.fusion_module], dev)
        self.d_group = ParamGroup([discriminator], dev)
        self.g_opt, self.d_opt = Adam(self.g_group, lr_g), Adam(self.d_group, lr_d)
        # config/exp1_stage1_3.yaml:43-60: g_scheduler and d_scheduler are separate YAML entries (same values in the shipped files)
        self.g_sched = MultiStepLR(lr_g, list(milestones), gamma)
        self.d_sched = MultiStepLR(lr_d, list(milestones if d_milestones is None else d_milestones), gamma if d_gamma is None else d_gamma)
        self.clip = clip_max_norm
        self.w = dict(DEFAULT_LOSS)
        if loss_weights:
            self.w.update(loss_weights)
        if code_distortion_reduction not in ("mean", "sum"):
            raise ValueError(f"code_distortion_reduction {code_distortion_reduction!r}: expected 'mean' or 'sum'")
        self.code_ce_loss, self.distortion_factor, self.code_distortion_reduction = code_ce_loss, float(distortion_factor), code_distortion_reduction
        self.sample_beta_batch = sample_beta_batch
        self.last_beta_rate: Optional[Tensor] = None   # the pair the last optimize_parameters trained with
        self.last_beta_vq: Optional[Tensor] = None
        self.dist = dist
        self.rng = np.random.RandomState(seed)
        self.last_fake: Optional[Tensor] = None
        self._build_lpips(self.w["perceptual"], lpips_state, dev)
        self.gumbel_sampling = bool(getattr(model, "gumbel_sampling", False) if gumbel_sampling is None else gumbel_sampling)
        self.gumbel_tau = 1.0
        self.gumbel_gen: Optional[torch.Generator] = None         # exists only with the option on: no draw, no state without it
        if self.gumbel_sampling:
            self.gumbel_tau = gumbel_tau(getattr(model, "gumbel_kwargs", None) if gumbel_kwargs is None else gumbel_kwargs)
            self.gumbel_gen = torch.Generator(device=dev).manual_seed(int(seed))

    # ---------------------------------------------------------------- training state (base_trainer.py:178-214 saves optimizer + scheduler state)
    def training_state(self, current_iter: int) -> Dict:
        st = {"iter": int(current_iter), "rng": self.rng.get_state()}
        for tag, opt_, sch in (("g", self.g_opt, self.g_sched), ("d", self.d_opt, self.d_sched)):
            st[tag] = dict(adam_state(opt_), last_epoch=int(sch.last_epoch))
        if self.gumbel_gen is not None:
            st["gumbel_gen"] = self.gumbel_gen.get_state().clone()
        return st

    def load_training_state(self, st: Dict) -> int:
        for tag, opt_, sch in (("g", self.g_opt, self.g_sched), ("d", self.d_opt, self.d_sched)):
            load_adam_state(opt_, st[tag], tag)
            sch.last_epoch = int(st[tag]["last_epoch"])
        if "rng" in st:
            self.rng.set_state(st["rng"])
        if self.gumbel_gen is not None:
            if "gumbel_gen" not in st:
                raise ValueError("training state: no gumbel_gen entry, it was saved by a run without model.gumbel_sampling")
            self.gumbel_gen.set_state(st["gumbel_gen"].cpu())
        return int(st["iter"])

    def resync_parameters(self) -> None:
        """After a state dict was loaded into the modules: parameters are views of the flat buffers, so load_state_dict's copy_
        already wrote them; cached packed weights are stale."""
        self.g_group.refresh_plans(); self.d_group.refresh_plans()
        self._drop_inference_graphs()

    def checkpoint_modules(self) -> Dict[str, torch.nn.Module]:
        """{name: module} of what a checkpoint holds beside the training state: <name>_iterXXXXXXX.pth.tar = {'iter', name: state_dict}."""
        return {"comp_model": self.model, "discriminator": self.D}

    @torch.no_grad()
    def generator_forward(self, ctx: Ctx, real: Tensor, vq_indices: Optional[Tensor], beta_rate, beta_vq):
        """run_comp_model (:116-133) -> forward (hyperprior_dc_vic_model.py:208-274, is_train, fix_entropy_models)."""
        m = self.model
        x = real.to(self.device, dtype=torch.float32).contiguous()
        gt_lat, gt_idx, feat = m.vq_encode(x, vq_indices, want_feat=True)                      # frozen VQGAN, no grad
        y = m.comp_encode(x, gt_lat, gt_idx, enc_kwargs=dict(beta_1=beta_rate, beta_2=beta_vq), feat=feat)
        e = m._entropy_encode_side(y, want_symbols=False)                                      # fix_entropy_models: no grad
        y_hat = e["y_hat"]
        gumbel = None
        if self.gumbel_sampling:
            # :254-260, one e per logit: [N, n_embed] over the VQ token grid
            n_embed = m.vq_model.quantize.embedding.weight.shape[0]
            gumbel = (self.draw_gumbel_noise(x.new_empty((x.shape[0], n_embed) + tuple(gt_lat.shape[-2:]))), self.gumbel_tau)
        s = nets.synthesis_forward(ctx, m, y_hat, beta_rate, beta_vq, gumbel)
        return dict(s, real=x, gt_vq_latent=gt_lat, gt_vq_indices=gt_idx, y_hat=y_hat, qbpp=self.qbpp(e["bits_y"], e["bits_z"], x))

    def draw_gumbel_noise(self, logits: Tensor) -> Tensor:
        """e ~ Exp(1) of the logits' shape from the trainer's generator: -log(e) is the Gumbel noise F.gumbel_softmax draws."""
        return torch.empty_like(logits).exponential_(generator=self.gumbel_gen)

    def calc_g_loss(self, ctx: Ctx, o: Dict, beta_rate, beta_vq) -> Dict[str, Tensor]:
        """:192-234; each term seeds its gradient on the tape."""
        w = self.w
        log = {}
        log["distortion"] = A.mse_loss(ctx, o["fake"], o["real"], w["distortion"] * self.distortion_factor)   # 0.25: MSELoss on [0,1], ((a+1)/2-(b+1)/2)^2
        log["perceptual"] = self.perceptual_term(ctx, o["real"], o["fake"])
        g_fake = nets.discriminator_forward(ctx, self.D, o["fake"], beta_rate, beta_vq)
        log["adv"] = self.calc_adv_loss(ctx, g_fake, o["gt_vq_indices"])
        w_cd = w["code_distortion"] * (o["gt_vq_latent"].numel() if self.code_distortion_reduction == "sum" else 1)
        log["code_distortion"] = A.mse_loss(ctx, o["pred_embed"], o["gt_vq_latent"], w_cd)
        if self.code_ce_loss is None:
            log["code_ce"] = A.cross_entropy_loss(ctx, o["logits"], o["gt_vq_indices"], w["code_ce"])
        else:
            log["code_ce"] = self.code_ce_loss(ctx, o["logits"], o["gt_vq_indices"])
        return log

    def calc_adv_loss(self, ctx: Ctx, g_fake, gt_vq_indices: Tensor) -> Tensor:
        """The generator's adversarial term: gan_loss(D(fake), is_real=True, is_disc=False) (:213-216)."""
        return A.bce_logits_loss(ctx, g_fake, True, self.w["gan"])

    def optimize_parameters(self, current_iter: int, data_dict: Dict) -> Optional[Dict[str, float]]:
        real = data_dict["real_images"]
        beta_rate, beta_vq = self.step_beta_pair(data_dict, real.shape[0])
        # ---------------------------------------------------------------- train G
        self.g_group.zero_grad()
        ctx = Ctx([self.g_group])                      # D's parameters receive no gradient here (requires_grad_(False), :146)
        o = self.generator_forward(ctx, real, data_dict.get("vq_indices"), beta_rate, beta_vq)
        g_log = self.calc_g_loss(ctx, o, beta_rate, beta_vq)
        total = sum(float(v.item()) for v in g_log.values())
        if self.skip_step(total, ctx):
            return None
        self.apply_gradients(ctx, self.g_opt, self.g_sched.lr(), self.clip)
        self._drop_inference_graphs()
        lr_now = self.g_sched.lr()
        self.g_sched.step()
        # ---------------------------------------------------------------- train D
        self.d_group.zero_grad()
        dctx = Ctx([self.d_group])
        fake_det = o["fake"].data                      # .detach()
        self.last_fake = fake_det
        d_real, d_fake = self.run_discriminator(dctx, o["real"], fake_det, beta_rate, beta_vq)
        l_real, l_fake = self.calc_d_loss(dctx, d_real, d_fake, o["gt_vq_indices"])
        self.apply_gradients(dctx, self.d_opt, self.d_sched.lr())
        self.d_sched.step()
        log = {k: float(v.item()) for k, v in g_log.items()}
        out_d_real, out_d_fake = self.calc_avg_d_score_for_log(d_real, d_fake)
        log.update(total=total, qbpp=o["qbpp"], vq_acc=self.vq_acc(o), lr=lr_now, d_real=float(l_real.item()), d_fake=float(l_fake.item()),
                   d_total=float(l_real.item()) + float(l_fake.item()), out_d_real=out_d_real, out_d_fake=out_d_fake)
        return log

    # :236-300 (run_discriminator, calc_d_loss, calc_avg_d_score_for_log): the hooks a subclass with another adversarial loss overrides
    def run_discriminator(self, dctx: Ctx, real: Tensor, fake_det: Tensor, beta_rate, beta_vq):
        d_real = nets.discriminator_forward(dctx, self.D, A.const(real), beta_rate, beta_vq)
        d_fake = nets.discriminator_forward(dctx, self.D, A.const(fake_det), beta_rate, beta_vq)
        return d_real, d_fake

    def calc_d_loss(self, dctx: Ctx, d_real, d_fake, gt_vq_indices: Tensor):
        """(0.5 * loss on real, 0.5 * loss on fake), each seeding its gradient on the tape."""
        l_real = A.bce_logits_loss(dctx, d_real, True, 0.5)
        l_fake = A.bce_logits_loss(dctx, d_fake, False, 0.5)
        return l_real, l_fake

    def calc_avg_d_score_for_log(self, d_real, d_fake) -> Tuple[float, float]:
        return float(d_real.data.mean().item()), float(d_fake.data.mean().item())


# ---------------------------------------------------------------------------------------------------- OASIS GAN loss / trainer
def _verify_logit_target_shape(logits_shape, target: Tensor) -> None:
    """src/losses/oasis_gan_loss.py:17-28, same messages."""
    if len(logits_shape) != 4:
        raise ValueError("Only expect 4-dimensional logits.")
    expected_target_numel = logits_shape[0] * logits_shape[-2] * logits_shape[-1]
    actual_target_shape = target.numel()
    if expected_target_numel != actual_target_shape:
        raise ValueError(f"Based on logits size {logits_shape}, expected target numel to be "
                         f"{expected_target_numel}, but found {actual_target_shape}")


@LOSS_REGISTRY.register()
class OasisGANLoss:
    """src/losses/oasis_gan_loss.py:31-79: the discriminator classifies every VQ token position into n_embed + 1 classes (0 = fake,
    k + 1 = real with codebook entry k); every adversarial term is a cross entropy against the ground-truth indices.  `loss_weight`
    multiplies the generator side only (is_disc=False).  `logits` is a `Var` (or a tensor): value, gradient and the optional log
    score come from one launch of dcvic_oasis_ce_f32; `weight` is the trainer's extra factor (0.5 on the D side)."""

    def __init__(self, loss_weight: float):
        self.lamb_gan = float(loss_weight)

    def __call__(self, ctx: Ctx, logits, target: Tensor, is_disc: bool, is_real: bool, weight: float = 1.0, want_score: bool = False):
        lv = logits if isinstance(logits, A.Var) else A.const(logits)
        _verify_logit_target_shape(lv.data.shape, target)
        if target.dtype != torch.long:
            raise ValueError("Expected target to have dtype torch.long.")
        return A.oasis_gan_loss(ctx, lv, target, is_real, weight * (1.0 if is_disc else self.lamb_gan), want_score=want_score)


@TRAINER_REGISTRY.register()
class DualBetaCondOasisGanDistortionVqFusionTrainer(DualBetaCondGanDistortionVqCodeTrainer):
    """src/trainer/dual_cond_oasis_gan_distortion_vq_code_trainer.py:16-113 (config/dc_vic_oasis.yaml): the stage-3 trainer with the
    OASIS adversarial loss.  Overrides what the reference overrides -- the adversarial term of calc_g_loss, calc_d_loss and the
    out_d_* log values (mean over the channels 1:) -- and inherits everything else.  `trainer.mc_sampling` (a D half of the batch
    with dataset-supplied indices) is not built."""

    def __init__(self, model, discriminator, *args, **kwargs):
        n_embed = int(model.vq_model.quantize.embedding.weight.shape[0])
        unet = isinstance(discriminator, nets.OasisDualBetaCondTamingNLayerDiscriminator)
        last = discriminator.head[-1] if unet else discriminator.main[-1]
        if int(last.out_channels) != n_embed + 1:
            raise ValueError(f"OASIS discriminator: out_nc is {int(last.out_channels)}, the model's codebook needs n_embed + 1 = {n_embed + 1} classes")
        if unet:
            if discriminator.logit_stride != 8:
                raise ValueError(f"OASIS U-Net discriminator: its logits lie on a grid of 2^(n_layers - num_upsample) = {discriminator.logit_stride} "
                                 "pixels, the VQ tokens on one of 8")
        elif int(last.kernel_size) != 3:
            raise ValueError("OASIS discriminator: keep_shape must be True so that the logits map is the VQ token grid (H / 8 x W / 8)")
        super().__init__(model, discriminator, *args, **kwargs)
        self.gan_loss = OasisGANLoss(self.w["gan"])
        self._d_scores: Optional[Tuple[Tensor, Tensor]] = None

    def calc_adv_loss(self, ctx: Ctx, g_fake, gt_vq_indices: Tensor) -> Tensor:
        return self.gan_loss(ctx, g_fake, gt_vq_indices, is_disc=False, is_real=True)

    def calc_d_loss(self, dctx: Ctx, d_real, d_fake, gt_vq_indices: Tensor):
        l_real, s_real = self.gan_loss(dctx, d_real, gt_vq_indices, is_disc=True, is_real=True, weight=0.5, want_score=True)
        l_fake, s_fake = self.gan_loss(dctx, d_fake, gt_vq_indices, is_disc=True, is_real=False, weight=0.5, want_score=True)
        self._d_scores = (s_real, s_fake)
        return l_real, l_fake

    def calc_avg_d_score_for_log(self, d_real, d_fake) -> Tuple[float, float]:
        s_real, s_fake = self._d_scores
        return float(s_real.item()), float(s_fake.item())
