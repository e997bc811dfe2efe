"""The trainer a parsed config asks for: which one (choose_trainer, choose_gan_trainer, read_gumbel_options), the constructors' keyword
arguments from the YAML's `trainer` / `optim` / `loss` / `model` sections (rd_trainer_kwargs, rd_stage_1_1_kwargs with read_g_scheduler and
read_rd_optimizers, gan_trainer_kwargs: pure, no GPU, no model)
and the built trainer with its `[train]` log lines (build_trainer): one place for scripts/train.py, the benchmarks under tools/ and the tests."""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Tuple

from ..registry import TRAINER_REGISTRY
from .losses import build_code_ce_loss
from .rd_trainer import DEFAULT_RD_LOSS
from .trainer import DEFAULT_LOSS, gumbel_tau


def get_in(d, *keys, default=None):
    for k in keys:
        try:
            d = d[k]
        except (KeyError, TypeError):
            return default
    return d


VANILLA_TRAINER, OASIS_TRAINER = "DualBetaCondGanDistortionVqCodeTrainer", "DualBetaCondOasisGanDistortionVqFusionTrainer"
_TRAINER_KIND = {VANILLA_TRAINER: "vanilla", OASIS_TRAINER: "oasis"}
_LOSS_KIND = {"VanillaGANLoss": "vanilla", "OasisGANLoss": "oasis"}
RD_TRAINER, RD_STAGE_1_1 = "DualBetaCondRateDistortionVqCodeTrainer", "RateDistortionVqCodeTrainer"
UNCONDITIONED_MODEL = "HyperpriorCharmVicModel"        # the model stage 1-1 trains
# the discriminator of a config without a `discriminator` section: the stage-3 PatchGAN
DEFAULT_DISCRIMINATOR = dict(type="DualBetaCondTamingNLayerDiscriminator", input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0,
                             max_beta_2=3.5, L=10, cond_ch=8, use_pi=False, include_x=True)


PATCHGAN, UNET = "DualBetaCondTamingNLayerDiscriminator", "OasisDualBetaCondTamingNLayerDiscriminator"
VQ_TOKEN_STRIDE = 8         # pixels per VQ token: the OASIS loss classifies one logit column per token


def read_discriminator(opt) -> Dict[str, Any]:
    """The `discriminator` section of a parsed config (pure: no GPU, no module) -> dict(type, kwargs: the section's other keys unchanged,
    norm_type and norm_kwargs as they take effect, norm_type_given, line: the `[train]` log line).  A config without the section gets
    DEFAULT_DISCRIMINATOR.  SystemExit, naming the key and its value, for an unknown type and for everything the classes do not build."""
    from . import nets
    d = dict(get_in(opt, "discriminator", default=None) or DEFAULT_DISCRIMINATOR)
    d_type = d.pop("type", PATCHGAN)
    if d_type not in (PATCHGAN, UNET):
        raise SystemExit(f"discriminator.type: {d_type} is unknown, expected {PATCHGAN} or {UNET}")
    given = "norm_type" in d or bool(d.get("use_actnorm", False))
    try:
        norm_type, nk = nets.resolve_norm(d.get("norm_type", "none"), bool(d.get("use_actnorm", False)), d.get("norm_kwargs"))
        nets.refuse_y_hat_cond(d.get("y_hat_cond", False))
        n_layers = int(d.get("n_layers", 3))
        if n_layers < 1:
            raise ValueError(f"n_layers: {n_layers}, needs at least 1")
        if d_type == UNET:
            nets.check_unet_options(n_layers, int(d.get("num_upsample", 1)), int(d.get("cond_ch", 8)), int(d.get("input_nc", 3)))
    except (NotImplementedError, ValueError) as e:
        raise SystemExit(f"discriminator.{e}")
    line = f"discriminator: {d_type}, n_layers {n_layers}, norm {norm_type}"
    if norm_type == "batchnorm":
        line += f" (eps {nk.get('eps', 1e-5):g}, momentum {nk.get('momentum', 0.1):g})"
    if d_type == UNET:
        line += f", num_upsample {int(d.get('num_upsample', 1))}"
    if not given:
        line += "; the YAML names no norm_type: the reference's class default is batchnorm, none is in effect here"
    return dict(type=d_type, kwargs=d, norm_type=norm_type, norm_kwargs=nk, norm_type_given=given, line=line)


def build_discriminator(opt, device):
    """(the discriminator `opt` asks for, on `device`; its `[train]` log line).  The caller seeds torch's generator first."""
    from ..registry import DISCRIMINATOR_REGISTRY
    r = read_discriminator(opt)
    return DISCRIMINATOR_REGISTRY.get(r["type"])(**r["kwargs"]).to(device), r["line"]


def choose_gan_trainer(opt, gan_flag=None):
    """(kind, trainer class name, reason) for a parsed config (pure: no GPU, no model).  Order: the --gan flag; `trainer.type`;
    `loss.gan_loss.type`; the discriminator's `out_nc` (absent or 1 -> vanilla, n_embed + 1 -> oasis).  SystemExit for an unknown
    type, for `trainer.mc_sampling` (not built) and for a choice the discriminator cannot serve: OASIS needs out_nc = n_embed + 1
    of the VQ codebook and keep_shape (one 257-way classification per token), the BCE PatchGAN must not get that discriminator."""
    n_embed = get_in(opt, "subnet", "vq_model", "n_embed")
    out_nc = int(get_in(opt, "discriminator", "out_nc", default=1))
    keep_shape = bool(get_in(opt, "discriminator", "keep_shape", default=False))
    if get_in(opt, "trainer", "mc_sampling", default=False):
        raise SystemExit("trainer.mc_sampling: true is not built (the reference's split of a batch into a generator half and a discriminator "
                         "half with dataset-supplied VQ indices): set it to false")
    t_type, l_type = get_in(opt, "trainer", "type"), get_in(opt, "loss", "gan_loss", "type")
    if gan_flag is not None:
        if gan_flag not in ("vanilla", "oasis"):
            raise SystemExit(f"--gan {gan_flag}: unknown, expected vanilla or oasis")
        kind, reason = gan_flag, f"--gan {gan_flag}"
    elif t_type is not None:
        if t_type not in _TRAINER_KIND:
            raise SystemExit(f"trainer.type: {t_type} is unknown, expected {VANILLA_TRAINER} or {OASIS_TRAINER}")
        kind, reason = _TRAINER_KIND[t_type], f"trainer.type: {t_type}"
    elif l_type is not None:
        if l_type not in _LOSS_KIND:
            raise SystemExit(f"loss.gan_loss.type: {l_type} is unknown, expected VanillaGANLoss or OasisGANLoss")
        kind, reason = _LOSS_KIND[l_type], f"loss.gan_loss.type: {l_type}"
    elif out_nc == 1:
        kind, reason = "vanilla", "discriminator.out_nc: 1"
    elif n_embed is not None and out_nc == int(n_embed) + 1:
        kind, reason = "oasis", f"discriminator.out_nc: {out_nc} = n_embed + 1"
    else:
        raise SystemExit(f"discriminator.out_nc: {out_nc} names no GAN loss (1 -> vanilla, n_embed + 1 = "
                         f"{'?' if n_embed is None else int(n_embed) + 1} -> oasis) and neither --gan, trainer.type nor loss.gan_loss.type is given")
    if gan_flag is None and t_type in _TRAINER_KIND and l_type in _LOSS_KIND and _TRAINER_KIND[t_type] != _LOSS_KIND[l_type]:
        raise SystemExit(f"trainer.type: {t_type} cannot train with loss.gan_loss.type: {l_type}")
    if kind == "oasis":
        if n_embed is None:
            raise SystemExit(f"OASIS GAN loss ({reason}) needs subnet.vq_model.n_embed to size the discriminator's classes")
        if out_nc != int(n_embed) + 1:
            raise SystemExit(f"OASIS GAN loss ({reason}) cannot train a discriminator with out_nc: {out_nc}; it needs n_embed + 1 = {int(n_embed) + 1}")
        if get_in(opt, "discriminator", "type") == UNET:          # keep_shape does not apply: the up blocks set the logits' grid
            n_layers, n_up = int(get_in(opt, "discriminator", "n_layers", default=3)), int(get_in(opt, "discriminator", "num_upsample", default=1))
            if 2 ** (n_layers - n_up) != VQ_TOKEN_STRIDE:
                raise SystemExit(f"OASIS GAN loss ({reason}) cannot train a U-Net discriminator with n_layers: {n_layers} and num_upsample: {n_up}; "
                                 f"its logits lie on a grid of 2^(n_layers - num_upsample) = {2 ** max(n_layers - n_up, 0)} pixels, the VQ tokens on one of "
                                 f"{VQ_TOKEN_STRIDE}")
        elif not keep_shape:
            raise SystemExit(f"OASIS GAN loss ({reason}) cannot train a discriminator with keep_shape: false; its logits must lie on the VQ token grid")
    elif n_embed is not None and out_nc == int(n_embed) + 1 and out_nc != 1:
        raise SystemExit(f"vanilla GAN loss ({reason}) cannot train a discriminator with out_nc: {out_nc} (n_embed + 1 classes: an OASIS "
                         "discriminator); use --gan oasis or out_nc: 1")
    return kind, (OASIS_TRAINER if kind == "oasis" else VANILLA_TRAINER), reason


def read_gumbel_options(opt):
    """(gumbel_sampling, tau) of a parsed config's `model` section for the GAN-stage trainers (pure: no GPU, no model), called after
    choose_gan_trainer.  `model.gumbel_kwargs` may hold `tau` (a number > 0, default 1) and nothing else: the sample is the reference's
    F.gumbel_softmax(logits, dim=1, hard=True, **gumbel_kwargs), so `hard` and `dim` would raise there and `eps` does nothing.
    SystemExit names the key and its value.  The keywords are checked with the option off too, as the model's constructor takes them."""
    kw = get_in(opt, "model", "gumbel_kwargs", default=None)
    try:
        tau = gumbel_tau(dict(kw) if kw else None)
    except ValueError as e:
        raise SystemExit(str(e))
    return bool(get_in(opt, "model", "gumbel_sampling", default=False)), tau


def choose_trainer(opt, gan_flag=None):
    """(kind, trainer class name, reason) for a parsed config (pure: no GPU, no model): kind "rd" for the stage 1-2 rate-distortion
    trainer (`trainer.type: DualBetaCondRateDistortionVqCodeTrainer`) and for the stage 1-1 trainer (`RateDistortionVqCodeTrainer` over
    `model.type: HyperpriorCharmVicModel`), else choose_gan_trainer's answer.  SystemExit for the stage 1-1 trainer over any other model
    type, for --gan together with a rate-distortion trainer type, and for what those trainers do not build."""
    t_type = get_in(opt, "trainer", "type")
    if t_type not in (RD_TRAINER, RD_STAGE_1_1):
        return choose_gan_trainer(opt, gan_flag)
    m_type = get_in(opt, "model", "type")
    if t_type == RD_STAGE_1_1 and m_type != UNCONDITIONED_MODEL:
        raise SystemExit(f"trainer.type: {t_type} (stage 1-1, config/exp1_stage1_1.yaml) is not built for model.type: {m_type}: it trains the "
                         f"unconditioned {UNCONDITIONED_MODEL} (ElicVqCatScEncoder, ElicFeatFusionDecoder, no beta pair) under a "
                         f"LinearWarmupScheduler; the dual-conditioned models train with the stage 1-2 trainer {RD_TRAINER}")
    if gan_flag is not None:
        raise SystemExit(f"--gan {gan_flag} cannot go with trainer.type: {t_type}: the rate-distortion trainer has no discriminator and no GAN loss")
    if get_in(opt, "model", "gumbel_sampling", default=False):
        raise SystemExit("model.gumbel_sampling: true is not built (the Gumbel-softmax sampling of the VQ indices in training mode): set it to false")
    if get_in(opt, "loss", "gan_loss") is not None:
        raise SystemExit(f"loss.gan_loss has no place under trainer.type: {t_type}: it trains no GAN loss")
    if t_type == RD_STAGE_1_1:
        for entry in ("rate_loss", "code_distortion_loss", "code_ce_loss"):
            if get_in(opt, "loss", entry, "reduction") == "none":
                raise SystemExit(f"loss.{entry}.reduction: none has no meaning under trainer.type: {t_type}: it keeps the per-image terms for the "
                                 "beta weights of the dual-conditioned trainer, and this one has none; use mean or sum")
        read_g_scheduler(opt)
        read_rd_optimizers(opt)
        return "rd", RD_STAGE_1_1, f"trainer.type: {t_type}, model.type: {m_type}"
    policy = get_in(opt, "trainer", "beta_policy", default="linear")
    if policy not in ("linear", "exp"):
        raise SystemExit(f"trainer.beta_policy: {policy} is unknown, expected linear or exp")
    return "rd", RD_TRAINER, f"trainer.type: {t_type}"


def _optim_kwargs(opt) -> Dict[str, Any]:
    """What both kinds of trainer read from `optim`: the generator side's schedule and the clip, with the stage-3 values when absent."""
    return dict(milestones=list(get_in(opt, "optim", "g_scheduler", "milestones", default=[300000])),
                gamma=float(get_in(opt, "optim", "g_scheduler", "gamma", default=0.1)), clip_max_norm=get_in(opt, "optim", "clip_max_norm", default=1.0))


def weight_load_report(report: Dict[str, List[str]], depth: int = 2) -> Optional[str]:
    """One line for BaseModel.load_learned_weight's answer when the checkpoint and the model differ in keys (a stage 1-1 file loaded
    into the dual-conditioned model of stage 1-2: its conditioning modules keep their constructor initialisation), None when they agree:
    the number of tensors loaded, then the missing and the unexpected keys grouped by their first `depth` name parts, with counts."""
    if not report["missing"] and not report["unexpected"]:
        return None

    def groups(keys: List[str]) -> str:
        count: Dict[str, int] = {}
        for k in keys:
            g = ".".join(k.split(".")[:depth])
            count[g] = count.get(g, 0) + 1
        return ", ".join(f"{g} {n}" for g, n in count.items()) or "none"
    return (f"weights: {len(report['loaded'])} tensors loaded; missing in the checkpoint (kept as initialised): {groups(report['missing'])}; "
            f"unexpected in the checkpoint (dropped): {groups(report['unexpected'])}")


def from_scratch_vqgan(opt) -> str:
    """The VQGAN checkpoint a stage 1-1 run from the initialisation starts with (pure but for one os.path.exists): the path of
    `subnet.vq_model.ckpt_path`, or SystemExit when it is absent or names no file -- a random frozen VQGAN trains nothing."""
    ck = get_in(opt, "subnet", "vq_model", "ckpt_path")
    if not ck:
        raise SystemExit("subnet.vq_model.ckpt_path is absent: a run without --model_path starts from the initialisation and needs the pretrained "
                         "VQGAN (frozen: a random one trains nothing); pass --synthetic_weights to run without one")
    if not os.path.exists(ck):
        raise SystemExit(f"subnet.vq_model.ckpt_path: {ck} does not exist: a run without --model_path starts from the initialisation and needs the "
                         "pretrained VQGAN (frozen: a random one trains nothing); pass --synthetic_weights to run without one")
    return ck


def read_g_scheduler(opt) -> Dict[str, Any]:
    """`optim.g_scheduler` of a parsed config (pure) -> dict(type="MultiStepLR", milestones, gamma) for that type or an absent one (the
    stage-3 values when absent), dict(type="LinearWarmupScheduler", warmup_iters, warmup_factor) for the stage 1-1 schedule.
    SystemExit with the YAML key and value for any other type (LinearWarmupMultiStepLR included) and for a malformed argument."""
    sec = dict(get_in(opt, "optim", "g_scheduler", default=None) or {})
    t = sec.pop("type", "MultiStepLR")
    if t == "MultiStepLR":
        return dict(type=t, milestones=list(sec.get("milestones", [300000])), gamma=float(sec.get("gamma", 0.1)))
    if t != "LinearWarmupScheduler":
        raise SystemExit(f"optim.g_scheduler.type: {t} is not built, expected MultiStepLR or LinearWarmupScheduler")
    for k in sec:
        if k not in ("warmup_iters", "warmup_factor"):
            raise SystemExit(f"optim.g_scheduler.{k}: {sec[k]!r} is not a keyword of LinearWarmupScheduler (warmup_iters, warmup_factor)")
    for k in ("warmup_iters", "warmup_factor"):
        if k not in sec:
            raise SystemExit(f"optim.g_scheduler.{k} is missing: LinearWarmupScheduler has no default for it")
    it, f = sec["warmup_iters"], sec["warmup_factor"]
    if isinstance(it, bool) or not isinstance(it, int) or it < 0:
        raise SystemExit(f"optim.g_scheduler.warmup_iters: {it!r} is not an integer >= 0")
    if isinstance(f, bool) or not isinstance(f, (int, float)):
        raise SystemExit(f"optim.g_scheduler.warmup_factor: {f!r} is not a number")
    return dict(type=t, warmup_iters=it, warmup_factor=float(f))


def read_rd_optimizers(opt) -> Dict[str, float]:
    """`optim.g_optimizer` / `optim.aux_optimizer` for the stage 1-1 trainer (pure) -> dict(lr, aux_lr): `type: Adam` (or absent) with
    `lr` (default 1e-4 / 1e-3) is honoured; another type or any further keyword is refused by key."""
    out = {}
    for entry, name, default in (("g_optimizer", "lr", 1e-4), ("aux_optimizer", "aux_lr", 1e-3)):
        sec = dict(get_in(opt, "optim", entry, default=None) or {})
        if sec.get("type", "Adam") != "Adam":
            raise SystemExit(f"optim.{entry}.type: {sec['type']} is not built, expected Adam")
        for k in sec:
            if k not in ("type", "lr"):
                raise SystemExit(f"optim.{entry}.{k}: {sec[k]!r} is not built: Adam runs with lr alone (betas 0.9 / 0.999, eps 1e-8, no weight decay)")
        lr = sec.get("lr", default)
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not lr > 0:
            raise SystemExit(f"optim.{entry}.lr: {lr!r} is not a number > 0")
        out[name] = float(lr)
    return out


def rd_stage_1_1_kwargs(opt, losses) -> Dict[str, Any]:
    """The stage 1-1 trainer's keyword arguments (all but model, dist, seed, lpips_state) from a parsed config and its read_loss_section."""
    lw = {k: v for k, v in losses["weights"].items() if k in DEFAULT_RD_LOSS}
    rate = losses["rate"] or dict(loss_weight=None, reduction="mean")
    if rate["loss_weight"] is not None:
        lw["rate"] = rate["loss_weight"]
    return dict(**read_rd_optimizers(opt), scheduler=read_g_scheduler(opt), clip_max_norm=get_in(opt, "optim", "clip_max_norm", default=1.0),
                loss_weights=lw, rate_reduction=rate["reduction"], code_ce_gamma=losses["code_ce"]["gamma"],
                code_ce_reduction=losses["code_ce"]["reduction"], code_distortion_reduction=losses["code_distortion_reduction"],
                distortion_factor=losses["distortion_factor"], distortion_type=losses["distortion_type"],
                gumbel_sampling=bool(get_in(opt, "model", "gumbel_sampling", default=False)))


def rd_trainer_kwargs(opt, losses) -> Dict[str, Any]:
    """The rate-distortion trainer's keyword arguments (all but model, dist, seed, lpips_state) from a parsed config and its read_loss_section."""
    lw = {k: v for k, v in losses["weights"].items() if k in DEFAULT_RD_LOSS}
    rate = losses["rate"] or dict(loss_weight=None, reduction="mean")
    if rate["loss_weight"] is not None:
        lw["rate"] = rate["loss_weight"]
    return dict(lr=float(get_in(opt, "optim", "g_optimizer", "lr", default=1e-4)), aux_lr=float(get_in(opt, "optim", "aux_optimizer", "lr", default=1e-3)),
                **_optim_kwargs(opt), loss_weights=lw, beta_policy=get_in(opt, "trainer", "beta_policy", default="linear"),
                beta_offset=float(get_in(opt, "trainer", "beta_offset", default=1.0)),
                sample_beta_batch=bool(get_in(opt, "trainer", "sample_beta_batch", default=False)), rate_reduction=rate["reduction"],
                code_ce_gamma=losses["code_ce"]["gamma"], code_ce_reduction=losses["code_ce"]["reduction"],
                code_distortion_reduction=losses["code_distortion_reduction"], distortion_factor=losses["distortion_factor"],
                distortion_type=losses["distortion_type"], gumbel_sampling=bool(get_in(opt, "model", "gumbel_sampling", default=False)))


def gan_trainer_kwargs(opt, losses, gumbel: Tuple[bool, float]) -> Dict[str, Any]:
    """The GAN-stage trainers' keyword arguments (all but model, discriminator, dist, seed, lpips_state); `gumbel`: read_gumbel_options' pair."""
    lw = dict(losses["weights"])
    return dict(lr_g=float(get_in(opt, "optim", "g_optimizer", "lr", default=1e-4)), lr_d=float(get_in(opt, "optim", "d_optimizer", "lr", default=1e-4)),
                **_optim_kwargs(opt), loss_weights=lw, sample_beta_batch=bool(get_in(opt, "trainer", "sample_beta_batch", default=True)),
                d_milestones=get_in(opt, "optim", "d_scheduler", "milestones", default=None), d_gamma=get_in(opt, "optim", "d_scheduler", "gamma", default=None),
                code_ce_loss=build_code_ce_loss(losses["code_ce"], lw.get("code_ce", DEFAULT_LOSS["code_ce"])),
                distortion_factor=losses["distortion_factor"], code_distortion_reduction=losses["code_distortion_reduction"],
                gumbel_sampling=gumbel[0], gumbel_kwargs=dict(tau=gumbel[1]))


def build_rd_trainer(opt, losses, model, dist, seed, lpips_state):
    """The rate-distortion trainer from the YAML's `trainer`, `optim` and `loss` sections -> (trainer, the `[train]` log line)."""
    kw = rd_trainer_kwargs(opt, losses)
    trainer = TRAINER_REGISTRY.get(RD_TRAINER)(model, dist=dist, seed=seed, lpips_state=lpips_state, **kw)
    line = (f"rate-distortion trainer: {RD_TRAINER}; beta_policy {kw['beta_policy']}" + (f" (offset {kw['beta_offset']:g})" if kw["beta_policy"] == "linear" else "")
            + f", sample_beta_batch {kw['sample_beta_batch']}; weights " + ", ".join(f"{k} {trainer.w[k]:g}" for k in DEFAULT_RD_LOSS)
            + f"; reductions rate {kw['rate_reduction']}, code_distortion {kw['code_distortion_reduction']}, code_ce {kw['code_ce_reduction']}"
            + f" (gamma {kw['code_ce_gamma']:g}); distortion {trainer.distortion_type}")
    return trainer, line


def build_rd_stage_1_1_trainer(opt, losses, model, dist, seed, lpips_state):
    """The stage 1-1 trainer from the YAML's `optim` and `loss` sections -> (trainer, the `[train]` log line)."""
    kw = rd_stage_1_1_kwargs(opt, losses)
    trainer = TRAINER_REGISTRY.get(RD_STAGE_1_1)(model, dist=dist, seed=seed, lpips_state=lpips_state, **kw)
    sch = dict(kw["scheduler"])
    line = (f"rate-distortion trainer: {RD_STAGE_1_1}; weights " + ", ".join(f"{k} {trainer.w[k]:g}" for k in DEFAULT_RD_LOSS)
            + f"; code_ce gamma {kw['code_ce_gamma']:g}; distortion {trainer.distortion_type}; lr {kw['lr']:g}, aux lr {kw['aux_lr']:g}; scheduler "
            + sch.pop("type") + " (" + ", ".join(f"{k} {v}" for k, v in sch.items()) + ")")
    return trainer, line


def build_trainer(opt, losses, model, discriminator, dist, seed, lpips_state, gan_flag: Optional[str] = None) -> Tuple[Any, List[str]]:
    """The trainer `opt` (with the --gan flag) asks for over `model` and, for a GAN one, `discriminator` -> (trainer, its `[train]` log lines)."""
    kind, name, reason = choose_trainer(opt, gan_flag)
    if kind == "rd":
        build = build_rd_stage_1_1_trainer if name == RD_STAGE_1_1 else build_rd_trainer
        trainer, line = build(opt, losses, model, dist, seed, lpips_state)
        return trainer, [line, "losses: " + losses["line"]]
    on, tau = read_gumbel_options(opt)
    kw = gan_trainer_kwargs(opt, losses, (on, tau))
    lw = kw["loss_weights"]
    w_src = "loss.gan_loss.loss_weight" if "gan" in lw else "default, no reference YAML pins it" if kind == "oasis" else "default"
    lines = [f"GAN trainer: {kind} ({name}), chosen by {reason}; generator-side gan weight {lw.get('gan', DEFAULT_LOSS['gan']):g} ({w_src})",
             "losses: " + losses["line"] + "; weights " + ", ".join(f"{k} {lw.get(k, v):g}" for k, v in DEFAULT_LOSS.items()),
             "VQ sampling: " + (f"gumbel-softmax (tau {tau:g})" if on else "argmax")]
    return TRAINER_REGISTRY.get(name)(model, discriminator, dist=dist, seed=seed, lpips_state=lpips_state, **kw), lines
