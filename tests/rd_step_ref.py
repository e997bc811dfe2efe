"""One stage 1-2 training step restated in plain torch on the CPU (no test in here; used by test_gpu_rd_trainer.py).

It composes tests/analysis_train_ref.py (encoder + estimate_entropy(is_train=True), fp64) with the oracle's elic_decoder_feats,
swin_estimator, fusion_decode and lpips_alex (`synth_dtype`: fp32 by default, as the stage-3 step test runs them; they accept fp64 too,
which takes 6 s in place of 1.7 s at 2 x 64x64 and moves no gradient by more than 3.4e-6 of its max on the step test's inputs) into ONE
autograd graph: y_hat leaves the fp64 analysis side through a cast, so total.backward() carries the image and code losses' gradient
through the straight-through estimators into the encoder, the hyperprior and CHARM.  The losses are written in the reference trainer's
own words (dual_cond_rate_distortion_vq_code_trainer.py:71-108, 153-200): `reduction='none'` maps, `_calc_batch_bpp`,
`apply_loss_weight`, `calc_vq_rate_loss_weight`.

Rounded symbols and the estimator's argmax are decisions: `force` gives the product's (dict(y=, z=, out_idx=)); the helper's own are
returned beside them with their distance from a tie.  The sign of a ReLU's input is a decision of the same kind: the networks are
piecewise linear, and two evaluations have comparable gradients only on the same piece.  About 30 of a step's 10^7 ReLU inputs lie
within 2e-6 of zero on the step test's inputs, where an fp32 convolution and this fp64 one can land on different sides; one such
position switches that position's whole contribution to one output channel's weight gradient.  `force["relu"]` (a ReluDecisions over the
product's ReLU outputs) therefore replaces relu(x) by x * [the product's output > 0] in the encoder, the hyperprior, CHARM and the
decoder; the helper's own signs and |x| are kept beside them for analysis_train_ref.tie_report.  LPIPS is left as it is."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import analysis_train_ref as AR
from oracle import dcvic_oracle as O
from oracle import train_oracle as T

SYNTH_PREFIXES = T.TRAINABLE_PREFIXES


class ReluDecisions:
    """The product's ReLU outputs of one step (any order), matched to the helper's relu calls by size and value: a call's relu(x) must
    agree with exactly one unused output within 1e-3 of its max.  Keeps, per matched call, the helper's own sign, the product's, and |x|."""

    def __init__(self, outputs):
        self.by_numel = {}
        for t in outputs:
            self.by_numel.setdefault(t.numel(), []).append(t.detach().reshape(-1).cpu())
        self.unmatched, self.own, self.used, self.margin = [], [], [], []

    def mask_for(self, x):
        r = torch.relu(x.detach()).reshape(-1).float()
        tol = 1e-3 * max(float(r.max()), 1e-30)
        cands = self.by_numel.get(r.numel(), [])
        errs = [float((c - r).abs().max()) for c in cands]
        if not errs or min(errs) > tol:
            self.unmatched.append(tuple(x.shape))
            return None
        c = cands.pop(errs.index(min(errs)))
        m = (c > 0).reshape(x.shape)
        self.own.append((x.detach() > 0).reshape(-1)); self.used.append(m.reshape(-1)); self.margin.append(x.detach().abs().reshape(-1).double())
        return m.to(x.dtype)

    def report(self):
        """(own signs, used signs, |x|) over every matched ReLU input of the step, for analysis_train_ref.tie_report."""
        return torch.cat(self.own).to(torch.int8), torch.cat(self.used).to(torch.int8), torch.cat(self.margin)


@contextlib.contextmanager
def _forced_relu(dec):
    """While active, the oracle's F.relu(x) is x * (the product's sign) for every call `dec` can match (dec None: nothing changes)."""
    real = F.relu

    def relu(x, *a, **k):
        m = dec.mask_for(x)
        return real(x, *a, **k) if m is None else x * m
    if dec is not None:
        F.relu = relu
    try:
        yield
    finally:
        F.relu = real


def apply_loss_weight(loss, weight):
    assert weight.ndim == 1
    if loss.ndim > 1:
        loss = loss.mean(dim=tuple(range(1, loss.ndim)))
    loss = (loss * weight).mean()
    return loss


def calc_vq_rate_loss_weight(policy, offset, beta_vq, beta_rate):
    if policy == "linear":
        return beta_vq + offset, beta_rate + offset
    if policy == "exp":
        return torch.exp(beta_vq), torch.exp(beta_rate)
    raise ValueError()


def _calc_batch_bpp(y_likelihood, z_likelihood, num_pixel):
    bit_y = -torch.log(y_likelihood) / np.log(2)
    bit_z = -torch.log(z_likelihood) / np.log(2)
    bit_y = torch.sum(bit_y, dim=tuple(range(1, bit_y.ndim)))
    bit_z = torch.sum(bit_z, dim=tuple(range(1, bit_z.ndim)))
    return (bit_y + bit_z) / num_pixel


def mse_factor(e):
    """MSELoss (distortion_loss.py:11-39) on [-1, 1] images as a factor on F.mse_loss(a, b)."""
    if e.get("mse_scale", "0_255") == "0_1":
        return 0.25
    return (255.0 / 2.0) ** 2 if e.get("normalize_img", False) else 255.0 ** 2 / 4000.0


def step(sd, I, b1, b2, opt, lsd, force, synth_dtype=torch.float32):
    """sd: the CPU state dict (fp32); I: analysis_train_ref.analysis_inputs; opt: dict(trainer=, loss=) of the YAML; lsd: the LPIPS
    state dict or None.  -> (loss terms {name: fp64 scalar}, values, {parameter name: gradient or None}, decisions)."""
    tr, ls = opt["trainer"], opt["loss"]
    x = I["x"]
    N, _, H, W = x.shape
    vq_weight, rate_weight = calc_vq_rate_loss_weight(tr.get("beta_policy", "linear"), tr.get("beta_offset", 1.0), b2.double(), b1.double())
    # ---- analysis side, fp64 leaves
    L = AR.leaf_state({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items() if k.split(".")[0] in AR.MODULES}, torch.float64)
    relu = force.get("relu")
    with AR._embed_as(torch.float64), _forced_relu(relu):
        y = O.elic_encoder(L, x.double(), I["feat"].double(), b1, b2)
        e = AR.estimate_entropy(L, y, I["noise_y"].double(), I["noise_z"].double(), True, dict(y=force["y"], z=force["z"]))
    R = {}
    rl = ls["rate_loss"]
    assert rl["reduction"] == "none" and tr.get("sample_beta_batch", False)
    R["rate"] = apply_loss_weight(rl["loss_weight"] * _calc_batch_bpp(e["lik_y"], e["lik_z"], H * W), rate_weight)
    # ---- synthesis side, leaves in synth_dtype, on the analysis side's y_hat
    S = {k: (v.to(synth_dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    s_names = [k for k in S if k.startswith(SYNTH_PREFIXES) and S[k].is_floating_point()]
    for k in s_names:
        S[k] = S[k].clone().requires_grad_(True)
    if lsd is not None:
        lsd = {k: v.to(synth_dtype) for k, v in lsd.items()}
    x = x.to(synth_dtype)
    y_hat = e["y_hat"].to(synth_dtype)
    with AR._embed_as(synth_dtype):
        z_q, idx = O.vq_encode(S, x)
        with _forced_relu(relu):
            feat_1, feats = O.elic_decoder_feats(S, y_hat, b1, b2)
    pred_embed, logits = O.swin_estimator(S, feat_1)
    own_idx = torch.argmax(logits, dim=1)
    out_idx = own_idx if force.get("out_idx") is None else force["out_idx"]
    lat = O._conv(S, "vq_model.post_quant_conv", O.vq_indices_to_latent(S, out_idx))
    fake = O.fusion_decode(S, lat, feats, 1.0)
    d, cd, ce = ls["distortion_loss"], ls["code_distortion_loss"], ls["code_ce_loss"]
    R["distortion"] = d["loss_weight"] * mse_factor(d) * F.mse_loss(x, fake)
    if lsd is not None:
        R["perceptual"] = ls["perceptual_loss"]["loss_weight"] * torch.mean(T.lpips_alex(lsd, x, fake))
    assert cd["reduction"] == "none" and ce["reduction"] == "none"
    R["code_distortion"] = apply_loss_weight(cd["loss_weight"] * F.mse_loss(z_q, pred_embed, reduction="none"), vq_weight.to(synth_dtype))
    ce_map = F.cross_entropy(logits, idx, reduction="none")
    pt = F.softmax(logits, dim=1).gather(1, idx.unsqueeze(1)).squeeze(1)
    R["code_ce"] = apply_loss_weight(ce["loss_weight"] * ((1 - pt) ** ce["gamma"]) * ce_map, vq_weight.to(synth_dtype))
    total = sum(v.double() for v in R.values())
    total.backward()
    grads = {k: L[k].grad for k in AR.trainable_names(sd)}
    grads.update({k: S[k].grad for k in s_names})
    q_bits = (e["q_bits_y"] + e["q_bits_z"]).detach()
    vals = dict(y_hat=e["y_hat"].detach(), fake=fake.detach(), total=total.detach(), qbpp=float(q_bits.sum()) / (N * H * W), gt_idx=idx,
                vq_acc=float((out_idx == idx).float().mean()), clamped=AR.clamped_share(e))
    decisions = dict(y=(e["own_symbols"]["y"], e["margin"]["y"]), z=(e["own_symbols"]["z"], e["margin"]["z"]), out_idx=own_idx)
    return {k: v.detach().double() for k, v in R.items()}, vals, grads, decisions
