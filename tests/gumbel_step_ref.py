"""The generator side of one GAN training step with model.gumbel_sampling, as torch autograd over the CPU oracle: what
oracle/train_oracle.py `generator_losses` states for the argmax path, with the decoder's latent taken from tests/gumbel_ref.py's
restatement of F.gumbel_softmax(logits, tau, hard=True, dim=1) for a given draw (hyperprior_dc_vic_model.py:254-260).  The image
losses then reach the estimator through the straight-through softmax; `out_idx` (vq_acc) stays the argmax of the logits."""
import torch
import torch.nn.functional as F

import gumbel_ref as R
from oracle import dcvic_oracle as O
from oracle import train_oracle as T


def generator_losses(sd, dsd, x, b1, b2, eb, e, tau=1.0, w=T.LOSS_W, lsd=None, force_y_hat=None, force_sample_idx=None):
    """-> (losses, dict(fake, logits, pred_embed, out_idx, sample_idx, own_sample_idx, sample_gap, gt_idx, y_hat, z_q)).
    `e`: the Exp(1) draw [N, n_embed, H / 8, W / 8].  `force_y_hat` / `force_sample_idx`: evaluate on given decisions (the rounded
    symbols, the sampled index) instead of this evaluation's own; `own_sample_idx` and `sample_gap` (the top-2 distance of
    logits - log e per position) say where and how closely the two differ."""
    z_q, idx, y_hat, _, _ = T.encode_side(sd, x, b1, b2, eb)
    if force_y_hat is not None:
        y_hat = force_y_hat
    feat_1, feats = O.elic_decoder_feats(sd, y_hat, b1, b2)
    pred_embed, logits = O.swin_estimator(sd, feat_1)
    own_idx, ret = R.restate_ret(logits, e, tau)
    sample_idx = own_idx
    if force_sample_idx is not None and not torch.equal(force_sample_idx, own_idx):
        sample_idx = force_sample_idx
        s = ((logits - e.log()) / tau).softmax(1)
        ret = torch.zeros_like(logits).scatter_(1, sample_idx.unsqueeze(1), 1.0) - s.detach() + s
    zq_s = torch.einsum("nchw,cd->ndhw", ret, sd["vq_model.quantize.embedding.weight"].detach())
    lat = O._conv(sd, "vq_model.post_quant_conv", zq_s)
    fake = O.fusion_decode(sd, lat, feats, 1.0)
    L = {}
    L["distortion"] = w["distortion"] * F.mse_loss((x + 1.0) / 2.0, (fake + 1.0) / 2.0)
    if lsd is not None:
        L["perceptual"] = w["perceptual"] * torch.mean(T.lpips_alex(lsd, x, fake))
    g_fake = T.discriminator(dsd, fake, b1, b2)
    L["adv"] = w["gan"] * F.binary_cross_entropy_with_logits(g_fake, torch.ones_like(g_fake))
    L["code_distortion"] = w["code_distortion"] * F.mse_loss(z_q, pred_embed)
    L["code_ce"] = w["code_ce"] * F.cross_entropy(logits, idx)
    return L, dict(fake=fake, logits=logits, pred_embed=pred_embed, out_idx=torch.argmax(logits.detach(), dim=1), sample_idx=sample_idx,
                   own_sample_idx=own_idx, sample_gap=R.top2_gap(logits.detach(), e, 1.0), gt_idx=idx, y_hat=y_hat, z_q=z_q)
