"""Training-mode (differentiable) forwards of the sub-networks the stage-3 trainer optimises, written against the SAME
parameter-holding modules the inference path uses (dc_vic_amd/{elic,swin,fusion,vqgan}.py), plus the PatchGAN
discriminator.  Reference: hyperprior_dc_vic_model.py:208-274 (forward, is_train=True, fix_entropy_models=True),
elic_dual_beta_ft_autoencoder.py:332-359, swin_vq_estimator.py:70-98, vq_fusion_module.py:78-126 driving ldm
model.py:462-568, dual_beta_taming_nlayer_discriminator.py:16-89 / taming_nlayer_discriminator.py:29-119.
Only decoder, vq_estimator and fusion_module are trainable (dual_cond_gan_distortion_vq_code_trainer.py:47-52); the frozen
VQGAN decoder is differentiated through (data gradients only).

The analysis side (stages 1-1 / 1-2: encoder, hyper-encoder, entropy bottleneck, hyper-decoder, CHARM) follows further down:
elic_dual_beta_ft_autoencoder.py:108-141, minnen20_hyperprior.py:20-55, minnen20_charm_context_model.py:70-119 (is_train=True,
calc_q_likelihood=True) and hyperprior_charm_dc_vic_model.py:24-56.  Nothing there reads a cached pack, a stacked hyper-partial plan,
a cached beta vector or a CDF table: every plan is built from the live weights of the step."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..elic import BetaScaleShiftModule, ChengNLAM, ConvTranspose2d, FourierEncoding, ResidualBottleneckBlocks
from ..layers import Act, ActNorm, BatchNorm2d, Conv2d, Linear
from ..registry import DISCRIMINATOR_REGISTRY
from . import autograd as A
from .autograd import Ctx, Var

Tensor = torch.Tensor


# ------------------------------------------------------------------------------------------- beta conditioning
def cond_vector(ctx: Ctx, owner, beta_1, beta_2, device) -> Var:
    """embed_1 / embed_2 (host, constants) -> mlp -> cond [B, cond_ch, 1, 1]   (elic_dual_beta_ft_autoencoder.py:109-113)."""
    c = torch.cat([owner.embed_1.embed(beta_1), owner.embed_2.embed(beta_2)], dim=1).to(device)
    c = c.reshape(c.shape[0], -1, 1, 1).contiguous().float()
    h = A.conv(ctx, A.const(c), owner.mlp[0], act=ops.ACT_RELU)
    return A.conv(ctx, h, owner.mlp[2])


def beta_vectors(ctx: Ctx, m: BetaScaleShiftModule, cond: Var) -> Tuple[Var, Var]:
    c = A.conv(ctx, cond, m.shared[0], act=ops.ACT_RELU)
    return A.conv(ctx, c, m.scale), A.conv(ctx, c, m.shift)


# ------------------------------------------------------------------------------------------- ELIC blocks
def bottleneck_blocks(ctx: Ctx, m: ResidualBottleneckBlocks, x: Var) -> Var:
    y = x
    for i in range(m.num_blocks):
        b = getattr(m, f"block{i}")
        h = A.conv(ctx, y, b.conv[0], act=ops.ACT_RELU)
        h = A.conv(ctx, h, b.conv[2], act=ops.ACT_RELU)
        y = A.add(ctx, A.conv(ctx, h, b.conv[4]), y)
    return y


def _nlam_res(ctx: Ctx, b, x: Var) -> Var:
    o = A.conv(ctx, x, b.c1, act=ops.ACT_RELU)
    o = A.conv(ctx, o, b.c2, act=ops.ACT_RELU)
    return A.add(ctx, A.conv(ctx, o, b.c3), x)


def nlam(ctx: Ctx, m: ChengNLAM, x: Var) -> Var:
    t, a = x, x
    for i in range(3):
        t = _nlam_res(ctx, m.trunk_block[i], t)
        a = _nlam_res(ctx, m.attention_block[i], a)
    return A.nlam_gate(ctx, x, t, A.conv(ctx, a, m.conv))


def _beta_ft(ctx: Ctx, owner, beta_1, beta_2, device):
    """The beta-FT of `owner` (an ELIC encoder or decoder) as a function (scale/shift module, v) -> v * (1 + s) + t, with the cond
    vector recorded once.  An unconditioned owner (no `beta_ft_list`: ElicVqCatScEncoder, ElicFeatFusionDecoder) gets the identity and
    nothing is recorded: no cond_vector, no beta_vectors, no chan_affine."""
    if not hasattr(owner, "beta_ft_list"):
        if beta_1 is not None or beta_2 is not None:
            raise ValueError(f"{type(owner).__name__} is unconditioned: beta_1 / beta_2 must be None, got {beta_1!r} / {beta_2!r}")
        return None
    cond = cond_vector(ctx, owner, beta_1, beta_2, device)

    def ft(m: BetaScaleShiftModule, v: Var, add_x: bool = False) -> Var:
        s, t = beta_vectors(ctx, m, cond)
        return A.chan_affine(ctx, v, s, t, add_x=add_x)
    return ft


def decoder_get_feats(ctx: Ctx, dec, y_hat, beta_1=None, beta_2=None):
    """ElicDualBetaFtFeatFusionDecoder.get_feats, or the unconditioned ElicFeatFusionDecoder's (betas None), with a tape.  y_hat is a Tensor
    (a constant: the GAN stages run the entropy side under no_grad) or a Var (estimate_entropy_train's quantized_code.y: the gradient that
    arrives on it continues into the analysis side)."""
    x = y_hat if isinstance(y_hat, Var) else A.const(y_hat)
    ft = _beta_ft(ctx, dec, beta_1, beta_2, x.data.device)
    if ft is not None:
        x = ft(dec.init_fuse, x, add_x=True)                              # init_fuse(x, c) + x   (:343)
    feats: Dict[str, Var] = {}
    query = list(dec.fusion_layer_dict.keys())
    feat_1 = None
    for li, name in enumerate(dec.layer_names):
        layer = getattr(dec, name)
        if ft is not None:
            x = ft(dec.beta_ft_list[li], x)
        if isinstance(layer, ResidualBottleneckBlocks):
            x = bottleneck_blocks(ctx, layer, x)
        elif isinstance(layer, ChengNLAM):
            x = nlam(ctx, layer, x)
        else:
            x = A.conv(ctx, x, layer)
        if name == dec.feat_layer:
            feat_1 = x
        if name in query:
            feats[dec.fusion_layer_dict[name]] = x
        if len(feats) == len(query):
            break
    return feat_1, feats


# ------------------------------------------------------------------------------------------- analysis side
def encoder_forward(ctx: Ctx, enc, x: Tensor, feat: Tensor, beta_1=None, beta_2=None) -> Var:
    """ElicDualBetaFtVqScEncoder.forward, or the unconditioned ElicVqCatScEncoder's (betas None), with a tape: the image and the VQ
    feature (latent | one-hot indices) are constants, the beta vectors are per sample ([B] tensors) or shared (scalars); beta-FT follows
    each layer of the conditioned class."""
    beta_ft = _beta_ft(ctx, enc, beta_1, beta_2, x.device)
    ft = (lambda i, v: v) if beta_ft is None else (lambda i, v: beta_ft(enc.beta_ft_list[i], v))
    h = ft(0, A.conv(ctx, A.const(x), enc.conv1))
    h = ft(1, bottleneck_blocks(ctx, enc.block1, h))
    h = ft(2, A.conv(ctx, h, enc.conv2))
    h = ft(3, bottleneck_blocks(ctx, enc.block2, h))
    h = ft(4, nlam(ctx, enc.attn2, h))
    h = ft(5, A.conv(ctx, h, enc.conv3))
    h = A.conv(ctx, [A.const(feat), h], enc.projection, res=h)          # x + conv3x3(cat[feat, x])   (:131-132)
    h = ft(6, bottleneck_blocks(ctx, enc.block3, h))
    h = ft(7, A.conv(ctx, h, enc.conv4))
    return ft(8, nlam(ctx, enc.attn4, h))


def hyper_encoder_forward(ctx: Ctx, he, y: Var) -> Var:
    h = A.conv(ctx, y, he.conv1, act=ops.ACT_RELU)
    h = A.conv(ctx, h, he.conv2, act=ops.ACT_RELU)
    return A.conv(ctx, h, he.conv3)


def hyper_decoder_forward(ctx: Ctx, hd, z_hat: Var) -> Var:
    """Minnen20HyperDecoder.forward: the two branches write the halves of ONE hyper_out."""
    N, _, H, W = z_hat.shape
    half = hd.half
    buf = torch.empty((N, 2 * half, 4 * H, 4 * W), dtype=torch.float32, device=z_hat.data.device)
    outs = []
    for blk, dst in ((hd.hd_mu, buf[:, :half]), (hd.hd_std, buf[:, half:])):
        h = A.conv(ctx, z_hat, blk.conv1, act=ops.ACT_RELU)
        h = A.conv(ctx, h, blk.conv2, act=ops.ACT_RELU)
        outs.append(A.conv(ctx, h, blk.conv3, out=dst))
    return A.join_channels(ctx, buf, outs)


def _slice_transform(ctx: Ctx, st, srcs, act: int = ops.ACT_NONE) -> Var:
    h = A.conv(ctx, srcs, st.model[0], act=ops.ACT_RELU)
    h = A.conv(ctx, h, st.model[2], act=ops.ACT_RELU)
    return A.conv(ctx, h, st.model[4], act=act)


def charm_forward_train(ctx: Ctx, cm, y: Var, hyper_out: Var, entropy_model_y, noise: Tensor, weights: Optional[Tensor], scale: float,
                        bits: Tensor, loss: Tensor, q_bits: Optional[Tensor] = None) -> Dict:
    """Minnen20CharmContextModel.forward(is_train=True, calc_q_likelihood=True) with a tape.  Per slice: mu and sigma from
    [hyper | y_hat[:k]] (multi-source convs on views, no cat), the gaussian_rate tape op on the slice views (STE output, noisy
    likelihood, bits / loss accumulated, rate gradients seeded now), the no-grad quantised likelihood from the eval kernel, the LRP
    with 0.5 tanh on [hyper_mean | support | yq], y_hat_i = yq + lrp into ONE y_hat buffer whose leading channels are the next
    slices' support.  A gradient arriving on the returned y_hat reaches `y` through the STE and earlier slices through the supports.
    -> dict(y_hat: Var, likelihood, q_likelihood, symbols (int32, of the quantised pass))."""
    N, Cy, H, W = y.shape
    dev = y.data.device
    sc, ns, hm = cm.slice_ch, cm.num_slices, cm.hyper_half
    if Cy != sc * ns or tuple(hyper_out.shape) != (N, 2 * hm, H, W) or tuple(noise.shape) != tuple(y.shape):
        raise ValueError(f"charm_forward_train: y {tuple(y.shape)}, hyper_out {tuple(hyper_out.shape)}, noise {tuple(noise.shape)}")
    new = lambda dtype=torch.float32: torch.empty((N, Cy, H, W), dtype=dtype, device=dev)
    y_hat_buf, dy_rate, lik, q_lik, sym = new(), new(), new(), new(), new(torch.int32)
    table = entropy_model_y._table_dev(y.data)
    # split_channels records its gather now, so it runs after every slice's backward (of y last: hyper_out's runs first)
    y_sl = A.split_channels(ctx, y, [sc] * ns)
    h_mean, h_scale = A.split_channels(ctx, hyper_out, [hm, hm])
    yh_sl = []
    for i in range(ns):
        sl = slice(i * sc, (i + 1) * sc)
        k = cm._n_support(i)
        # the support's join is recorded before this slice's three transforms: it hands their gradients on to the earlier slices after them
        support = [A.join_channels(ctx, y_hat_buf[:, :k * sc], yh_sl[:k])] if k > 0 else []
        mu = _slice_transform(ctx, cm.mean_slice_transforms[i], [h_mean] + support)
        sigma = _slice_transform(ctx, cm.scale_slice_transforms[i], [h_scale] + support)
        yq = A.gaussian_rate(ctx, y_sl[i], mu, sigma, noise[:, sl], weights, scale, bits, loss, dy_out=dy_rate[:, sl] if y.needs_grad else None,
                             lik_out=lik[:, sl])
        # the quantised likelihood (no gradient): the eval kernel on the same mu / sigma
        ops.gaussian_rate(y_sl[i].data, None, mu.data, sigma.data, table, None, sym[:, sl], None, q_lik[:, sl], q_bits)
        lrp = _slice_transform(ctx, cm.lrp_slice_transforms[i], [h_mean] + support + [yq], act=ops.ACT_HALF_TANH)
        yh_sl.append(A.add(ctx, yq, lrp, out=y_hat_buf[:, sl]))
    A.acc(y, dy_rate)            # the rate gradient, seeded at forward time; what comes through the STE is added by y's split_channels
    y_hat = A.join_channels(ctx, y_hat_buf, yh_sl)
    return dict(y_hat=y_hat, likelihood=lik, q_likelihood=q_lik, symbols=sym)


def estimate_entropy_train(ctx: Ctx, model, y: Var, noise_y: Tensor, noise_z: Tensor, weights: Optional[Tensor] = None, scale: float = 1.0) -> Dict:
    """HyperpriorCharmDualCondVicModel.estimate_entropy(is_train=True) with a tape: the reference's keys (quantized_code.y / .z are
    Vars: the decoder side continues the tape from them), the per-image bits of the noisy and of the quantised likelihoods, and
    `loss` [1] = sum_n scale * weights[n] * (bits_y[n] + bits_z[n]), whose gradients are already seeded."""
    from ..entropy import pack_entropy_bottleneck
    N = y.shape[0]
    dev = y.data.device
    z = hyper_encoder_forward(ctx, model.hyperencoder, y)
    bits_y, bits_z, q_bits_y, q_bits_z = (torch.zeros(N, dtype=torch.float32, device=dev) for _ in range(4))
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    eb = model.entropy_model_z
    z_lik, z_qlik = torch.empty_like(z.data), torch.empty_like(z.data)
    z_sym = torch.empty(z.shape, dtype=torch.int32, device=dev)
    z_hat = A.eb_rate(ctx, z, eb, noise_z, weights, scale, bits_z, loss, lik_out=z_lik)
    # the quantised likelihood of z (no gradient): the eval kernel on packs made from the LIVE parameters, not eb.packs()
    packs = pack_entropy_bottleneck({f"eb.{k}": v.data for k, v in eb.named_parameters()}, "eb")
    ops.eb_rate(A._dense(z.data), packs, torch.empty_like(z.data), z_sym, z_qlik, q_bits_z)
    hyper_out = hyper_decoder_forward(ctx, model.hyperdecoder, z_hat)
    r = charm_forward_train(ctx, model.context_model, y, hyper_out, model.entropy_model_y, noise_y, weights, scale, bits_y, loss, q_bits=q_bits_y)
    return {"quantized_code": {"y": r["y_hat"], "z": z_hat}, "latent_code": {"y": y, "z": z},
            "likelihoods": {"y": r["likelihood"], "z": z_lik}, "q_likelihoods": {"y": r["q_likelihood"], "z": z_qlik},
            "bits_y": bits_y, "bits_z": bits_z, "q_bits_y": q_bits_y, "q_bits_z": q_bits_z, "loss": loss,
            "symbols": {"y": r["symbols"], "z": z_sym}, "hyper_out": hyper_out}


def analysis_forward(ctx: Ctx, model, x: Tensor, beta_rate=None, beta_vq=None, vq_indices: Optional[Tensor] = None, noise_y: Optional[Tensor] = None,
                     noise_z: Optional[Tensor] = None, generator: Optional[torch.Generator] = None, weights: Optional[Tensor] = None,
                     scale: float = 1.0) -> Dict:
    """The analysis side of one training step on a preprocessed batch x [N, 3, H, W] (sides multiples of 64): the no-grad VQ encode,
    the encoder (beta-conditioned, or unconditioned with both betas None) and estimate_entropy_train.  Without explicit noise, U(-0.5, 0.5) is drawn on the device from
    `generator` (as entropy._train_noise does).  -> estimate_entropy_train's dict plus gt_vq_latent / gt_vq_indices."""
    from ..entropy import _train_noise
    if x.shape[2] % 64 or x.shape[3] % 64:
        raise ValueError(f"analysis_forward: image sides must be multiples of 64, got {tuple(x.shape[2:])}")
    with torch.no_grad():
        zq, idx, feat = model.vq_encode(x, vq_indices, want_feat=True)
    y = encoder_forward(ctx, model.encoder, x, feat, beta_rate, beta_vq)
    N, Cy, H, W = y.shape
    like_z = torch.empty((N, model.hyperencoder.conv3.out_channels, H // 4, W // 4), dtype=torch.float32, device=x.device)
    noise_y = _train_noise(y.data, noise_y, generator)
    noise_z = _train_noise(like_z, noise_z, generator)
    out = estimate_entropy_train(ctx, model, y, noise_y, noise_z, weights, scale)
    out.update(gt_vq_latent=zq, gt_vq_indices=idx)
    return out


# ------------------------------------------------------------------------------------------- Swin estimator
def _femasr_res(ctx: Ctx, rb, x: Var) -> Var:
    h = A.group_norm(ctx, x, rb.conv[0].norm, act=ops.ACT_SWISH)
    h = A.conv(ctx, h, rb.conv[2])
    h = A.group_norm(ctx, h, rb.conv[3].norm, act=ops.ACT_SWISH)
    return A.add(ctx, A.conv(ctx, h, rb.conv[5]), x)


def _swin_block(ctx: Ctx, blk, x: Var) -> Var:
    h = A.layer_norm_c(ctx, x, blk.norm1)
    qkv = A.conv(ctx, h, blk.attn.qkv)
    a = A.swin_attention(ctx, qkv, blk.attn.relative_position_bias_table, blk.num_heads, blk.window_size, blk.shift_size)
    x = A.add(ctx, A.conv(ctx, a, blk.attn.proj), x)
    h = A.layer_norm_c(ctx, x, blk.norm2)
    h = A.activation(ctx, A.conv(ctx, h, blk.mlp.fc1), ops.ACT_GELU)
    return A.add(ctx, A.conv(ctx, h, blk.mlp.fc2), x)


def estimator_forward(ctx: Ctx, est, feat: Var) -> Tuple[Var, Var]:
    """DualBlockSwinVqEstimator.forward -> (pred_embed, logits)."""
    x = A.conv(ctx, feat, est.first_block[0])
    x = _femasr_res(ctx, est.first_block[2], x)
    x = _femasr_res(ctx, est.first_block[3], x)
    x = A.conv(ctx, x, est.first_block[4])
    pred_embed = A.conv(ctx, x, est.embed_projection)
    h, w = x.shape[2:]
    if h % est.window_size or w % est.window_size:
        raise NotImplementedError("training crops are 256x256 (32x32 tokens): the reflect-padded estimator path is inference-only")
    for rstb in est.swin_blks:
        g = x
        for blk in rstb.residual_group.blocks:
            g = _swin_block(ctx, blk, g)
        x = A.add(ctx, A.conv(ctx, g, rstb.conv), x)
    x = _femasr_res(ctx, est.out_block[0], x)
    return pred_embed, A.conv(ctx, x, est.out_block[1])


# ------------------------------------------------------------------------------------------- VQGAN decoder + SFT fusion
def _ldm_resnet(ctx: Ctx, rb, x: Var) -> Var:
    h = A.group_norm(ctx, x, rb.norm1, act=ops.ACT_SWISH)
    h = A.conv(ctx, h, rb.conv1)
    h = A.group_norm(ctx, h, rb.norm2, act=ops.ACT_SWISH)
    h = A.conv(ctx, h, rb.conv2)
    skip = A.conv(ctx, x, rb.nin_shortcut) if rb.in_channels != rb.out_channels else x
    return A.add(ctx, skip, h)


def _ldm_attn(ctx: Ctx, ab, x: Var) -> Var:
    h = A.group_norm(ctx, x, ab.norm)
    qkv = A.cat_channels(ctx, [A.conv(ctx, h, ab.q), A.conv(ctx, h, ab.k), A.conv(ctx, h, ab.v)])
    o = A.attn_single_head(ctx, qkv, ab.in_channels)
    return A.add(ctx, x, A.conv(ctx, o, ab.proj_out))


def _cf_resblock(ctx: Ctx, rb, x_in: Var) -> Var:
    x = A.group_norm(ctx, x_in, rb.norm1, act=ops.ACT_SWISH)
    x = A.conv(ctx, x, rb.conv1)
    x = A.group_norm(ctx, x, rb.norm2, act=ops.ACT_SWISH)
    x = A.conv(ctx, x, rb.conv2)
    skip = A.conv(ctx, x_in, rb.conv_out) if rb.in_channels != rb.out_channels else x_in
    return A.add(ctx, x, skip)


def _fuse_sft(ctx: Ctx, fb, dec: Var, cond: Var, w: float) -> Var:
    f = _cf_resblock(ctx, fb.fuse_block, A.cat_channels(ctx, [cond, dec]))
    sc = A.conv(ctx, A.conv(ctx, f, fb.scale[0], act=ops.ACT_LRELU02), fb.scale[2])
    sh = A.conv(ctx, A.conv(ctx, f, fb.shift[0], act=ops.ACT_LRELU02), fb.shift[2])
    return A.sft(ctx, dec, sc, sh, w)


def fusion_decode(ctx: Ctx, fm, vq_dec, z: Var, cond_feats: Dict[str, Var], w: float = 1.0) -> Var:
    """VqDecFusionModule.forward (vq_fusion_module.py:78-126) with a tape."""
    h = A.conv(ctx, z, vq_dec.conv_in)
    h = _ldm_resnet(ctx, vq_dec.mid.block_1, h)
    h = _ldm_attn(ctx, vq_dec.mid.attn_1, h)
    h = _ldm_resnet(ctx, vq_dec.mid.block_2, h)
    for i_level in reversed(range(vq_dec.num_resolutions)):
        lvl = vq_dec.up[i_level]
        for i_block in range(vq_dec.num_res_blocks + 1):
            h = _ldm_resnet(ctx, lvl.block[i_block], h)
            if len(lvl.attn) > 0:
                h = _ldm_attn(ctx, lvl.attn[i_block], h)
        key = f"block_1_{2 ** i_level}"
        if key in fm.fusion_keys:
            h = _fuse_sft(ctx, fm.fusion_modules[key], h, cond_feats[key], w)
        if i_level != 0:
            h = A.conv(ctx, h, lvl.upsample.conv)
    h = A.group_norm(ctx, h, vq_dec.norm_out, act=ops.ACT_SWISH)
    return A.conv(ctx, h, vq_dec.conv_out)


def synthesis_forward(ctx: Ctx, model, y_hat, beta_rate=None, beta_vq=None, gumbel: Optional[Tuple[Tensor, float]] = None) -> Dict:
    """The synthesis side of a training step, analysis_forward's counterpart (hyperprior_dc_vic_model.py:240-274): decoder features of y_hat
    (Tensor or Var, see decoder_get_feats), the VQ estimator, its logits' argmax through the post_quant_conv LUT, the fusion decoder.  With
    `gumbel` = (noise, tau), the caller's draw, the decoder reads the hard Gumbel-softmax sample's latent (:254-260); out_vq_indices stays the argmax."""
    feat_1, feats = decoder_get_feats(ctx, model.decoder, y_hat, beta_rate, beta_vq)
    pred_embed, logits = estimator_forward(ctx, model.vq_estimator, feat_1)
    pq = model.vq_model.post_quant_conv
    codebook, pq_w = model.vq_model.quantize.embedding.weight, pq.weight.reshape(pq.out_channels, -1).contiguous()
    out_idx, lat = ops.argmax_lut(logits.data, codebook, pq_w, pq.bias)
    z = A.const(lat)
    if gumbel is not None:
        _, z = A.gumbel_vq_latent(ctx, logits, gumbel[0], codebook, pq_w, pq.bias, gumbel[1])
    fake = fusion_decode(ctx, model.fusion_module, model.vq_model.decoder, z, feats, w=1.0)
    return dict(fake=fake, pred_embed=pred_embed, logits=logits, out_vq_indices=out_idx)


# ------------------------------------------------------------------------------------------- discriminator
@DISCRIMINATOR_REGISTRY.register()
class DualBetaCondTamingNLayerDiscriminator(nn.Module):
    """PatchGAN conditioned on (beta_rate, beta_vq): state-dict keys `main.{0,2,5,8,11}.{weight,bias}` (n_layers 3),
    `mlp.{0,2}.{weight,bias}` as in the reference.  norm_type 'none' -> Identity layers keep their Sequential indices, biases on;
    'batchnorm' -> `main.{3,6,9}.{weight,bias,running_mean,running_var,num_batches_tracked}` and no bias on the convolutions in front
    of them; 'actnorm' (or use_actnorm) -> `main.{3,6,9}.{loc,scale,initialized}`.  The Python default stays 'none' (the
    reference's class default is 'batchnorm'; every shipped YAML names its norm_type)."""

    def __init__(self, input_nc: int = 11, ndf: int = 64, out_nc: int = 1, n_layers: int = 3, keep_shape: bool = False,
                 use_actnorm: bool = False, norm_type: str = "none", norm_kwargs: dict = {}, max_beta_1: float = -1.0,
                 max_beta_2: float = -1.0, L: int = 10, cond_ch: int = 8, use_pi: bool = False, include_x: bool = True,
                 y_hat_cond: bool = False, y_hat_in_ch=None, y_hat_out_ch=None, weight_init: bool = True, **kwargs):
        super().__init__()
        self.norm_type, self.norm_kwargs = resolve_norm(norm_type, use_actnorm, norm_kwargs)
        refuse_y_hat_cond(y_hat_cond)
        if int(n_layers) < 1:
            raise ValueError(f"n_layers: {n_layers!r}, needs at least 1")
        kw = 4
        use_bias = self.norm_type != "batchnorm"        # the reference: no conv bias in front of a BatchNorm's own shift
        seq = [Conv2d(input_nc, ndf, kw, 2, 1), Act()]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [Conv2d(ndf * prev, ndf * mult, kw, 2, 1, bias=use_bias), make_norm(ndf * mult, self.norm_type, self.norm_kwargs), Act()]
        kl = 3 if keep_shape else kw
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [Conv2d(ndf * prev, ndf * mult, kl, 1, 1, bias=use_bias), make_norm(ndf * mult, self.norm_type, self.norm_kwargs), Act()]
        seq += [Conv2d(ndf * mult, out_nc, kl, 1, 1)]
        self.main = nn.Sequential(*seq)
        self.n_layers = int(n_layers)
        self.embed_1 = FourierEncoding(L=L, max_beta=max_beta_1, use_pi=use_pi, include_x=include_x)
        self.embed_2 = FourierEncoding(L=L, max_beta=max_beta_2, use_pi=use_pi, include_x=include_x)
        mlp_in = 2 * (2 * L + 1) if include_x else 2 * 2 * L
        self.mlp = nn.Sequential(Linear(mlp_in, cond_ch), Act(), Linear(cond_ch, cond_ch))
        self.cond_ch = cond_ch
        self.y_hat_cond = False
        if weight_init:
            weights_init(self.main)


NORM_TYPES = ("none", "batchnorm", "actnorm")
_NORMS_NOT_BUILT = ("instancenorm", "groupnorm", "layernorm")


def resolve_norm(norm_type: str, use_actnorm: bool = False, norm_kwargs: Optional[dict] = None) -> Tuple[str, Dict[str, float]]:
    """(norm type, BatchNorm2d's keywords) of a discriminator's options, as get_norm_layer reads them
    (taming_nlayer_discriminator.py:11-26,53-59): `use_actnorm: true` means actnorm; `norm_kwargs` may hold `eps` and `momentum` as
    numbers for batchnorm and nothing else.  Every other norm type, key or value is refused with the setting and its value."""
    if use_actnorm:
        norm_type = "actnorm"
    if norm_type in _NORMS_NOT_BUILT:
        raise NotImplementedError(f"norm_type: {norm_type} is not built (none, batchnorm and actnorm are)")
    if norm_type not in NORM_TYPES:
        raise NotImplementedError(f"norm_type: {norm_type!r} is unknown, expected one of {', '.join(NORM_TYPES)}")
    out = {}
    for k, v in dict(norm_kwargs or {}).items():
        if norm_type != "batchnorm" or k not in ("eps", "momentum") or isinstance(v, bool) or not isinstance(v, (int, float)):
            raise NotImplementedError(f"norm_kwargs.{k}: {v!r} is not built with norm_type {norm_type} (batchnorm takes eps and momentum as "
                                      "numbers; affine: false, track_running_stats: false and the cumulative average of momentum: null are not built)")
        out[k] = float(v)
    if "eps" in out and not (out["eps"] > 0.0 and math.isfinite(out["eps"])):
        raise ValueError(f"norm_kwargs.eps: {out['eps']!r}, needs a finite positive number")
    if "momentum" in out and not 0.0 <= out["momentum"] <= 1.0:
        raise ValueError(f"norm_kwargs.momentum: {out['momentum']!r}, needs a number in [0, 1]")
    return norm_type, out


def refuse_y_hat_cond(y_hat_cond) -> None:
    if y_hat_cond:
        raise NotImplementedError("y_hat_cond: true is not built (the reflect-padded y_hat embedding as a further discriminator input)")


def check_unet_options(n_layers: int, num_upsample: int, cond_ch: int, input_nc: int) -> None:
    """What the U-Net discriminator's constructor refuses, as a function of its own for the builder (pure)."""
    if not 1 <= num_upsample <= n_layers - 1:
        raise ValueError(f"num_upsample: {num_upsample} with n_layers: {n_layers}, needs 1 <= num_upsample <= n_layers - 1 (every up block adds "
                         "the body's output of its resolution)")
    if cond_ch != 3:
        raise NotImplementedError(f"cond_ch: {cond_ch} is not built: the reference expands the beta embedding with expand_as(x), which runs only "
                                  "when cond_ch equals the image's 3 channels")
    if input_nc != 3 + cond_ch:
        raise ValueError(f"input_nc: {input_nc}, needs 3 + cond_ch = {3 + cond_ch} (the image and the expanded beta embedding)")


def make_norm(channels: int, norm_type: str, norm_kwargs: Dict[str, float]) -> nn.Module:
    if norm_type == "batchnorm":
        return BatchNorm2d(channels, **norm_kwargs)
    return ActNorm(channels) if norm_type == "actnorm" else nn.Identity()


def weights_init(root: nn.Module) -> None:
    """taming's weights_init applied over `root` in module order: conv weights ~ N(0, 0.02), BatchNorm weight ~ N(1, 0.02), bias 0."""
    for m in root.modules():
        if isinstance(m, Conv2d):
            nn.init.normal_(m.weight, 0.0, 0.02)
        elif isinstance(m, BatchNorm2d):
            nn.init.normal_(m.weight, 1.0, 0.02)
            nn.init.constant_(m.bias, 0.0)


class BetaEmbedding(nn.Module):
    """oasis_discriminator.py:15-45: the two Fourier encodings and the MLP, under the U-Net's `beta_emb`."""

    def __init__(self, max_beta_1: float, max_beta_2: float, L: int, cond_ch: int, use_pi: bool, include_x: bool):
        super().__init__()
        self.embed_1 = FourierEncoding(L=L, max_beta=max_beta_1, use_pi=use_pi, include_x=include_x)
        self.embed_2 = FourierEncoding(L=L, max_beta=max_beta_2, use_pi=use_pi, include_x=include_x)
        mlp_in = 2 * (2 * L + 1) if include_x else 2 * 2 * L
        self.mlp = nn.Sequential(Linear(mlp_in, cond_ch), Act(), Linear(cond_ch, cond_ch))


@DISCRIMINATOR_REGISTRY.register()
class OasisDualBetaCondTamingNLayerDiscriminator(nn.Module):
    """The OASIS U-Net discriminator (oasis_discriminator.py:67-203) with the reference's state-dict keys: `body.{i}.0` convolutions
    (k4, s2; `body.{i}.1` their norm from i = 1), `bottleneck.{0,1}` (k3), `up_blocks.{i}.{1,2}` (nearest x2, k3 with bias, norm, then
    + the body's output of that resolution), `head.{0,2}` (k1) and `beta_emb.mlp.{0,2}`.  The logits lie on a grid of
    2^(n_layers - num_upsample) pixels.  One quirk is restated literally: the reference expands the beta embedding with
    `expand_as(x)`, so it runs only when cond_ch equals the image's 3 channels, and input_nc must be 3 + cond_ch."""

    def __init__(self, input_nc: int = 3, ndf: int = 64, n_layers: int = 3, num_upsample: int = 1, out_nc: int = 128, use_actnorm: bool = False,
                 norm_type: str = "none", norm_kwargs: dict = {}, y_hat_cond: bool = False, y_hat_in_ch=None, y_hat_out_ch=None,
                 max_beta_1: float = -1.0, max_beta_2: float = -1.0, L: int = 10, cond_ch: int = 8, use_pi: bool = False, include_x: bool = True,
                 weight_init: bool = True, **kwargs):
        super().__init__()
        self.norm_type, self.norm_kwargs = resolve_norm(norm_type, use_actnorm, norm_kwargs)
        refuse_y_hat_cond(y_hat_cond)
        n_layers, num_upsample = int(n_layers), int(num_upsample)
        check_unet_options(n_layers, num_upsample, int(cond_ch), int(input_nc))
        use_bias = self.norm_type != "batchnorm"
        norm = lambda ch: make_norm(ch, self.norm_type, self.norm_kwargs)
        channels = [ndf * min(2 ** i, 8) for i in range(n_layers)]
        self.body = nn.ModuleList([nn.Sequential(Conv2d(input_nc, channels[0], 4, 2, 1), Act())])
        for n in range(1, n_layers):
            self.body.append(nn.Sequential(Conv2d(channels[n - 1], channels[n], 4, 2, 1, bias=use_bias), norm(channels[n]), Act()))
        self.bottleneck = nn.Sequential(Conv2d(channels[-1], channels[-1], 3, 1, 1, bias=use_bias), norm(channels[-1]), Act())
        self.up_blocks = nn.ModuleList()
        for i in range(num_upsample):
            c_in, c_out = channels[n_layers - 1 - i], channels[n_layers - 2 - i]
            self.up_blocks.append(nn.Sequential(Act(), Conv2d(c_in, c_out, 3, 1, 1), norm(c_out), Act()))       # index 0: the nearest x2
        self.head = nn.Sequential(Conv2d(channels[n_layers - 1 - num_upsample], 64, 1, 1, 0), Act(), Conv2d(64, out_nc, 1, 1, 0))
        self.beta_emb = BetaEmbedding(max_beta_1, max_beta_2, L, cond_ch, use_pi, include_x)
        self.n_layers, self.num_upsample, self.cond_ch = n_layers, num_upsample, int(cond_ch)
        self.y_hat_cond = False
        if weight_init:
            weights_init(self)

    @property
    def logit_stride(self) -> int:
        return 2 ** (self.n_layers - self.num_upsample)


def _conv_norm_lrelu(ctx: Ctx, h: Var, conv: Conv2d, norm: nn.Module) -> Var:
    """conv -> norm -> LeakyReLU(0.2): the activation is fused into the norm's apply pass, or into the conv where there is no norm."""
    if isinstance(norm, BatchNorm2d):
        return A.batch_norm(ctx, A.conv(ctx, h, conv), norm, act=ops.ACT_LRELU02)
    if isinstance(norm, ActNorm):
        return A.act_norm(ctx, A.conv(ctx, h, conv), norm, act=ops.ACT_LRELU02)
    return A.conv(ctx, h, conv, act=ops.ACT_LRELU02)


def _beta_map(ctx: Ctx, owner, cond_ch: int, x: Var, beta_1, beta_2) -> Var:
    """The beta embedding [B, cond_ch, 1, 1] broadcast over x's batch and pixels, differentiable."""
    N, _, H, W = x.shape
    dev = x.data.device
    cond = cond_vector(ctx, owner, beta_1, beta_2, dev)                   # [B, cond_ch, 1, 1]
    zeros = torch.zeros((N, cond_ch, H, W), dtype=torch.float32, device=dev)
    zvec = torch.zeros((cond.shape[0], cond_ch, 1, 1), dtype=torch.float32, device=dev)
    return A.chan_affine(ctx, A.const(zeros), A.const(zvec), cond)        # 0 * (1 + 0) + cond[n][c]


def _unet_forward(ctx: Ctx, D: OasisDualBetaCondTamingNLayerDiscriminator, x: Var, beta_1, beta_2) -> Var:
    if x.shape[1] != D.cond_ch:
        raise ValueError(f"OASIS U-Net discriminator: images of {x.shape[1]} channels, the beta embedding expands to cond_ch = {D.cond_ch}")
    h = A.cat_channels(ctx, [x, _beta_map(ctx, D.beta_emb, D.cond_ch, x, beta_1, beta_2)])
    shortcuts = []
    for i, blk in enumerate(D.body):
        h = A.conv(ctx, h, blk[0], act=ops.ACT_LRELU02) if i == 0 else _conv_norm_lrelu(ctx, h, blk[0], blk[1])
        shortcuts.append(h)
    h = _conv_norm_lrelu(ctx, h, D.bottleneck[0], D.bottleneck[1])
    for i, blk in enumerate(D.up_blocks):
        h = _conv_norm_lrelu(ctx, A.upsample2(ctx, h), blk[1], blk[2])
        h = A.add(ctx, h, shortcuts[-i - 2])
    h = A.conv(ctx, h, D.head[0], act=ops.ACT_LRELU02)
    return A.conv(ctx, h, D.head[2])


def discriminator_forward(ctx: Ctx, D: nn.Module, x: Var, beta_1, beta_2) -> Var:
    """D(x, beta_1, beta_2) on the tape, for either discriminator class.  A normalised one runs in train mode: every call takes its own
    batch statistics and updates the running ones."""
    if isinstance(D, OasisDualBetaCondTamingNLayerDiscriminator):
        return _unet_forward(ctx, D, x, beta_1, beta_2)
    h = A.cat_channels(ctx, [x, _beta_map(ctx, D, D.cond_ch, x, beta_1, beta_2)])
    h = A.conv(ctx, h, D.main[0], act=ops.ACT_LRELU02)
    for i in range(2, len(D.main) - 1, 3):
        h = _conv_norm_lrelu(ctx, h, D.main[i], D.main[i + 1])
    return A.conv(ctx, h, D.main[-1])
