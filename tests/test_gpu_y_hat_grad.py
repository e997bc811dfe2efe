"""The synthesis side of a stage 1-2 step on a real MI355X: nets.decoder_get_feats on a `Var` y_hat, the estimator, the fusion decoder
and the per-sample weighted code losses (A.mse_loss_weighted, A.focal_cross_entropy_loss_weighted with losses.sample_loss_weights),
against torch autograd over the CPU oracle with the losses in the reference trainer's own words (reduction 'none' maps,
apply_loss_weight; config/exp1_stage1_2.yaml's loss section from tests/golden/reference_loss_sections.json, beta policy exp).

Bounds, those of test_generator_and_discriminator_step_vs_oracle: 2e-4 of max for values and loss terms, 3e-3 of the tensor's max for
every gradient.  The estimator's argmax is a decision: the product's indices are fed to the oracle (force_out_idx) and at most
max(1, 1e-5 x decisions) may differ from the oracle's own."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
VAL_TOL, GRAD_TOL = 2e-4, 3e-3


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def apply_loss_weight(loss, weight):
    """dual_cond_rate_distortion_vq_code_trainer.py:92-98."""
    assert weight.ndim == 1
    if loss.ndim > 1:
        loss = loss.mean(dim=tuple(range(1, loss.ndim)))
    return (loss * weight).mean()


@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


def synthesis_losses(ctx, m, x, y_hat, gt_lat, gt_idx, b1, b2, section, bw):
    """The product's synthesis side and its three losses on the tape -> (terms, Vars, out_idx)."""
    from dc_vic_amd import ops
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import nets
    from dc_vic_amd.train.losses import mse_distortion_factor, sample_loss_weights
    feat_1, feats = nets.decoder_get_feats(ctx, m.decoder, y_hat, b1, b2)
    pred_embed, logits = nets.estimator_forward(ctx, m.vq_estimator, feat_1)
    pq = m.vq_model.post_quant_conv
    out_idx, lat = ops.argmax_lut(logits.data, m.vq_model.quantize.embedding.weight, pq.weight.reshape(pq.out_channels, -1).contiguous(), pq.bias)
    fake = nets.fusion_decode(ctx, m.fusion_module, m.vq_model.decoder, A.const(lat), feats, w=1.0)
    N = x.shape[0]
    d, cd, ce = section["distortion_loss"], section["code_distortion_loss"], section["code_ce_loss"]
    L = {"distortion": A.mse_loss(ctx, fake, x, d["loss_weight"] * mse_distortion_factor(d["normalize_img"], d["mse_scale"]))}
    L["code_distortion"] = A.mse_loss_weighted(ctx, pred_embed, gt_lat, sample_loss_weights(cd["loss_weight"], cd["reduction"], N, gt_lat[0].numel(), bw))
    L["code_ce"] = A.focal_cross_entropy_loss_weighted(ctx, logits, gt_idx, sample_loss_weights(ce["loss_weight"], ce["reduction"], N, gt_idx[0].numel(), bw),
                                                       ce["gamma"])
    return L, dict(fake=fake, pred_embed=pred_embed, logits=logits), out_idx


def test_synthesis_side_gradient_reaches_y_hat(model, synth_sd):
    from dc_vic_amd.train import autograd as A
    from oracle import dcvic_oracle as O
    from oracle import train_oracle as T
    from oracle.entropy_oracle import EntropyBottleneckOracle
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        opt = json.load(f)["exp1_stage1_2.yaml"]
    section = opt["loss"]
    assert opt["trainer"]["beta_policy"] == "exp" and section["code_ce_loss"]["reduction"] == "none" == section["code_distortion_loss"]["reduction"]
    m = model
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(90)) * 2 - 1
    b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
    bw = torch.exp(b2)                                                   # calc_vq_rate_loss_weight, policy exp
    grp = A.ParamGroup([m.decoder, m.vq_estimator, m.fusion_module], DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        gt_lat, gt_idx, feat = m.vq_encode(xd, None, want_feat=True)
        y = m.comp_encode(xd, gt_lat, gt_idx, enc_kwargs=dict(beta_1=b1, beta_2=b2), feat=feat)
        y_hat = m._entropy_encode_side(y, want_symbols=False)["y_hat"]

    # ---- product: y_hat as a Var
    ctx = A.Ctx([grp])
    yv = A.Var(y_hat)
    L, V, out_idx = synthesis_losses(ctx, m, xd, yv, gt_lat, gt_idx, b1, b2, section, bw.to(DEV))
    ctx.backward()
    assert yv.grad is not None and tuple(yv.grad.shape) == tuple(y_hat.shape)
    grad_var = grp.grad.clone()

    # ---- oracle: the same y_hat as a leaf, the same argmax, the losses as the reference trainer writes them
    sd = {k: v.clone() for k, v in synth_sd.items()}
    names = [k for k in sd if k.startswith(T.TRAINABLE_PREFIXES) and sd[k].is_floating_point()]
    for k in names:
        sd[k].requires_grad_(True)
    yh = y_hat.cpu().clone().requires_grad_(True)
    z_q, idx = O.vq_encode(sd, x)
    assert torch.equal(idx, gt_idx.cpu())
    feat_1, feats = O.elic_decoder_feats(sd, yh, b1, b2)
    pred_embed, logits = O.swin_estimator(sd, feat_1)
    own_idx = torch.argmax(logits, dim=1)
    differ = int((own_idx != out_idx.cpu()).sum())
    assert differ <= max(1, int(1e-5 * own_idx.numel())), f"{differ} of {own_idx.numel()} argmax decisions differ"
    lat = O._conv(sd, "vq_model.post_quant_conv", O.vq_indices_to_latent(sd, out_idx.cpu()))
    fake = O.fusion_decode(sd, lat, feats, 1.0)
    pred_embed.retain_grad(), logits.retain_grad()
    ce_map = F.cross_entropy(logits, idx, reduction="none")
    pt = F.softmax(logits, dim=1).gather(1, idx.unsqueeze(1)).squeeze(1)
    focal = section["code_ce_loss"]["loss_weight"] * ((1 - pt) ** section["code_ce_loss"]["gamma"]) * ce_map          # reduction 'none'
    R = {"distortion": section["distortion_loss"]["loss_weight"] * F.mse_loss((x + 1.0) / 2.0, (fake + 1.0) / 2.0),
         "code_distortion": apply_loss_weight(section["code_distortion_loss"]["loss_weight"] * F.mse_loss(z_q, pred_embed, reduction="none"), bw),
         "code_ce": apply_loss_weight(focal, bw)}
    sum(R.values()).backward()

    worst = {}
    for k in R:
        worst[f"loss {k}"] = relerr(L[k], R[k].detach().reshape(1))
        assert worst[f"loss {k}"] <= VAL_TOL, (k, worst)
    worst["fake"] = relerr(V["fake"].data, fake)
    assert worst["fake"] <= VAL_TOL
    for name, got, want in (("d/d y_hat", yv.grad, yh.grad), ("d/d pred_embed", V["pred_embed"].grad, pred_embed.grad), ("d/d logits", V["logits"].grad, logits.grad)):
        worst[name] = relerr(got, want)
        assert worst[name] <= GRAD_TOL, (name, worst[name])
    own = dict(m.named_parameters())
    checked, w_par = 0, 0.0
    for k in names:
        if sd[k].grad is None:
            assert float(grp.grad_of(own[k]).abs().max()) == 0.0, k
            continue
        e = relerr(grp.grad_of(own[k]), sd[k].grad)
        assert e <= GRAD_TOL, (k, e)
        w_par, checked = max(w_par, e), checked + 1
    assert checked == 403, checked        # the synthesis-side tensors test_generator_and_discriminator_step_vs_oracle counts
    print("[synthesis side, Var y_hat] " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f", {checked} parameter gradients worst {w_par:.3e}")

    # ---- a Tensor y_hat behaves as before: the same values and parameter gradients bit for bit, and nothing flows back
    grp.zero_grad()
    ctx2 = A.Ctx([grp])
    L2, V2, out2 = synthesis_losses(ctx2, m, xd, y_hat, gt_lat, gt_idx, b1, b2, section, bw.to(DEV))
    ctx2.backward()
    assert torch.equal(out2, out_idx) and torch.equal(V2["fake"].data, V["fake"].data) and all(torch.equal(L2[k], L[k]) for k in L)
    assert torch.equal(grp.grad, grad_var)
