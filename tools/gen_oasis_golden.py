#!/usr/bin/env python3
"""tests/golden/oasis.npz -- the OASIS stage-3 pieces the reference lets us import, from its OWN classes (build container only:
needs the reference tree; runs on the CPU).  Same recipe as oracle/gen_golden.py:gen_train for train.npz:

  * `DualBetaCondTamingNLayerDiscriminator(**config/dc_vic_oasis.yaml's discriminator kwargs)` (out_nc 257, keep_shape) with
    dc_vic_amd.synth.synth_discriminator_state(shapes, seed 5) loaded strict=True -- the fixture stores the key -> shape manifest
    and the seed, not the 12 MB of weights;
  * `OasisGANLoss(loss_weight)` (src/losses/oasis_gan_loss.py).  No reference YAML carries its weight; the fixture uses 0.01 (the
    trainer's default gan weight) and stores it as `gan_loss_weight`;
  * stored: images, betas, VQ indices [2, 8, 8], D(fake) / D(real) logits for per-sample betas, D(real) for scalar betas, the
    generator adv loss, 0.5 x the D-real and D-fake losses (calc_d_loss), d(adv)/d(fake image), d(loss)/d(logits) of the two D-side
    terms (is_real True on D(real), False on D(fake), each x 0.5) and the two out_d_* log values (mean over channels 1:, accumulated
    in fp64 and rounded to fp32; `out_d_*_fp32` is the plain fp32 torch.mean of the same logits).

    python tools/gen_oasis_golden.py
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from oracle.gen_golden import img  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "oasis.npz")
GAN_WEIGHT = 0.01


def main():
    torch.set_num_threads(8)
    ref_loader.install_training_names()
    from dc_vic_amd.synth import synth_discriminator_state
    top = yaml.safe_load(open(os.path.join(ref_loader.REF, "config/dc_vic_oasis.yaml")))
    with contextlib.redirect_stdout(io.StringIO()):
        dm = ref_loader.ref("src.models.discriminator.dual_beta_taming_nlayer_discriminator")
        ol = ref_loader.ref("src.losses.oasis_gan_loss")
    dcfg = dict(top["discriminator"]); assert dcfg.pop("type") == "DualBetaCondTamingNLayerDiscriminator"
    D = dm.DualBetaCondTamingNLayerDiscriminator(**dcfg).eval()
    shapes = {k: tuple(v.shape) for k, v in D.state_dict().items()}
    D.load_state_dict(synth_discriminator_state(shapes, 5), strict=True)
    gan = ol.OasisGANLoss(loss_weight=GAN_WEIGHT)
    G = {"d_manifest": json.dumps({k: list(v) for k, v in shapes.items()}, sort_keys=True), "d_seed": np.int64(5),
         "d_kwargs": json.dumps(dcfg, sort_keys=True), "gan_loss_weight": np.float64(GAN_WEIGHT)}
    real, fake = img((2, 3, 64, 64), 171), img((2, 3, 64, 64), 172)
    b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
    idx = torch.randint(0, 256, (2, 8, 8), generator=torch.Generator().manual_seed(173))
    idx[0, 0, 0], idx[1, 7, 7] = 0, 255                    # both ends of the codebook
    G["real"], G["fake"], G["beta_1"], G["beta_2"], G["vq_indices"] = real.numpy(), fake.numpy(), b1.numpy(), b2.numpy(), idx.numpy()
    # generator side: adv = gan_loss(D(fake), gt_vq_indices, is_real=True, is_disc=False), gradient back to the image
    fk = fake.clone().requires_grad_(True)
    g_fake = D(fk, beta_1=b1, beta_2=b2, y_hat=None)
    assert tuple(g_fake.shape) == (2, 257, 8, 8)
    adv = gan(g_fake, idx, is_real=True, is_disc=False)
    adv.backward()
    G["d_fake_logits"], G["adv_loss"], G["adv_grad_fake"] = g_fake.detach().numpy(), adv.detach().numpy(), fk.grad.numpy()
    # discriminator side (calc_d_loss): 0.5 * CE(D(real), idx + 1) + 0.5 * CE(D(fake.detach()), 0), and the logged scores
    d_real = D(real, beta_1=b1, beta_2=b2, y_hat=None).detach().requires_grad_(True)
    d_fake = g_fake.detach().clone().requires_grad_(True)
    l_real = gan(d_real, idx, is_real=True, is_disc=True) * 0.5
    l_fake = gan(d_fake, idx, is_real=False, is_disc=True) * 0.5
    (l_real + l_fake).backward()
    G["d_real_logits"], G["d_loss_real"], G["d_loss_fake"] = d_real.detach().numpy(), l_real.detach().numpy(), l_fake.detach().numpy()
    G["d_loss_real_grad_logits"], G["d_loss_fake_grad_logits"] = d_real.grad.numpy(), d_fake.grad.numpy()
    # calc_avg_d_score_for_log: torch.mean(d[:, 1:, :, :].detach()).  The trainer module cannot be imported (wandb, compressai), so the
    # expression is restated here.  These logits nearly cancel (mean ~1e-3 of values near 1), and an fp32 sum of them is a few 1e-6
    # of the MEAN away from its exact value, depending on the summation order.  The fixture pins the expression's value, not one
    # summation order: it is accumulated in fp64 and rounded to fp32 once; the fp32 torch.mean is kept beside it as *_fp32.
    for key, d in (("out_d_real", d_real), ("out_d_fake", d_fake)):
        G[key] = torch.mean(d.detach().double()[:, 1:, :, :]).float().numpy()
        G[key + "_fp32"] = torch.mean(d[:, 1:, :, :].detach()).numpy()
    with torch.no_grad():
        G["d_real_logits_scalar_beta"] = D(real, beta_1=1.51, beta_2=2.25, y_hat=None).numpy()
    np.savez_compressed(OUT, **G)
    print("oasis.npz:", {k: (v.shape if hasattr(v, "shape") else v) for k, v in G.items() if not isinstance(v, str)}, os.path.getsize(OUT), "bytes",
          "max |logit|", float(np.abs(G["d_fake_logits"]).max()))


if __name__ == "__main__":
    main()
