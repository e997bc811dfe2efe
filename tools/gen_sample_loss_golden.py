#!/usr/bin/env python3
"""tests/golden/sample_loss.npz -- the reference's OWN `FocalCrossEntropyLoss` (src/losses/cross_entropy_loss.py:32-53) and
`VanillaMSELoss` (src/losses/distortion_loss.py:43-51) on seeded inputs, carried through the per-sample beta weighting of
DualBetaCondRateDistortionVqCodeTrainer (build container only: needs the reference tree; runs on the CPU, fp32 as the reference
trains).  Same recipe as tools/gen_focal_golden.py:

  * `logits` [3, 64, 4, 4] = randn * 2 (seed 191), `target` [3, 4, 4] int64 (seed 192) with both ends of the codebook;
    `latent` and `gt_latent` [3, 4, 4, 4] = randn (seeds 193, 194); `beta_vq` = [3.0, 0.0, 1.5];
  * for policy in {linear (offset 1), exp} and reduction in {none, mean, sum}:
      vq_weight = beta_vq + offset or exp(beta_vq)                       (calc_vq_rate_loss_weight, trainer source :71-78)
      apply_loss_weight(FocalCrossEntropyLoss(0.05, gamma 2, reduction)(logits, target), vq_weight)  as `ce_<policy>_<reduction>`,
      its autograd gradient d / d logits as `ce_grad_<policy>_<reduction>`, and the same for
      apply_loss_weight(VanillaMSELoss(1.0, reduction)(gt_latent, latent), vq_weight) as `mse_...` / `mse_grad_...` (d / d latent).
    `apply_loss_weight` (:92-98) is restated below word for word: the trainer module imports wandb and compressai at its head and
    cannot be loaded here.
  * `ce_weight`, `gamma`, `mse_weight`, `beta_offset`, `policies`, `reductions` name what was run.

    python tools/gen_sample_loss_golden.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sample_loss.npz")
CE_WEIGHT, GAMMA, MSE_WEIGHT, BETA_OFFSET = 0.05, 2.0, 1.0, 1.0
POLICIES = ("linear", "exp")
REDUCTIONS = ("none", "mean", "sum")
BETA_VQ = (3.0, 0.0, 1.5)


def apply_loss_weight(loss, weight):
    assert weight.ndim == 1
    if loss.ndim > 1:
        loss = loss.mean(dim=tuple(range(1, loss.ndim)))
    loss = (loss * weight).mean()
    return loss


def vq_weight(policy, beta_vq):
    return beta_vq + BETA_OFFSET if policy == "linear" else torch.exp(beta_vq)


def main():
    torch.set_num_threads(8)
    ref_loader.install_training_names()
    with contextlib.redirect_stdout(io.StringIO()):
        cl = ref_loader.ref("src.losses.cross_entropy_loss")
        dl = ref_loader.ref("src.losses.distortion_loss")
    gen = lambda seed: torch.Generator().manual_seed(seed)
    logits = torch.randn((3, 64, 4, 4), generator=gen(191)) * 2
    target = torch.randint(0, 64, (3, 4, 4), generator=gen(192))
    target[0, 0, 0], target[2, 3, 3] = 0, 63               # both ends of the codebook
    latent, gt_latent = torch.randn((3, 4, 4, 4), generator=gen(193)), torch.randn((3, 4, 4, 4), generator=gen(194))
    beta_vq = torch.tensor(BETA_VQ, dtype=torch.float32)
    G = {"logits": logits.numpy(), "target": target.numpy(), "latent": latent.numpy(), "gt_latent": gt_latent.numpy(), "beta_vq": beta_vq.numpy(),
         "ce_weight": np.float64(CE_WEIGHT), "gamma": np.float64(GAMMA), "mse_weight": np.float64(MSE_WEIGHT), "beta_offset": np.float64(BETA_OFFSET),
         "policies": np.asarray(POLICIES), "reductions": np.asarray(REDUCTIONS)}
    for policy in POLICIES:
        w = vq_weight(policy, beta_vq)
        for red in REDUCTIONS:
            lg = logits.clone().requires_grad_(True)
            val = apply_loss_weight(cl.FocalCrossEntropyLoss(loss_weight=CE_WEIGHT, gamma=GAMMA, reduction=red)(lg, target), w)
            val.backward()
            G[f"ce_{policy}_{red}"], G[f"ce_grad_{policy}_{red}"] = val.detach().numpy(), lg.grad.numpy()
            lt = latent.clone().requires_grad_(True)
            val = apply_loss_weight(dl.VanillaMSELoss(loss_weight=MSE_WEIGHT, reduction=red)(gt_latent, lt), w)
            val.backward()
            G[f"mse_{policy}_{red}"], G[f"mse_grad_{policy}_{red}"] = val.detach().numpy(), lt.grad.numpy()
    np.savez_compressed(OUT, **G)
    print("sample_loss.npz:", {k: (v.shape if hasattr(v, "shape") and v.shape else v) for k, v in G.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
