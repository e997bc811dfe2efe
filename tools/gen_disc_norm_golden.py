#!/usr/bin/env python3
"""tests/golden/disc_norm.npz -- the normalised GAN discriminators in TRAIN mode, from the reference's OWN classes (build container
only: needs the reference tree; runs on the CPU in fp32).  Same recipe as tools/gen_oasis_golden.py.  Three cases:

  patchgan_bn   DualBetaCondTamingNLayerDiscriminator(**config/exp1_stage1_3.yaml's kwargs, norm_type batchnorm)
  patchgan_an   the same with norm_type actnorm
  unet_bn       OasisDualBetaCondTamingNLayerDiscriminator(input_nc 6, n_layers 4, num_upsample 1, out_nc 257, cond_ch 3, batchnorm)

Per case `<case>.` + :
  kwargs, type, manifest (key -> shape, JSON), seed       dc_vic_amd.synth.synth_norm_discriminator_state(manifest, seed) is the state
                                                          that was loaded strict=True (positive running_var, integer counters)
  logits1, logits2                                        two successive train-mode calls on x with the per-sample betas
  buf1/<key>, buf2/<key>                                  every norm buffer after each call
  cot                                                     the seeded cotangent on logits1
  grad_x, grad/<parameter key>                            d <cot, logits1> / d x, every norm parameter and the first convolution's weight
and once: x [2, 3, 64, 64], beta_1, beta_2.  It also writes tests/golden/reference_discriminator_sections.json: the `discriminator`
section of every reference YAML that has one (settings only).

    python tools/gen_disc_norm_golden.py
"""
from __future__ import annotations

import contextlib
import glob
import io
import json
import os
import sys
import warnings

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from oracle.gen_golden import img  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "disc_norm.npz")
SECTIONS = os.path.join(ROOT, "tests", "golden", "reference_discriminator_sections.json")
BUFFER_LEAVES = ("running_mean", "running_var", "num_batches_tracked", "initialized")
PATCHGAN, UNET = "DualBetaCondTamingNLayerDiscriminator", "OasisDualBetaCondTamingNLayerDiscriminator"


def buffers(D):
    return {k: v.detach().clone().numpy() for k, v in D.state_dict().items() if k.rsplit(".", 1)[-1] in BUFFER_LEAVES}


def main():
    torch.set_num_threads(8)
    ref_loader.install_training_names()
    from dc_vic_amd.synth import synth_norm_discriminator_state
    with contextlib.redirect_stdout(io.StringIO()):
        pm = ref_loader.ref("src.models.discriminator.dual_beta_taming_nlayer_discriminator")
        um = ref_loader.ref("src.models.discriminator.oasis_discriminator")
    sections = {}
    for path in sorted(glob.glob(os.path.join(ref_loader.REF, "config", "*.yaml"))):
        top = yaml.safe_load(open(path))
        if isinstance(top, dict) and isinstance(top.get("discriminator"), dict):
            sections[os.path.basename(path)] = top["discriminator"]
    with open(SECTIONS, "w") as f:
        json.dump(sections, f, indent=1, sort_keys=True)
        f.write("\n")
    base = dict(sections["exp1_stage1_3.yaml"])
    assert base.pop("type") == PATCHGAN
    unet_kw = dict(input_nc=6, ndf=64, n_layers=4, num_upsample=1, out_nc=257, norm_type="batchnorm", max_beta_1=3.0, max_beta_2=3.5, L=10,
                   cond_ch=3, use_pi=False, include_x=True, weight_init=True)
    cases = (("patchgan_bn", PATCHGAN, pm.DualBetaCondTamingNLayerDiscriminator, dict(base, norm_type="batchnorm"), 11),
             ("patchgan_an", PATCHGAN, pm.DualBetaCondTamingNLayerDiscriminator, dict(base, norm_type="actnorm"), 12),
             ("unet_bn", UNET, um.OasisDualBetaCondTamingNLayerDiscriminator, unet_kw, 13))
    x = img((2, 3, 64, 64), 181)
    b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
    G = {"x": x.numpy(), "beta_1": b1.numpy(), "beta_2": b2.numpy()}
    for case, d_type, cls, kw, seed in cases:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            D = cls(**kw).train()
        shapes = {k: tuple(v.shape) for k, v in D.state_dict().items()}
        D.load_state_dict(synth_norm_discriminator_state(shapes, seed), strict=True)
        p = case + "."
        G[p + "kwargs"], G[p + "type"], G[p + "seed"] = json.dumps(kw, sort_keys=True), d_type, np.int64(seed)
        G[p + "manifest"] = json.dumps({k: list(v) for k, v in shapes.items()}, sort_keys=True)
        xg = x.clone().requires_grad_(True)
        call = (lambda t: D(t, beta_1=b1, beta_2=b2, y_hat=None))
        l1 = call(xg)
        cot = torch.randn(l1.shape, generator=torch.Generator().manual_seed(seed + 100))
        (l1 * cot).sum().backward()
        G[p + "logits1"], G[p + "cot"], G[p + "grad_x"] = l1.detach().numpy(), cot.numpy(), xg.grad.numpy()
        for k, v in buffers(D).items():
            G[p + "buf1/" + k] = v
        first = "main.0.weight" if d_type == PATCHGAN else "body.0.0.weight"
        norm_keys = [f"{n}.{leaf}" for n, m in D.named_modules() for leaf in (("weight", "bias") if isinstance(m, torch.nn.BatchNorm2d) else
                                                                             ("loc", "scale") if type(m).__name__ == "ActNorm" else ())]
        params = dict(D.named_parameters())
        for k in norm_keys + [first]:
            G[p + "grad/" + k] = params[k].grad.numpy().copy()
        with torch.no_grad():
            G[p + "logits2"] = call(x).numpy()
        for k, v in buffers(D).items():
            G[p + "buf2/" + k] = v
        print(case, "logits", tuple(l1.shape), "max |logit|", float(l1.abs().max()), "max |grad_x|", float(xg.grad.abs().max()), "norm keys", len(norm_keys))
    np.savez_compressed(OUT, **G)
    print("disc_norm.npz:", len(G), "entries,", os.path.getsize(OUT), "bytes;", os.path.basename(SECTIONS), sorted(sections))


if __name__ == "__main__":
    main()
