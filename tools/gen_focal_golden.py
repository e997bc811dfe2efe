#!/usr/bin/env python3
"""tests/golden/focal.npz -- the reference's OWN `FocalCrossEntropyLoss` (src/losses/cross_entropy_loss.py:32-53) on seeded inputs
(build container only: needs the reference tree; runs on the CPU, fp32 as the reference trains).  Same recipe as
tools/gen_oasis_golden.py:

  * `logits` [2, 256, 8, 8] = randn * 2 (seed 181), `target` [2, 8, 8] int64 (seed 182) with both ends of the codebook;
  * for gamma in {0, 1, 2} and reduction in {mean, sum}: `FocalCrossEntropyLoss(loss_weight=0.05, gamma, reduction)(logits, target)`
    as `loss_g<gamma>_<reduction>` and its autograd gradient d loss / d logits as `grad_g<gamma>_<reduction>`;
  * `loss_weight`, `gammas`, `reductions` name what was run.

Beside it tests/golden/reference_loss_sections.json: the `trainer` and `loss` sections of every YAML under the reference's config/
after `_base_` inheritance (settings only), which tests/test_focal_host.py feeds to read_loss_section.

    python tools/gen_focal_golden.py
"""
from __future__ import annotations

import contextlib
import glob
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "focal.npz")
OUT_SECTIONS = os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")
LOSS_WEIGHT = 0.05
GAMMAS = (0.0, 1.0, 2.0)
REDUCTIONS = ("mean", "sum")


def loss_sections():
    from dc_vic_amd import BaseConfig
    out = {}
    for path in sorted(glob.glob(os.path.join(ref_loader.REF, "config", "*.yaml"))):
        opt = BaseConfig.fromfile(path, {"is_train": True})
        out[os.path.basename(path)] = {k: opt.get(k) for k in ("trainer", "loss")}
    with open(OUT_SECTIONS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("reference_loss_sections.json:", sorted(out))


def main():
    torch.set_num_threads(8)
    loss_sections()
    ref_loader.install_training_names()
    with contextlib.redirect_stdout(io.StringIO()):
        cl = ref_loader.ref("src.losses.cross_entropy_loss")
    logits = torch.randn((2, 256, 8, 8), generator=torch.Generator().manual_seed(181)) * 2
    target = torch.randint(0, 256, (2, 8, 8), generator=torch.Generator().manual_seed(182))
    target[0, 0, 0], target[1, 7, 7] = 0, 255              # both ends of the codebook
    G = {"logits": logits.numpy(), "target": target.numpy(), "loss_weight": np.float64(LOSS_WEIGHT), "gammas": np.asarray(GAMMAS, dtype=np.float64),
         "reductions": np.asarray(REDUCTIONS)}
    for gamma in GAMMAS:
        for red in REDUCTIONS:
            loss = cl.FocalCrossEntropyLoss(loss_weight=LOSS_WEIGHT, gamma=gamma, reduction=red)
            lg = logits.clone().requires_grad_(True)
            val = loss(lg, target)
            val.backward()
            G[f"loss_g{gamma:g}_{red}"], G[f"grad_g{gamma:g}_{red}"] = val.detach().numpy(), lg.grad.numpy()
    np.savez_compressed(OUT, **G)
    print("focal.npz:", {k: (v.shape if hasattr(v, "shape") and v.shape else v) for k, v in G.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
