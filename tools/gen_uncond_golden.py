#!/usr/bin/env python3
"""tests/golden/uncond.npz -- the unconditioned stage 1-1 sub-networks from the reference's OWN classes (build container only: needs the
reference tree; runs on the CPU).  Same recipe as tools/gen_oasis_golden.py:

  * `ElicVqCatScEncoder` / `ElicFeatFusionDecoder` (src/models/subnet/autoencoder/elic_insert_encoder.py, elic_feat_decoder.py) built
    with config/exp1_stage1_1.yaml's kwargs, the synthetic state (seed 1234) restricted to their 140 + 138 keys loaded strict=True --
    the fixture stores the key -> shape manifests and the seed, not the weights;
  * inputs: 2 x 3 x 64 x 64 images on the 8-bit grid (stored as uint8: x = u8 / 127.5 - 1), their VQ indices from the oracle's VQGAN
    encoder on the same synthetic state (the encoder's feature is cat[latent, one-hot] of them);
  * stored: `y` of both images; the decoder's input `y_hat` = round(8 y[:1]) (integers as a quantised
    latent's, and not all zero as round(y) is with these weights) and, for that ONE image (a committed file holds at most
    1 MiB), `feat_1` (the block1 output, which is also the block_1_8 fusion feature) and the block_1_4 / block_1_2 fusion features;
  * the first 8 values of the reference's LinearWarmupScheduler (warmup_iters 5, warmup_factor 0.1, base lr 1e-4) when
    src/trainer/optimizer/build_optimizer_scheduler.py imports here, else `warmup_lr` is absent and the host test compares with
    torch's LambdaLR alone.

    python tools/gen_uncond_golden.py
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

from oracle import dcvic_oracle as O  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "uncond.npz")
SEED, IMG_SEED = 1234, 311


def warmup_values():
    """The reference scheduler's lr over 8 steps, or None when its module does not import (it pulls in the logger and registries)."""
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            bo = ref_loader.ref("src.trainer.optimizer.build_optimizer_scheduler")
    except Exception as e:                                 # noqa: BLE001 -- any import failure means "not available here"
        print("LinearWarmupScheduler does not import here:", type(e).__name__, e)
        return None
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-4)
    sch = bo.LinearWarmupScheduler(opt, warmup_iters=5, warmup_factor=0.1)
    out = []
    for _ in range(8):
        out.append(opt.param_groups[0]["lr"])
        opt.step(); sch.step()
    return np.asarray(out, dtype=np.float64)


def main():
    torch.set_num_threads(8)
    ref_loader.install_training_names()
    from dc_vic_amd.synth import full_synth_state_dict
    top = yaml.safe_load(open(os.path.join(ref_loader.REF, "config/exp1_stage1_1.yaml")))
    with contextlib.redirect_stdout(io.StringIO()):
        em = ref_loader.ref("src.models.subnet.autoencoder.elic_insert_encoder")
        dm = ref_loader.ref("src.models.subnet.autoencoder.elic_feat_decoder")
    ecfg, dcfg = dict(top["subnet"]["encoder"]), dict(top["subnet"]["decoder"])
    for c, t in ((ecfg, "ElicVqCatScEncoder"), (dcfg, "ElicFeatFusionDecoder")):
        c.pop("_delete_", None)
        assert c.pop("type") == t
    enc, dec = em.ElicVqCatScEncoder(**ecfg).eval(), dm.ElicFeatFusionDecoder(**dcfg).eval()
    sd = full_synth_state_dict(SEED)
    G = {"seed": np.int64(SEED), "enc_kwargs": json.dumps(ecfg, sort_keys=True), "dec_kwargs": json.dumps(dcfg, sort_keys=True)}
    for tag, mod in (("encoder", enc), ("decoder", dec)):
        shapes = {k: list(v.shape) for k, v in mod.state_dict().items()}
        mod.load_state_dict({k: sd[f"{tag}.{k}"] for k in shapes}, strict=True)
        G[f"{tag}_manifest"] = json.dumps(shapes, sort_keys=True)
    u8 = torch.randint(0, 256, (2, 3, 64, 64), generator=torch.Generator().manual_seed(IMG_SEED), dtype=torch.uint8)
    x = u8.float() / 127.5 - 1.0
    with torch.no_grad():
        zq, idx = O.vq_encode(sd, x)
        y = enc(x, O.onehot_feat(sd, zq, idx))
        y_hat = torch.round(8.0 * y[:1])
        feat_1, feats = dec.get_feats(y_hat)
    assert torch.equal(feat_1, feats["block_1_8"]) and sorted(feats) == ["block_1_2", "block_1_4", "block_1_8"]
    G.update(x_u8=u8.numpy(), vq_indices=idx.numpy().astype(np.int16), y=y.numpy(), y_hat=y_hat.numpy(), feat_1=feat_1.numpy(),
             block_1_4=feats["block_1_4"].numpy(), block_1_2=feats["block_1_2"].numpy())
    w = warmup_values()
    if w is not None:
        G["warmup_lr"] = w
    np.savez_compressed(OUT, **G)
    print("uncond.npz:", {k: (v.shape if hasattr(v, "shape") else v) for k, v in G.items() if not isinstance(v, str)}, os.path.getsize(OUT), "bytes",
          "max |y|", float(y.abs().max()), "nonzero y_hat", int((y_hat != 0).sum()))


if __name__ == "__main__":
    main()
