#!/usr/bin/env python3
"""Which of the bf16-eligible decoder / SFT 3x3 layers cost the most reconstruction fidelity (source of the fp32 exemptions in
dc_vic_amd/fusion.py and vqgan.py).

For each marked layer alone on bf16 (every other layer fp32): PSNR of the reconstruction against the all-fp32 one, on the five synthetic
256x256 cases (q 0..4) and the demo images.  Then the greedy curve: all layers on bf16 except the k worst, k = 0, 1, ...  One JSON
document on stdout (or --out).  Exemptions already in the code are ignored here (every marked layer is a candidate)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", type=str, default="")
    p.add_argument("--max_k", type=int, default=16)
    a = p.parse_args()
    from PIL import Image

    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.layers import Conv2d
    from dc_vic_amd.synth import load_synth_weights
    dev = "cuda:0"
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": dev})
    model = build_comp_model(opt)
    load_synth_weights(model, 1234)
    model.codec_setup()
    model._graphs.disabled = True
    cases = []
    for q in range(5):
        x = torch.rand((1, 3, 256, 256), generator=torch.Generator().manual_seed(100 + q)) * 2 - 1
        cases.append((f"synth_q{q}", x, q))
    demo = os.path.join(ROOT, "tests", "golden", "demo_images")
    for n in sorted(os.listdir(demo)):
        x = torch.from_numpy(np.asarray(Image.open(os.path.join(demo, n)).convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1).float()
        cases.append((n, (x / 255.0 - 0.5).div(0.5).unsqueeze(0), 2))
    lat = []
    for name, x, q in cases:
        r = model.compress(x, q)
        _, _, y_hat = model.decompress(r["string_list"])
        lat.append((name, y_hat, q))
    layers = [(n, m) for n, m in model.named_modules() if isinstance(m, Conv2d) and m.wino44 and m.in_channels % 8 == 0 and m.out_channels >= 16]

    def set_on(names):
        for n, m in layers:
            m.bf16 = n in names
            m.bf16_keep_fp32 = False

    def recon():
        out = []
        for name, y_hat, q in lat:
            img, _ = model._decode(y_hat, 1.0, model.selected_beta_rate[q], model.selected_beta_vq[q])
            out.append(img.clone())
        return out

    def mse(a_, b_):
        return [float((((u.double() - v.double()) / 2) ** 2).mean()) for u, v in zip(a_, b_)]

    set_on(set())
    ref = recon()
    per = {}
    for n, _ in layers:
        set_on({n})
        per[n] = mse(recon(), ref)
        print(f"[sens] {n}: worst case {10 * np.log10(1 / max(per[n])):.2f} dB", file=sys.stderr, flush=True)
    order = sorted(per, key=lambda n: -float(np.mean(per[n])))
    curve = []
    for k in range(0, min(a.max_k, len(order)) + 1):
        set_on(set(order[k:]))
        e = mse(recon(), ref)
        curve.append({"k": k, "fp32_layers": order[:k], "min_psnr_db": 10 * np.log10(1 / max(e)), "mean_mse": float(np.mean(e))})
        print(f"[sens] k={k}: min PSNR {curve[-1]['min_psnr_db']:.2f} dB", file=sys.stderr, flush=True)
    res = {"cases": [c[0] for c in cases],
           "per_layer": [{"layer": n, "Cin": m.in_channels, "Cout": m.out_channels, "upsample": bool(m.upsample),
                          "alone_min_psnr_db": 10 * np.log10(1 / max(per[n])), "alone_mean_mse": float(np.mean(per[n]))}
                         for n, m in sorted(layers, key=lambda nm: -float(np.mean(per[nm[0]])))],
           "greedy": curve}
    s = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
