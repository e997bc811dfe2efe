#!/usr/bin/env python3
"""Decoder precision fp32 vs bf16 (model.set_decoder_precision) on the bench workload: config 2 (synthetic 256x256 images, batch 32,
quality 0, compress_batch + decompress_batch through real rANS bytes, hipGraph segments on), one GPU.

Reports per mode: images/s, decode-NN ms per step (the eager decoder network, device-synchronised), the fraction of the marked
layers' launches that ran on the bf16 kernel, per-shape kernel time / TFLOP/s (HIP events around each convolution launch of one eager
decode: conv3x3_bf16_kernel against the fp32 kernels of the same shapes), N = 1 compress + decompress latency at 256x256 and
512x768; and the PSNR of the bf16 reconstruction against the fp32 one.  One JSON document on stdout (or --out).

    python tools/bf16_decode_bench.py --steps 10 --warmup 2 --out profiles/bf16_decode_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_PEAK_TF = 2500.0      # MI355X dense bf16 MFMA, spec


def psnr01(a, b):
    mse = float((((a.double() - b.double()) / 2) ** 2).mean())
    return float("inf") if mse == 0 else 10 * np.log10(1.0 / mse)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--quality", type=int, default=0)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--latency_reps", type=int, default=10)
    p.add_argument("--out", type=str, default="")
    a = p.parse_args()

    from dc_vic_amd import BaseConfig, build_comp_model, ops
    from dc_vic_amd.layers import Conv2d
    from dc_vic_amd.synth import load_synth_weights
    dev = torch.device("cuda:0")
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": str(dev)})
    model = build_comp_model(opt)
    load_synth_weights(model, 1234)
    model.codec_setup()
    g = torch.Generator().manual_seed(1000)
    x = (torch.rand((a.batch, 3, 256, 256), generator=g) * 2 - 1).to(dev)
    q = a.quality
    br, bv = model.selected_beta_rate[q], model.selected_beta_vq[q]
    marked = [m for mod in (model.vq_model.decoder, model.fusion_module) for m in mod.modules()
              if isinstance(m, Conv2d) and m.kernel_size == 3 and m.stride == 1 and m.padding == 1]

    def log(msg):
        print(f"[bf16_bench] {msg}", file=sys.stderr, flush=True)

    res = {"workload": f"config 2: synthetic 256x256, batch {a.batch}, q{q}, compress_batch + decompress_batch (real rANS bytes)",
           "modes": {}}
    recon = {}
    r0 = model.compress_batch(x, q)
    streams = r0["string_lists"]
    _, _, y_hat = model.decompress_batch(streams)
    for mode in ("fp32", "bf16"):
        model.set_decoder_precision(mode)
        out = {}

        def step():
            r = model.compress_batch(x, q)
            imgs, _, _ = model.decompress_batch(r["string_lists"])
            return imgs

        for _ in range(2 + a.warmup):          # packs, hipGraph capture, warm-up
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            imgs = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["images_per_s"] = a.batch * a.steps / dt
        out["step_ms"] = 1e3 * dt / a.steps
        recon[mode], _, _ = model.decompress_batch(streams)
        # decode NN: the eager decoder network of the same latents
        for m in marked:
            if m._plan is not None:
                m._plan.bf16_launches = m._plan.fp32_launches = 0
        model._decode(y_hat, 1.0, br, bv)
        torch.cuda.synchronize()
        n16 = sum(m._plan.bf16_launches for m in marked if m._plan is not None)
        n32 = sum(m._plan.fp32_launches for m in marked if m._plan is not None)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            model._decode(y_hat, 1.0, br, bv)
        torch.cuda.synchronize()
        out["decode_nn_ms_eager"] = 1e3 * (time.perf_counter() - t0) / a.steps
        if mode == "bf16":
            out["marked_launches_bf16"] = n16
            out["marked_launches_total"] = n16 + n32
            out["bf16_launch_fraction"] = n16 / max(1, n16 + n32)
            out["marked_layers_fp32"] = sorted(n for n, m in model.named_modules() if any(m is k for k in marked)
                                               and m._plan is not None and m._plan.fp32_launches)
        # per-shape kernel time of one eager decode
        ops.kernel_events_start()
        model._decode(y_hat, 1.0, br, bv)
        torch.cuda.synchronize()
        ops.kernel_events_stop()
        shapes = []
        for k, (n, fl, t) in sorted(ops.LAST_SHAPE_STATS.items(), key=lambda kv: -kv[1][2]):
            cfg, Cin, Cout, T, st, ups, H, W, N = k
            if T != 9 or st != 1 or Cin < 8 or Cout < 16:
                continue
            shapes.append({"kernel": ops.conv_kernel_name(cfg), "Cin": Cin, "Cout": Cout, "upsample": bool(ups), "H_in": H, "W_in": W, "N": N,
                           "launches": n, "ms": 1e3 * t, "tflops_algorithmic": fl / t / 1e12 if t > 0 else 0.0,
                           "pct_of_bf16_peak": 100.0 * fl / t / 1e12 / BF16_PEAK_TF if t > 0 else 0.0})
        out["conv3x3_shapes"] = shapes
        # N = 1 latency, compress + decompress
        lat = {}
        for (H, W) in ((256, 256), (512, 768)):
            xi = (torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(H)) * 2 - 1).to(dev)
            for _ in range(3):
                model.decompress(model.compress(xi, q)["string_list"])
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.latency_reps):
                t0 = time.perf_counter()
                model.decompress(model.compress(xi, q)["string_list"])
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            lat[f"{W}x{H}"] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts))}
        out["latency_n1_compress_decompress"] = lat
        res["modes"][mode] = out
        log(f"{mode}: {out['images_per_s']:.1f} images/s, decode NN {out['decode_nn_ms_eager']:.2f} ms, latency {lat}")
    model.set_decoder_precision("fp32")
    ps = [psnr01(recon["bf16"][i], recon["fp32"][i]) for i in range(a.batch)]
    res["psnr_bf16_vs_fp32_db"] = {"min": min(ps), "max": max(ps), "mean": float(np.mean(ps))}
    res["max_abs_diff"] = float((recon["bf16"] - recon["fp32"]).abs().max())
    res["bf16_kernel_mfma_shape"] = int(__import__("dc_vic_amd")._lib.lib().dcvic_conv3x3_bf16_mfma_shape())
    s = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
