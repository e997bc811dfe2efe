#!/usr/bin/env python3
"""The MS-SSIM distortion loss (csrc/msssim_loss.hip) at the trainer's crop, beside the same arithmetic as torch ops on the device -- one
process, alternating, device events around back-to-back calls:
  dcvic_msssim_loss_f32   forward, and forward + gradient, at (8, 3, 256, 256)
  dcvic_abs_err_f32       value + gradient at the same shape
  torch                   tests/msssim_loss_ref.py's fp32 restatement on the device, forward under no_grad and forward + autograd backward
python tools/msssim_loss_bench.py [--n 8 --hw 256] [--iters 200 --rounds 5] [--out FILE]
Writes one JSON file (default profiles/msssim_loss_bench.json) and prints it.  The per-call times include the host launch cost and the
output allocations of train.kernels; the loss is 11 launches forward and 5 more backward on 6 MB of images, so the figures show launch
and latency cost, not the memory system."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=8)
    p.add_argument("--hw", type=int, default=256)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "msssim_loss_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_loss_bench: needs a GPU; a CPU run measures nothing")
    import msssim_loss_ref as R
    from dc_vic_amd.train import kernels as K
    dev = "cuda:0"
    shape = (a.n, 3, a.hw, a.hw)
    real, fake = (t.to(dev) for t in R.pair(shape, "far"))
    scale = 50.0 / (a.n * 3)

    def torch_fwd():
        with torch.no_grad():
            return R.ms_ssim_loss(real, fake, 50.0, torch.float32)

    def torch_fwd_bwd():
        y = fake.detach().requires_grad_(True)
        R.ms_ssim_loss(real, y, 50.0, torch.float32).backward()
        return y.grad

    fns = {"msssim_loss_forward_us": lambda: K.ms_ssim_loss(real, fake, scale, want_grad=False),
           "msssim_loss_forward_gradient_us": lambda: K.ms_ssim_loss(real, fake, scale),
           "abs_err_value_gradient_us": lambda: K.abs_err(fake, real, 50.0 / fake.numel()),
           "torch_forward_us": torch_fwd, "torch_forward_backward_us": torch_fwd_bwd}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters          # microseconds per call

    for _ in range(10):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    loss, df, _ = fns["msssim_loss_forward_gradient_us"]()
    g_t = torch_fwd_bwd()
    mins = {k + "_min": min(v) for k, v in t.items()}
    out = {"shape": list(shape), "regime": "far", "iters": a.iters, "rounds": a.rounds, **t, **mins,
           "torch_forward_over_kernel": mins["torch_forward_us_min"] / mins["msssim_loss_forward_us_min"],
           "torch_forward_backward_over_kernel": mins["torch_forward_backward_us_min"] / mins["msssim_loss_forward_gradient_us_min"],
           "loss_vs_torch_fp32_abs": abs(float(loss) - float(torch_fwd())), "gradient_vs_torch_fp32_rel_max": float((df - g_t).abs().max() / g_t.abs().max()),
           "note": "per-call time of back-to-back calls incl. host launch cost and output allocation; device events"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
