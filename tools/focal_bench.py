#!/usr/bin/env python3
"""dcvic_focal_ce_f32 (value + gradient in one pass) at the trainer's shape, beside the plain cross entropy the trainer runs
(dcvic_cross_entropy_f32 + dcvic_reduce_loss_f32) at gamma 0 -- one process, alternating, device events around synchronised batches
of launches -- and, with --step, the stage-3 training step of tools/train_bench.py with the beta grid sampler against selected
pairs (one trainer, the model's use_selected_beta_pairs flipped between rounds) and with the focal code loss.
python tools/focal_bench.py [--n 8 --c 256 --hw 32] [--iters 200 --rounds 5] [--step --batch 8 --steps 5]
Prints one JSON line per part.  Bytes: the logits read once and the gradient written once; at this size the figure mostly shows
launch and latency cost, not bandwidth."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_part(a):
    from dc_vic_amd.train import kernels as K
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    lg = (torch.randn((a.n, a.c, a.hw, a.hw), generator=g) * 2).to(dev)
    idx = torch.randint(0, a.c, (a.n, a.hw, a.hw), generator=g).to(dev)
    scale = 0.5 / (a.n * a.hw * a.hw)

    def focal(gamma):
        return lambda: K.focal_ce(lg, idx, gamma, scale, want_grad=True)

    def plain():
        nll, dl = K.cross_entropy(lg, idx, scale, want_grad=True)
        return K.reduce_loss(3, nll, None, scale), dl

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters          # microseconds per call

    fns = {"focal_gamma2_us": focal(2.0), "focal_gamma0_us": focal(0.0), "cross_entropy_plus_reduce_us": plain}
    for _ in range(20):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    same = abs(float(focal(0.0)()[0]) - float(plain()[0]))
    nbytes = 2 * lg.numel() * 4 + idx.numel() * 8
    print(json.dumps({"part": "kernel", "shape": [a.n, a.c, a.hw, a.hw], "iters": a.iters, **t, **{k + "_min": min(v) for k, v in t.items()},
                      "bytes": nbytes, "focal_gamma2_GBps_at_min": nbytes / min(t["focal_gamma2_us"]) * 1e-3,
                      "gamma0_minus_plain_value": same,
                      "note": "per-call time of back-to-back launches incl. host launch cost and output allocation"}), flush=True)


def step_part(a):
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondTamingNLayerDiscriminator, FocalCrossEntropyLoss
    dev = "cuda:0"
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": dev}))
    load_synth_weights(m, 1234)
    torch.manual_seed(0)
    D = DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5).to(dev)
    tr = DualBetaCondGanDistortionVqCodeTrainer(m, D, seed=0)
    x = torch.rand((a.batch, 3, 256, 256), generator=torch.Generator().manual_seed(100)) * 2 - 1
    modes = {"selected_pairs_plain_ce": (True, None), "beta_grid_plain_ce": (False, None),
             "beta_grid_focal_gamma2": (False, FocalCrossEntropyLoss(tr.w["code_ce"], 2.0))}

    def run(mode, steps):
        m.use_selected_beta_pairs, tr.code_ce_loss = modes[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            tr.optimize_parameters(i, {"real_images": x})
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps      # milliseconds per step

    for mode in modes:
        run(mode, a.warmup)
    t = {k: [] for k in modes}
    for _ in range(a.rounds):
        for mode in modes:
            t[mode].append(run(mode, a.steps))
    print(json.dumps({"part": "step", "metric": "stage-3 G+D step @256x256, ms per step", "batch": a.batch, "steps": a.steps, "rounds": a.rounds,
                      **{k + "_ms": v for k, v in t.items()}, **{k + "_ms_min": min(v) for k, v in t.items()},
                      "note": "host clock around synchronised windows, the three modes alternating in one process on one trainer"}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=8)
    p.add_argument("--c", type=int, default=256)
    p.add_argument("--hw", type=int, default=32)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--step", action="store_true", help="also time the training step (grid sampler vs selected pairs, focal vs plain)")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("focal_bench: needs a GPU; a CPU run measures nothing")
    kernel_part(a)
    if a.step:
        step_part(a)


if __name__ == "__main__":
    main()
