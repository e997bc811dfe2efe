#!/usr/bin/env python3
"""The two per-image weighted loss calls (csrc/sample_loss.hip) at the stage 1-2 trainer's shapes, beside what they replace -- one
process, alternating, device events around synchronised batches of launches:
  dcvic_focal_ce_sample_f32 at (8, 256, 32, 32)   against N per-image calls of dcvic_focal_ce_f32 (one scale each), their values added
  dcvic_sq_err_sample_f32   at (8, 4, 32, 32)     against reduce_loss(SUM_SQ_ERR) + ew(EW_MSE_GRAD), the two launches of mse_loss (which
                                                   take ONE weight: the per-image form would need N of each)
and, with --step, the stage 1-2 training step (train/rd_trainer.py, config/exp1_stage1_2.yaml's trainer and loss sections over the
synthetic model) with its forward + losses, backward and optimizer + aux parts timed apart by host clock around synchronisations.
python tools/sample_loss_bench.py [--n 8 --c 256 --hw 32 --d 4] [--iters 200 --rounds 5] [--step --batch 8 --steps 5]
Prints one JSON line per part.  These calls are launch-bound at these sizes: the figures show launch and latency cost."""
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
    lat, gt = torch.randn((a.n, a.d, a.hw, a.hw), generator=g).to(dev), torch.randn((a.n, a.d, a.hw, a.hw), generator=g).to(dev)
    wl = [0.003 * (1.0 + 0.5 * i) / (a.n * a.hw * a.hw) for i in range(a.n)]
    w = torch.tensor(wl, dtype=torch.float32, device=dev)
    per_image = [(lg[i:i + 1], idx[i:i + 1]) for i in range(a.n)]

    def focal_sample():
        return K.focal_ce_sample(lg, idx, w, 2.0, want_grad=True)

    def focal_per_image():
        out = [K.focal_ce(l, t, 2.0, s, want_grad=True) for (l, t), s in zip(per_image, wl)]
        val = out[0][0]
        for o in out[1:]:
            val = K.ew(K.EW_ADD, None, val, o[0])
        return val, [o[1] for o in out]

    def sq_sample():
        return K.sq_err_sample(lat, gt, w, want_grad=True)

    def sq_composed():
        return K.reduce_loss(K.SUM_SQ_ERR, lat, gt, wl[0]), K.ew(K.EW_MSE_GRAD, None, lat, gt, w=wl[0])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters          # microseconds per call

    fns = {"focal_ce_sample_us": focal_sample, "focal_ce_per_image_calls_us": focal_per_image, "sq_err_sample_us": sq_sample,
           "reduce_loss_plus_ew_us": sq_composed}
    for _ in range(20):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    dv = abs(float(focal_sample()[0]) - float(focal_per_image()[0])) / abs(float(focal_sample()[0]))
    print(json.dumps({"part": "kernels", "focal_shape": [a.n, a.c, a.hw, a.hw], "sq_err_shape": [a.n, a.d, a.hw, a.hw], "iters": a.iters, **t,
                      **{k + "_min": min(v) for k, v in t.items()}, "focal_sample_vs_per_image_value_rel": dv,
                      "note": "per-call time of back-to-back launches incl. host launch cost and output allocation; reduce_loss + ew is the "
                              "single-weight composition (2 launches), the per-image calls are N x 2 launches + N - 1 adds"}), flush=True)


def step_part(a):
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    from dc_vic_amd.train import DualBetaCondRateDistortionVqCodeTrainer
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train.build import rd_trainer_kwargs
    from dc_vic_amd.train.losses import read_loss_section
    dev = "cuda:0"
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        opt = json.load(f)["exp1_stage1_2.yaml"]
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": dev}))
    load_synth_weights(m, 1234)
    tr = DualBetaCondRateDistortionVqCodeTrainer(m, seed=0, **rd_trainer_kwargs(opt, read_loss_section(opt)))
    x = torch.rand((a.batch, 3, 256, 256), generator=torch.Generator().manual_seed(100)) * 2 - 1
    sync = torch.cuda.synchronize

    def whole(steps):
        sync()
        t0 = time.perf_counter()
        done = 0
        for i in range(steps):
            done += tr.optimize_parameters(i, {"real_images": x}) is not None
        sync()
        return 1e3 * (time.perf_counter() - t0) / steps, done

    def split(steps):
        """The same step with a synchronisation after each part (so the parts add up to more than the whole step's time)."""
        acc = dict(forward_ms=0.0, backward_ms=0.0, optimizer_ms=0.0, aux_ms=0.0)
        for i in range(steps):
            beta_rate, beta_vq = tr.sample_beta_pair(a.batch)
            tr.group.zero_grad()
            ctx = A.Ctx([tr.group])
            sync(); t0 = time.perf_counter()
            tr.forward_losses(ctx, x, None, beta_rate, beta_vq)
            sync(); t1 = time.perf_counter()
            ctx.backward()
            sync(); t2 = time.perf_counter()
            tr.apply_gradients(None, tr.opt, tr.sched.lr(), tr.clip)         # the tape has run: all-reduce, clip scale, Adam
            tr.sched.step()
            sync(); t3 = time.perf_counter()
            tr.optimize_aux_parameters()
            sync(); t4 = time.perf_counter()
            for k, v in zip(acc, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                acc[k] += 1e3 * v / steps
        return acc

    whole(a.warmup)
    t, parts, done = [], [], 0
    for _ in range(a.rounds):
        ms, d = whole(a.steps)
        t.append(ms)
        done += d
        parts.append(split(a.steps))
    print(json.dumps({"part": "step", "metric": "stage 1-2 rate-distortion step @256x256, ms per step", "batch": a.batch, "steps": a.steps,
                      "rounds": a.rounds, "step_ms": t, "step_ms_min": min(t), "samples_per_s_at_min": a.batch / min(t) * 1e3,
                      "steps_not_skipped": done, "of": a.rounds * a.steps,
                      **{k + "_min": min(p[k] for p in parts) for k in parts[0]}, "parts": parts,
                      "note": "host clock around synchronised windows; whole steps and split steps alternate in one process on one trainer; "
                              "synthetic weights, synthetic LPIPS weights"}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=8)
    p.add_argument("--c", type=int, default=256)
    p.add_argument("--hw", type=int, default=32)
    p.add_argument("--d", type=int, default=4)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--step", action="store_true", help="also time the stage 1-2 training step and its parts")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_loss_bench: needs a GPU; a CPU run measures nothing")
    kernel_part(a)
    if a.step:
        step_part(a)


if __name__ == "__main__":
    main()
