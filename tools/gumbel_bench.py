#!/usr/bin/env python3
"""The Gumbel-softmax VQ sample (csrc/gumbel.hip) at the trainer's shape, beside the same arithmetic as torch ops on the device -- one
process, alternating, device events around synchronised batches of launches:
  dcvic_gumbel_lut_f32      forward  at (8, 256, 32 x 32), D = 4
  dcvic_gumbel_lut_bwd_f32  backward at the same shape
  torch                     z = (logits - log e) / tau; s = softmax(z, 1); ret = one_hot(argmax s) - s.detach() + s;
                            lat = post_quant(ret @ codebook), forward, and lat.backward(g) with autograd, on the same inputs
and, with --step, the G + D training step (train/trainer.py, the synthetic model, batch x 256 x 256) with gumbel_sampling off and on,
alternating on two trainers over one model.
python tools/gumbel_bench.py [--n 8 --c 256 --hw 32 --d 4 --tau 1] [--iters 200 --rounds 5] [--step --batch 8 --steps 5] [--out FILE]
Kernel-only time comes from a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o gumbel -- python tools/gumbel_bench.py --profile-only
(profiles/gumbel_kernel_stats.csv keeps that run's kernel_stats.csv).  Writes every part into one JSON file (default profiles/gumbel_bench.json) and prints it.  Bytes per call follow from the shapes:
forward 2 * N*C*HW*4 read plus the idx and latent written, backward 3 * N*C*HW*4 (two read, one written) plus the latent gradient read.
At 8 to 25 MB per call the bytes/s figure mostly shows launch and latency cost, not the memory system."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12          # bytes/s, the MI355X specification; a float4 copy reaches about 6.3e12


def kernel_part(a):
    from dc_vic_amd import ops
    from dc_vic_amd.train import kernels as K
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    shape = (a.n, a.c, a.hw, a.hw)
    logits = (3.0 * torch.randn(shape, generator=g)).to(dev)
    e = torch.empty(shape).exponential_(generator=g).to(dev)
    cb, w, b = torch.randn((a.c, a.d), generator=g).to(dev), (0.5 * torch.randn((a.d, a.d), generator=g)).to(dev), torch.randn(a.d, generator=g).to(dev)
    G = torch.randn((a.n, a.d, a.hw, a.hw), generator=g).to(dev)
    w4 = w.reshape(a.d, a.d, 1, 1)

    def torch_forward(lg):
        z = (lg - e.log()) / a.tau
        s = z.softmax(1)
        idx = s.max(1, keepdim=True)[1]
        ret = torch.zeros_like(lg).scatter_(1, idx, 1.0) - s.detach() + s
        return idx, torch.nn.functional.conv2d(torch.einsum("nchw,cd->ndhw", ret, cb), w4, b)

    def torch_fwd_only():
        with torch.no_grad():
            return torch_forward(logits)

    def torch_fwd_bwd():
        lg = logits.detach().requires_grad_(True)
        torch_forward(lg)[1].backward(G)
        return lg.grad

    if a.profile_only:                                     # for a rocprofv3 --kernel-trace --stats run: the two entry points alone
        for _ in range(10 + a.iters):
            ops.gumbel_lut(logits, e, cb, w, b, a.tau)
            K.gumbel_lut_bwd(logits, e, G, cb, w, a.tau)
        torch.cuda.synchronize()
        return None
    fns = {"gumbel_lut_us": lambda: ops.gumbel_lut(logits, e, cb, w, b, a.tau),
           "gumbel_lut_bwd_us": lambda: K.gumbel_lut_bwd(logits, e, G, cb, w, a.tau),
           "torch_forward_us": torch_fwd_only, "torch_forward_backward_us": torch_fwd_bwd}

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
    idx, lat = fns["gumbel_lut_us"]()
    idx_t, lat_t = torch_fwd_only()
    dl, dl_t = fns["gumbel_lut_bwd_us"](), torch_fwd_bwd()
    plane = a.n * a.c * a.hw * a.hw * 4
    small = a.n * a.hw * a.hw
    nbytes = {"gumbel_lut_us": 2 * plane + small * (8 + 4 * a.d), "gumbel_lut_bwd_us": 3 * plane + small * 4 * a.d}
    mins = {k: min(v) for k, v in t.items()}
    rate = {k.replace("_us", "_bytes_per_s"): nbytes[k] / (mins[k] * 1e-6) for k in nbytes}
    return {"part": "kernels", "shape": list(shape), "D": a.d, "tau": a.tau, "iters": a.iters, "rounds": a.rounds, **t,
            **{k + "_min": v for k, v in mins.items()}, "bytes_per_call": {k.replace("_us", ""): v for k, v in nbytes.items()}, **rate,
            **{k.replace("_bytes_per_s", "_fraction_of_hbm_peak"): v / HBM_PEAK for k, v in rate.items()}, "hbm_peak_bytes_per_s": HBM_PEAK,
            "torch_forward_over_gumbel_lut": mins["torch_forward_us"] / mins["gumbel_lut_us"],
            "torch_backward_over_gumbel_lut_bwd": (mins["torch_forward_backward_us"] - mins["torch_forward_us"]) / mins["gumbel_lut_bwd_us"],
            "idx_equal_torch": bool(torch.equal(idx, idx_t.squeeze(1))),
            "lat_vs_torch_rel": float((lat - lat_t).abs().max() / lat_t.abs().max()), "dlogits_vs_torch_rel": float((dl - dl_t).abs().max() / dl_t.abs().max()),
            "note": "per-call time of back-to-back launches incl. host launch cost and output allocation; the torch backward is the "
                    "forward + backward time minus the forward time"}


def step_part(a):
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondTamingNLayerDiscriminator
    dev = "cuda:0"
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": dev}))
    load_synth_weights(m, 1234)
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.rand((a.batch, 3, 256, 256), generator=torch.Generator().manual_seed(100)) * 2 - 1
    kw = dict(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, L=10, cond_ch=8, use_pi=False, include_x=True)

    def run(on, steps):
        """`steps` G + D steps of a fresh trainer from the synthetic weights: ms per step after `warmup` untimed ones."""
        m.load_state_dict(start)
        torch.manual_seed(0)
        tr = DualBetaCondGanDistortionVqCodeTrainer(m, DualBetaCondTamingNLayerDiscriminator(**kw).to(dev), seed=0, gumbel_sampling=on,
                                                    gumbel_kwargs=dict(tau=a.tau))
        tr.resync_parameters()
        done = 0
        for i in range(a.warmup):
            tr.optimize_parameters(i, {"real_images": x})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            done += tr.optimize_parameters(a.warmup + i, {"real_images": x}) is not None
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps, done

    t = {"argmax_step_ms": [], "gumbel_step_ms": []}
    done = 0
    for _ in range(a.rounds):
        for key, on in (("argmax_step_ms", False), ("gumbel_step_ms", True)):
            ms, d = run(on, a.steps)
            t[key].append(ms)
            done += d
    lo = {k + "_min": min(v) for k, v in t.items()}
    return {"part": "step", "metric": "G + D step @256x256, ms per step", "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, **t, **lo,
            "gumbel_over_argmax": lo["gumbel_step_ms_min"] / lo["argmax_step_ms_min"], "steps_not_skipped": done, "of": 2 * a.rounds * a.steps,
            "note": "host clock around synchronised windows; option off and on alternate in one process, each round a fresh trainer from the "
                    "same synthetic weights; synthetic LPIPS weights; the option adds the estimator's backward for the image losses and the data "
                    "gradient of the VQGAN decoder's conv_in"}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=8)
    p.add_argument("--c", type=int, default=256)
    p.add_argument("--hw", type=int, default=32)
    p.add_argument("--d", type=int, default=4)
    p.add_argument("--tau", type=float, default=1.0)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--step", action="store_true", help="also time the G + D training step with the option off and on")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--profile-only", action="store_true", help="10 + iters calls of each entry point and nothing else (for rocprofv3)")
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "gumbel_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gumbel_bench: needs a GPU; a CPU run measures nothing")
    if a.profile_only:
        kernel_part(a)
        return
    parts = [kernel_part(a)]
    if a.step:
        parts.append(step_part(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(parts, f, indent=1)
        f.write("\n")
    for part in parts:
        print(json.dumps(part), flush=True)


if __name__ == "__main__":
    main()
