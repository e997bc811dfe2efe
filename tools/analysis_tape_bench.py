"""Forward + backward of the analysis side on the tape (train/nets.analysis_forward: beta-conditioned ELIC encoder, hyper-encoder,
entropy bottleneck, hyper-decoder, six CHARM slices) at batch 8 x 256x256, synthetic weights: device-event times over 5 alternating
rounds of the two weight-gradient forms of the multi-source convolutions (one dcvic_conv_wgrad_src_f32 launch per source against one
cat per multi-source conv + one launch), library calls per step, and the forward / backward split.  Prints one JSON document;
`--out` also writes it.  `--kernel-stats CSV` folds a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of a separate run in:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tape -- python tools/analysis_tape_bench.py --profile-only
    python tools/analysis_tape_bench.py --kernel-stats DIR/.../tape_kernel_stats.csv --out profiles/analysis_tape_bench.json
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
PROFILE_STEPS = 3


def build():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    from dc_vic_amd.train import autograd as A
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    for t in m.context_model.scale_slice_transforms:        # synthetic sigmas sit below the 0.11 bound otherwise (see tests/analysis_train_ref.py)
        t.model[4].bias.data += 1.5
    grp = A.ParamGroup([m.encoder, m.hyperencoder, m.hyperdecoder, m.context_model, m.entropy_model_z], DEV)
    return m, grp


class Step:
    def __init__(self, m, grp, N, H, W):
        g = torch.Generator().manual_seed(3)
        self.m, self.grp = m, grp
        self.x = (torch.rand((N, 3, H, W), generator=g) * 2 - 1).to(DEV)
        self.b1 = torch.rand(N, generator=g) * 3.0
        self.b2 = torch.rand(N, generator=g) * 3.5
        self.w = (0.5 + torch.rand(N, generator=g)).to(DEV)
        self.G = (torch.randn((N, 192, H // 16, W // 16), generator=g) * 0.05).to(DEV)
        self.gen = torch.Generator(device=DEV).manual_seed(5)
        with torch.no_grad():
            _, self.idx = m.vq_encode(self.x)
        self.scale = 1.0 / (H * W)
        self.mid = torch.cuda.Event(enable_timing=True)

    def __call__(self, vq=True):
        from dc_vic_amd.train import autograd as A
        from dc_vic_amd.train import nets
        self.grp.zero_grad()
        ctx = A.Ctx([self.grp])
        out = nets.analysis_forward(ctx, self.m, self.x, self.b1, self.b2, vq_indices=None if vq else self.idx, generator=self.gen,
                                    weights=self.w, scale=self.scale)
        A.eb_aux_loss(ctx, self.m.entropy_model_z)
        out["quantized_code"]["y"].grad = self.G
        self.mid.record()
        ctx.backward()
        return out


def timed(step, n, **kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fwd = []
    tot = []
    for _ in range(n):
        e0.record()
        step(**kw)
        e1.record()
        torch.cuda.synchronize()
        tot.append(e0.elapsed_time(e1))
        fwd.append(e0.elapsed_time(step.mid))
    return statistics.median(tot), statistics.median(fwd)


def count_calls(step):
    """Library entry-point calls of one step (a weight gradient is two kernels: partials + slab reduce; a k5/s2 transposed
    convolution four phase launches, counted one by one)."""
    from dc_vic_amd import ops
    from dc_vic_amd.train import kernels as K
    n = [0]
    real_o, real_k = ops.check, K.check

    def counting(rc, what=""):
        n[0] += 1
        return real_o(rc, what)
    ops.check = K.check = counting
    try:
        step()
        torch.cuda.synchronize()
    finally:
        ops.check, K.check = real_o, real_k
    return n[0]


def kernel_stats(path, steps):
    rows = list(csv.DictReader(open(path)))
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    calls = sum(int(r["Calls"]) for r in rows)
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]
    return {"source": os.path.basename(path), "steps_in_trace": steps, "kernel_launches_per_step": calls / steps,
            "kernel_ms_per_step": total_ns * 1e-6 / steps, "mean_kernel_us": total_ns * 1e-3 / max(calls, 1),
            "top": [{"kernel": r["Name"][:90], "calls_per_step": int(r["Calls"]) / steps, "ms_per_step": float(r["TotalDurationNs"]) * 1e-6 / steps,
                     "mean_us": float(r["AverageNs"]) * 1e-3, "pct": float(r["Percentage"])} for r in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-only", action="store_true", help=f"warm up, then {PROFILE_STEPS} steps and nothing else (for rocprofv3)")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a --profile-only run under rocprofv3")
    ap.add_argument("--out")
    a = ap.parse_args()
    from dc_vic_amd.train import autograd as A
    m, grp = build()
    step = Step(m, grp, a.batch, a.size, a.size)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    if a.profile_only:
        for _ in range(PROFILE_STEPS):
            step()
        torch.cuda.synchronize()
        return
    res = {"workload": f"analysis side forward + backward, batch {a.batch} x {a.size}x{a.size}, synthetic weights, fp32",
           "device": torch.cuda.get_device_name(0), "steps_per_round": a.steps, "rounds": a.rounds}
    per_round = {"per_source": [], "cat": []}
    default = A.WGRAD_PER_SOURCE
    fwd_ms = []
    for _ in range(a.rounds):
        for mode in ("per_source", "cat"):
            A.WGRAD_PER_SOURCE = mode == "per_source"
            tot, fwd = timed(step, a.steps)
            per_round[mode].append(tot)
            if mode == "per_source":
                fwd_ms.append(fwd)
    A.WGRAD_PER_SOURCE = default
    res["tape_default"] = "per_source" if default else "cat"
    res["step_ms"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for k, v in per_round.items()}
    res["forward_ms"] = statistics.median(fwd_ms)
    res["backward_ms"] = res["step_ms"]["per_source"]["median"] - res["forward_ms"]        # (both of the per-source form)
    res["step_ms_without_vq_encode"] = timed(step, a.steps, vq=False)[0]
    res["library_calls_per_step"] = count_calls(step)
    res["stage3_step_ms_for_scale"] = 150.0
    if a.kernel_stats:
        res["kernel_stats"] = kernel_stats(a.kernel_stats, PROFILE_STEPS + 2)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
