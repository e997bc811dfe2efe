#!/usr/bin/env python3
"""MS-SSIM + PSNR (dc_vic_amd.metrics.ms_ssim_psnr, csrc/ssim.hip) on one MI355X -> profiles/ssim_bench.json.

    python tools/ssim_bench.py [--out profiles/ssim_bench.json] [--kernel-stats DIR_768x512_N1 DIR_2048x1365_N8]
    rocprofv3 --kernel-trace --stats -d DIR -o ssim --output-format csv -- python tools/ssim_bench.py --profile H W N

Time per pair from device events after warm-up at 768x512 and 2048x1365, N = 1 and 8; the kernel-time split of a separate rocprofv3
run per shape (--profile; --kernel-stats reads its *kernel_stats.csv); the bytes the scale-0 stats kernel must read (x and y once,
fp32) over its kernel time; and, for comparison, the fp32 CPU restatement of pytorch-msssim + calc_psnr on 16 threads.
Inputs: a smooth random image and a noisy copy (seeded)."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(512, 768), (1365, 2048)]          # H, W: Kodak 768x512 and a 2048x1365 photo
BATCHES = [1, 8]


def pair(N, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand((N, 3, H // 8 + 1, W // 8 + 1), generator=g) * 2 - 1, size=(H, W), mode="bilinear", align_corners=False)
    return base.clamp(-1, 1), (base + 0.08 * torch.randn((N, 3, H, W), generator=g)).clamp(-1, 1)


def cpu_fp32(x, y):
    """pytorch-msssim 0.2.1 ms_ssim + calc_psnr in fp32 on the CPU (what the reference runs after a device-to-host copy)."""
    X, Y = ((x + 1.0) / 2.0 * 255.0).int().float(), ((y + 1.0) / 2.0 * 255.0).int().float()
    c = torch.arange(11).float() - 5
    g = torch.exp(-(c ** 2) / 4.5)
    g /= g.sum()
    C = X.shape[1]
    wh, ww = g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), g.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    flt = lambda t: F.conv2d(F.conv2d(t, wh, groups=C), ww, groups=C)      # noqa: E731
    wts = torch.tensor([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
    mcs = []
    for i in range(5):
        m1, m2 = flt(X), flt(Y)
        s1, s2, s12 = flt(X * X) - m1 * m1, flt(Y * Y) - m2 * m2, flt(X * Y) - m1 * m2
        cs_map = (2 * s12 + 58.5225) / (s1 + s2 + 58.5225)
        ss = ((2 * m1 * m2 + 6.5025) / (m1 * m1 + m2 * m2 + 6.5025) * cs_map).flatten(2).mean(-1)
        if i < 4:
            mcs.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    ms = torch.prod(torch.stack(mcs + [torch.relu(ss)]) ** wts.view(-1, 1, 1), dim=0).mean(1)
    a, b = ((x + 1.0) / 2.0 * 255.0).int().float(), ((y + 1.0) / 2.0 * 255.0).int().float()
    psnr = 10.0 * torch.log10(65025.0 / ((a - b) ** 2).flatten(1).mean(1))
    return ms, psnr


def kernel_stats(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    rows = list(csv.DictReader(open(files[0])))
    out = {}
    for r in rows:
        if "msssim" not in r["Name"]:
            continue
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        out[name] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "total_us": float(r["TotalDurationNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    ap.add_argument("--profile", type=int, nargs=3, default=None, metavar=("H", "W", "N"))
    ap.add_argument("--kernel-stats", nargs=2, default=None, metavar=("DIR_768x512_N1", "DIR_2048x1365_N8"))
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ssim_bench needs the GPU"
    from dc_vic_amd.metrics import ms_ssim_psnr
    if a.profile:
        H, W, N = a.profile
        x, y = [t.cuda().contiguous() for t in pair(N, H, W)]
        for _ in range(20):
            ms_ssim_psnr(x, y)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "timing": [], "note": "time per pair = device-event time of one ms_ssim_psnr call "
           f"(10 launches + 3 small torch allocations) / N, mean of {a.iters} calls after 20 warm-up calls"}
    for H, W in SHAPES:
        for N in BATCHES:
            x, y = [t.cuda().contiguous() for t in pair(N, H, W)]
            for _ in range(20):
                ms_ssim_psnr(x, y)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                ms_ssim_psnr(x, y)
            e1.record()
            torch.cuda.synchronize()
            call_us = e0.elapsed_time(e1) * 1e3 / a.iters
            res["timing"].append({"H": H, "W": W, "N": N, "us_per_call": round(call_us, 2), "us_per_pair": round(call_us / N, 2)})
            print(res["timing"][-1], flush=True)
    torch.set_num_threads(16)
    cpu = []
    for H, W in SHAPES:
        x, y = pair(1, H, W)
        cpu_fp32(x, y)
        t0 = time.perf_counter()
        for _ in range(3):
            cpu_fp32(x, y)
        cpu.append({"H": H, "W": W, "N": 1, "ms_per_pair": round((time.perf_counter() - t0) / 3 * 1e3, 2)})
        print(cpu[-1], flush=True)
    res["cpu_fp32_16_threads"] = cpu
    if a.kernel_stats:
        for (H, W, N), d in zip(((512, 768, 1), (1365, 2048, 8)), a.kernel_stats):
            ks = kernel_stats(d)
            if ks is None:
                continue
            ent = {"H": H, "W": W, "N": N, "kernels": ks}
            st0 = ks.get("msssim_stats_kernel<true>")
            if st0:
                nbytes = 2 * N * 3 * H * W * 4
                ent["stats_scale0_bytes"] = nbytes
                ent["stats_scale0_GBps"] = round(nbytes / (st0["avg_us"] * 1e-6) / 1e9, 1)
            ent["kernel_us_per_call"] = round(sum(v["total_us"] for v in ks.values()) / 20, 2)
            res.setdefault("kernel_split", []).append(ent)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
