#!/usr/bin/env python3
"""The two batch-statistics calls (csrc/bn_train.hip: BatchNorm2d training forward and backward, each with the fused LeakyReLU) at the
discriminator's shapes, beside the same arithmetic written as torch ops on the device (per-channel mean / var, normalise, affine,
LeakyReLU, and the three backward sums and dx), which is what the tape would otherwise have to launch.  Device events around
`--iters` calls, the median over `--rounds` rounds; one JSON line per shape.

python tools/bn_bench.py [--iters 200 --rounds 5] [--out profiles/bn_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = ((8, 128, 64, 64), (8, 256, 32, 32), (8, 512, 31, 31))
EPS, MOM, ACT_LRELU = 1e-5, 0.1, 2


def timed(fn, iters, rounds):
    for _ in range(10):
        fn()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms), min(ms), max(ms)


def torch_fwd(x, gamma, beta, rm, rv):
    M = x.shape[0] * x.shape[2] * x.shape[3]
    var, mean = torch.var_mean(x, (0, 2, 3), unbiased=False)
    rstd = torch.rsqrt(var + EPS)
    rm.mul_(1 - MOM).add_(mean, alpha=MOM)
    rv.mul_(1 - MOM).add_(var, alpha=MOM * M / (M - 1))
    y = torch.nn.functional.leaky_relu((x - mean[None, :, None, None]) * (rstd * gamma)[None, :, None, None] + beta[None, :, None, None], 0.2)
    return y, mean, rstd


def torch_bwd(x, g, y, mean, rstd, gamma):
    M = x.shape[0] * x.shape[2] * x.shape[3]
    gp = torch.where(y > 0, g, 0.2 * g)
    xhat = (x - mean[None, :, None, None]) * rstd[None, :, None, None]
    dbeta, dgamma = gp.sum((0, 2, 3)), (gp * xhat).sum((0, 2, 3))
    dx = (gamma * rstd)[None, :, None, None] * (gp - dbeta[None, :, None, None] / M - xhat * dgamma[None, :, None, None] / M)
    return dx, dgamma, dbeta


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_bench: needs a GPU; a CPU run measures nothing")
    from dc_vic_amd.train import kernels as K
    dev = "cuda:0"
    rows = []
    for shape in SHAPES:
        g_ = torch.Generator().manual_seed(1)
        x, g = torch.randn(shape, generator=g_).to(dev), torch.randn(shape, generator=g_).to(dev)
        C = shape[1]
        gamma, beta = torch.rand(C, generator=g_).to(dev) + 0.5, torch.randn(C, generator=g_).to(dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        y, mean, rstd = K.bn_train_fwd(x, gamma, beta, rm, rv, MOM, EPS, ACT_LRELU)
        dx = torch.empty_like(x)
        mb = x.numel() * 4 / 1e6
        row = {"shape": list(shape), "tensor_MB": round(mb, 2), "iters": a.iters, "rounds": a.rounds}
        for name, fn, passes in (
                ("hip_fwd", lambda: K.bn_train_fwd(x, gamma, beta, rm, rv, MOM, EPS, ACT_LRELU, out=y), 3),          # read x twice, write y
                ("hip_bwd", lambda: K.bn_train_bwd(x, g, y, mean, rstd, gamma, dg, db, True, ACT_LRELU, dx=dx), 7),  # read x, g, y twice, write dx
                ("torch_fwd", lambda: torch_fwd(x, gamma, beta, rm, rv), None),
                ("torch_bwd", lambda: torch_bwd(x, g, y, mean, rstd, gamma), None)):
            med, lo, hi = timed(fn, a.iters, a.rounds)
            row[name + "_us"] = {"median": round(med * 1e3, 2), "min": round(lo * 1e3, 2), "max": round(hi * 1e3, 2)}
            if passes:
                row[name + "_GBps_at_minimum_traffic"] = round(passes * mb / 1e3 / (med / 1e3), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
