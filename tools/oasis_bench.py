#!/usr/bin/env python3
"""dcvic_oasis_ce_f32 (value + gradient + score in one pass) against the path it replaces -- dcvic_cross_entropy_f32 on shifted
targets + dcvic_reduce_loss_f32 + a torch mean over channels 1: -- at the OASIS trainer's shape, in one process, alternating,
device events around synchronised batches of launches.  python tools/oasis_bench.py [--n 8 --c 257 --hw 32] [--iters 200 --rounds 5]
Prints one JSON line.  Bytes: the logits read once and the gradient written once; at this size the figure mostly shows launch
and latency cost, not bandwidth."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=8)
    p.add_argument("--c", type=int, default=257)
    p.add_argument("--hw", type=int, default=32)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    a = p.parse_args()
    from dc_vic_amd.train import kernels as K
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    lg = (torch.randn((a.n, a.c, a.hw, a.hw), generator=g) * 2).to(dev)
    idx = torch.randint(0, a.c - 1, (a.n, a.hw, a.hw), generator=g).to(dev)
    scale = 0.5 / (a.n * a.hw * a.hw)

    def new():
        return K.oasis_ce(lg, idx, True, scale, want_grad=True, want_score=True)

    def old():
        nll, dl = K.cross_entropy(lg, idx + 1, scale, want_grad=True)
        return K.reduce_loss(3, nll, None, scale), dl, lg[:, 1:].mean()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters          # microseconds per call

    for _ in range(20):
        new(); old()
    t_new, t_old = [], []
    for _ in range(a.rounds):
        t_new.append(timed(new)); t_old.append(timed(old))
    nbytes = 2 * lg.numel() * 4 + idx.numel() * 8
    best = min(t_new)
    print(json.dumps({"shape": [a.n, a.c, a.hw, a.hw], "iters": a.iters, "oasis_ce_us": t_new, "replaced_path_us": t_old,
                      "oasis_ce_us_min": best, "replaced_path_us_min": min(t_old), "speedup_min_over_min": min(t_old) / best,
                      "bytes": nbytes, "GBps_at_min": nbytes / best * 1e-3,
                      "note": "per-call time of back-to-back launches incl. host launch cost; the replaced path allocates and launches 4-5 kernels"}),
          flush=True)


if __name__ == "__main__":
    main()
