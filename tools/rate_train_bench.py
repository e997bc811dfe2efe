#!/usr/bin/env python3
"""The rate-term kernels (csrc/rate_train.hip: value + gradients in one pass) at the rate-distortion trainers' sizes, beside the eval
kernels of csrc/rate.hip for scale -- one process, the variants alternating, device events around synchronised batches of launches:
  gaussian_train_slices_us   six calls on (8, 32, 16, 16) slice views of 192-channel tensors, filling one dy   (per CALL)
  gaussian_train_192_us      one call on (8, 192, 16, 16)
  eb_train_us                dcvic_eb_rate_train_f32 on (8, 192, 4, 4): dz, the 58 x 192 raw-parameter gradients, bits, loss
  gaussian_eval_192_us, eb_eval_us   dcvic_gaussian_rate_f32 / dcvic_eb_rate_f32 (y_hat, lik, bits) at the same sizes
python tools/rate_train_bench.py [--n 8] [--iters 200 --rounds 5] [--out profiles/rate_train_bench.json]
Prints one JSON line and writes it to --out.  No speed figure is a goal: these calls are far below 1 % of a training step; what
matters is few launches, no host synchronisation and reproducible sums.  Times include the host launch cost."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=8)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_train_bench.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rate_train_bench: needs a GPU; a CPU run measures nothing")
    from dc_vic_amd import ops
    from dc_vic_amd.entropy import SteEntropyBottleneck, get_scale_table
    from dc_vic_amd.train import kernels as K
    dev = "cuda:0"
    N = a.n
    g = torch.Generator().manual_seed(0)
    y = (3 * torch.randn((N, 192, 16, 16), generator=g)).to(dev)
    sigma = torch.exp(torch.rand((N, 192, 16, 16), generator=g) * 5 - 3).to(dev)
    mu = y + 1.5 * sigma * torch.randn((N, 192, 16, 16), generator=g).to(dev)
    u = (torch.rand((N, 192, 16, 16), generator=g) - 0.5).to(dev)
    w = (torch.rand(N, generator=g) / (N * 65536)).to(dev)
    torch.manual_seed(0)
    eb = SteEntropyBottleneck(192).to(dev)
    z = (4 * torch.randn((N, 192, 4, 4), generator=g)).to(dev)
    uz = (torch.rand((N, 192, 4, 4), generator=g) - 0.5).to(dev)
    params, med = eb.raw_params(), eb.quantiles.data[:, 0, 1]
    grads = [torch.zeros_like(t) for t in params]
    table = get_scale_table().to(dev)
    new = lambda t: torch.empty_like(t)
    y_hat, dy, dmu, dsigma, lik = new(y), new(y), new(y), new(y), new(y)
    z_hat, dz, likz = new(z), new(z), new(z)
    bits, loss = torch.zeros(N, device=dev), torch.zeros(1, device=dev)

    def slices():
        for k in range(6):
            s = slice(32 * k, 32 * k + 32)
            K.gaussian_rate_train(y[:, s], mu[:, s], sigma[:, s], u[:, s], w, 1.0, y_hat=y_hat[:, s], bits=bits, loss=loss, dy=dy[:, s],
                                  dmu=dmu[:, s], dsigma=dsigma[:, s])

    fns = {
        "gaussian_train_slices_us": (slices, 6),
        "gaussian_train_192_us": (lambda: K.gaussian_rate_train(y, mu, sigma, u, w, 1.0, y_hat=y_hat, bits=bits, loss=loss, dy=dy, dmu=dmu, dsigma=dsigma), 1),
        "eb_train_us": (lambda: K.eb_rate_train(z, uz, params, med, w, 1.0, z_hat=z_hat, bits=bits, loss=loss, dz=dz, grads=grads), 1),
        "gaussian_eval_192_us": (lambda: ops.gaussian_rate(y, None, mu, sigma, table, y_hat, None, None, lik, bits), 1),
        "eb_eval_us": (lambda: ops.eb_rate(z, eb.packs(), z_hat, None, likz, bits), 1),
    }

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / (a.iters * calls)          # microseconds per call

    for _ in range(20):
        for fn, _c in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, (fn, calls) in fns.items():
            t[k].append(timed(fn, calls))
    # reproducible sums: two runs of the value + gradient calls from zeroed accumulators give the same bits
    def once():
        bits.zero_(), loss.zero_()
        for gr in grads:
            gr.zero_()
        slices()
        fns["eb_train_us"][0]()
        return [bits.clone(), loss.clone(), dy.clone(), dz.clone()] + [gr.clone() for gr in grads]
    same = all(torch.equal(p_, q_) for p_, q_ in zip(once(), once()))
    res = {"tool": "rate_train_bench", "device": torch.cuda.get_device_name(0), "n": N, "iters": a.iters, "rounds": a.rounds, **t,
           **{k + "_min": min(v) for k, v in t.items()}, "two_runs_bit_equal": same,
           "launches_per_call": {"gaussian_train": 2, "eb_train": 3, "gaussian_eval": 2, "eb_eval": 1},
           "note": "device events around back-to-back launches incl. host launch cost; slices: per call of the six"}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
