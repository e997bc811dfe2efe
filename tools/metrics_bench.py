"""LPIPS / DISTS throughput (dc_vic_amd.metrics) at Kodak (512x768) and CLIC-sized (2048x1365) image pairs, the bandwidth of the L2 pool
and paired-moments kernels, and the plain-torch fp32 CPU restatement of one DISTS pair beside them.  Synthetic weights (the numbers
depend on the image size only).  Prints one JSON document; `--out` also writes it to a file.

    python tools/metrics_bench.py [--out profiles/metrics_bench.json] [--reps 5] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from dc_vic_amd import metrics as M

HBM_BPS = 8e12


def timeit(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def dists_cpu_fp32(m, x, y):
    """DISTS_pytorch's forward restated with torch CPU operators in fp32 (the comparison point, not a product path)."""
    def feats(t):
        h = (t - m.mean) / m.std
        out = [t]
        for pool, convs in m.stages():
            if pool is not None:
                h = torch.sqrt(F.conv2d(h * h, pool.filter, stride=2, padding=1, groups=h.shape[1]) + 1e-12)
            for c in convs:
                h = F.relu(F.conv2d(h, c.weight, c.bias, padding=1))
            out.append(h)
        return out
    fx, fy = feats(x), feats(y)
    w = m.alpha.sum() + m.beta.sum()
    a, b = torch.split(m.alpha / w, list(M.DISTS_CHNS), 1), torch.split(m.beta / w, list(M.DISTS_CHNS), 1)
    d = 0
    for k in range(6):
        mx, my = fx[k].mean([2, 3], keepdim=True), fy[k].mean([2, 3], keepdim=True)
        vx, vy = ((fx[k] - mx) ** 2).mean([2, 3], keepdim=True), ((fy[k] - my) ** 2).mean([2, 3], keepdim=True)
        cxy = (fx[k] * fy[k]).mean([2, 3], keepdim=True) - mx * my
        d = d + (a[k] * (2 * mx * my + 1e-6) / (mx ** 2 + my ** 2 + 1e-6)).sum(1) + (b[k] * (2 * cxy + 1e-6) / (vx + vy + 1e-6)).sum(1)
    return 1 - d.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dm = M.DISTSVGG.synthetic(0).to(dev)
    lm = M.load_lpips(None, seed=0).to(dev)
    g = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "metrics": {}, "kernels": {}}
    for H, W in ((512, 768), (2048, 1365)):
        x = torch.rand((1, 3, H, W), generator=g)
        y = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(0, 1)
        xd, yd = x.to(dev), y.to(dev)
        td = timeit(lambda: M.dists(dm, xd, yd), a.reps)
        tl = timeit(lambda: M.lpips(lm, xd * 2 - 1, yd * 2 - 1), a.reps)
        r = {"dists_pairs_per_s": 1 / td, "dists_ms_per_pair": td * 1e3, "lpips_pairs_per_s": 1 / tl, "lpips_ms_per_pair": tl * 1e3,
             "dists_value": float(M.dists(dm, xd, yd)[0]), "lpips_value": float(M.lpips(lm, xd * 2 - 1, yd * 2 - 1)[0])}
        # the two memory-bound kernels on this image's first (largest) tap: relu1_2 of the 2-image batch
        f = torch.rand((2, 64, H, W), generator=g).to(dev)
        tp = timeit(lambda: M.l2pool(f), a.reps * 4)
        pb = f.numel() * 4 + M.l2pool(f).numel() * 4
        tm = timeit(lambda: M.pair_moments(f[:1], f[1:]), a.reps * 4)
        mb = f.numel() * 4
        res["kernels"][f"{H}x{W}_relu1_2"] = {
            "l2pool_s": tp, "l2pool_GBps": pb / tp / 1e9, "l2pool_frac_of_8TBps": pb / tp / HBM_BPS,
            "pair_moments_s": tm, "pair_moments_GBps": mb / tm / 1e9, "pair_moments_frac_of_8TBps": mb / tm / HBM_BPS}
        if not a.no_cpu and H == 512:
            m32 = M.DISTSVGG.synthetic(0)
            t0 = time.perf_counter()
            with torch.no_grad():
                v = float(dists_cpu_fp32(m32, x, y)[0])
            r["cpu_fp32_dists_s_per_pair"] = time.perf_counter() - t0
            r["cpu_fp32_dists_value"] = v
            r["cpu_threads"] = torch.get_num_threads()
        res["metrics"][f"{H}x{W}"] = r
        del f
        torch.cuda.empty_cache()
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
