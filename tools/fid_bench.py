"""HiFiC patch FID throughput (dc_vic_amd.fid) with synthetic FID-Inception weights at batch 100: patches/s, the FLOP per patch from the
layer shapes, the achieved convolution rate, the per-layer rates (event-timed, in a run of their own), the end-to-end time of a few
CLIC-sized (2048 x 1365) image pairs scaled per patch, and a plain-torch fp32 CPU forward of a few patches for scale.  Prints one JSON
document; `--out` also writes it to a file.  `--kernel-stats CSV` folds a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of a
`--profile-only` run (a few batches, nothing else) into the document as the kernel-time split.

    python tools/fid_bench.py [--out profiles/fid_bench.json] [--reps 5] [--no-cpu] [--kernel-stats kernel_stats.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fid -- python tools/fid_bench.py --profile-only
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch

from dc_vic_amd import fid, ops

CLIC_HW = (1365, 2048)


def timeit(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def shape_class(kh, kw, stride):
    if stride == 2:
        return "strided"
    if (kh, kw) == (1, 1):
        return "1x1"
    if (kh, kw) in ((1, 7), (7, 1), (1, 3), (3, 1)):
        return "1xk/kx1"
    return f"{kh}x{kw}"


def kernel_split(path):
    """rocprofv3 kernel_stats.csv -> {class: {ms, pct}} with classes conv / pools / resize / statistics / other."""
    out = {}
    tot = 0.0
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            if "patch_resize" in name:
                k = "resize"
            elif "pool3" in name or "mean_hw" in name:
                k = "pools"
            elif "gram" in name or "colsum" in name:
                k = "statistics"
            elif "conv" in name or "wino" in name:
                k = "conv"
            else:
                k = "other"
            d = out.setdefault(k, {"ms": 0.0, "kernels": {}})
            d["ms"] += ns * 1e-6
            d["kernels"][name[:120]] = round(ns * 1e-6, 3)
            tot += ns
    for d in out.values():
        d["pct"] = 100.0 * d["ms"] / (tot * 1e-6) if tot else 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=3, help="CLIC-sized synthetic image pairs of the end-to-end run")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--profile-only", action="store_true", help="run 3 full batches (patches -> features -> statistics) and exit")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model = fid.FIDInception.synthetic(0).to(dev)
    B = a.batch
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, CLIC_HW + (3,), dtype=np.uint8)).to(dev)
    from calc_metrics import hific_patch_origins
    org = hific_patch_origins(*CLIC_HW, 256)
    # one batch of B patches of the CLIC-sized image (its 68 patch origins, cycled)
    o = torch.from_numpy(fid.check_origins(np.resize(org, (B, 2)), *CLIC_HW, 256, 256)).to(dev)
    Bp = len(o)
    x = torch.empty((Bp, 3, fid.INCEPTION_SIZE, fid.INCEPTION_SIZE), device=dev)
    st = fid.FIDStats(dev)

    def batch():
        fid.patch_inputs(img, o, 256, out=x)
        st.add(model.features(x))

    if a.profile_only:
        for _ in range(3):
            batch()
        torch.cuda.synchronize()
        print(f"[fid_bench] profiled 3 batches of {Bp} patches")
        return

    shapes = fid.conv_layer_shapes()
    flop = sum(2.0 * ci * co * kh * kw * ho * ho for _, ci, co, kh, kw, s, h, ho in shapes)
    res = {"device": torch.cuda.get_device_name(dev), "batch": Bp, "reps": a.reps, "flop_per_patch": flop, "convs": len(shapes)}
    t_batch = timeit(batch, a.reps)
    t_feat = timeit(lambda: model.features(x), a.reps)
    t_resize = timeit(lambda: fid.patch_inputs(img, o, 256, out=x), a.reps * 4)
    f = model.features(x)
    t_stats = timeit(lambda: st.add(f), a.reps * 4)
    res.update({"patches_per_s": Bp / t_batch, "ms_per_1000_patches": t_batch / Bp * 1e6, "ms_per_batch": t_batch * 1e3,
                "features_ms_per_batch": t_feat * 1e3, "resize_ms_per_batch": t_resize * 1e3, "stats_ms_per_batch": t_stats * 1e3,
                "network_TFLOPs": flop * Bp / t_feat / 1e12})

    # per-layer rates: event-timed launches (a run of its own: the events serialise the launches)
    model.features(x); torch.cuda.synchronize()
    ops.kernel_events_start()
    model.features(x)
    torch.cuda.synchronize()
    ops.kernel_events_stop()
    by_key = {}
    for (cfg, Cin, Cout, T, s, ups, H, W, N), (n, fl, t) in ops.LAST_SHAPE_STATS.items():
        by_key.setdefault((Cin, Cout, T, s, H), [0.0, 0.0])
        by_key[(Cin, Cout, T, s, H)][0] += fl
        by_key[(Cin, Cout, T, s, H)][1] += t
    layers, classes = [], {}
    conv_t = conv_fl = 0.0
    seen = set()
    for name, ci, co, kh, kw, s, h, ho in shapes:
        k = (ci, co, kh * kw, s, h)
        if k in seen or k not in by_key:
            continue
        seen.add(k)
        fl, t = by_key[k]
        conv_t += t; conv_fl += fl
        cls = shape_class(kh, kw, s)
        c = classes.setdefault(cls, {"ms": 0.0, "flop": 0.0})
        c["ms"] += t * 1e3; c["flop"] += fl
        layers.append({"layer": name, "Cin": ci, "Cout": co, "k": f"{kh}x{kw}", "stride": s, "H_in": h, "H_out": ho, "ms": t * 1e3,
                       "TFLOPs": fl / t / 1e12})
    for c in classes.values():
        c["TFLOPs"] = c["flop"] / (c["ms"] * 1e-3) / 1e12
        c["pct_of_conv_time"] = 100.0 * c["ms"] / (conv_t * 1e3)
    res["conv_event_timed"] = {"ms": conv_t * 1e3, "TFLOPs": conv_fl / conv_t / 1e12, "by_shape_class": classes}
    med = float(np.median([l["TFLOPs"] for l in layers]))
    res["conv_layers_median_TFLOPs"] = med
    res["conv_layers_below_third_of_median"] = sorted([l for l in layers if l["TFLOPs"] < med / 3], key=lambda l: l["TFLOPs"])
    res["conv_layers"] = layers

    # end to end: CLIC-sized pairs through calc_metrics' device path, scaled per patch
    imgs = [rng.integers(0, 256, CLIC_HW + (3,), dtype=np.uint8) for _ in range(a.pairs)]
    pf = fid.PatchFeatures(model, dev, B, 256)
    items = [(im, hific_patch_origins(*CLIC_HW, 256)) for im in imgs]
    pf.statistics(items[:1]).mu_sigma()
    t0 = time.perf_counter()
    s1, s2 = pf.statistics(items), pf.statistics(items)
    n = s1.n + s2.n
    (m1, c1), (m2, c2) = s1.mu_sigma(), s2.mu_sigma()
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    fid.frechet_distance(m1, c1, m2, c2)
    t_fd = time.perf_counter() - t0
    per_img = len(org)
    res["end_to_end"] = {"pairs": a.pairs, "patches": n, "patches_per_image": per_img,
                         "device_s_excluding_png_decode": t_dev, "device_ms_per_patch": t_dev / n * 1e3, "frechet_sqrtm_s": t_fd,
                         "clic2020_test_428_pairs_estimate_s": t_dev / n * 428 * 2 * per_img + t_fd,
                         "note": "PNG decoding is excluded (the synthetic images are in memory); calc_metrics overlaps it on 4 threads"}

    if not a.no_cpu:
        # the plain-torch restatement of tests/test_fid_host.py, run in fp32 on the CPU (the comparison point, not a product path)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_fid_host import ref_features, ref_inputs
        u8 = rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)
        xin = ref_inputs(u8).float()
        sd = fid.FIDInception.synthetic(0).state_dict()
        t0 = time.perf_counter()
        with torch.no_grad():
            ref_features(sd, xin, dtype=torch.float32)
        t_cpu = (time.perf_counter() - t0) / len(u8)
        res["cpu_fp32_s_per_patch"] = t_cpu
        res["cpu_threads"] = torch.get_num_threads()
        res["gpu_speedup_vs_cpu_fp32"] = t_cpu / (t_batch / Bp)
    if a.kernel_stats:
        res["kernel_split_rocprof"] = kernel_split(a.kernel_stats)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
