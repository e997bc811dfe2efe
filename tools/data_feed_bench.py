#!/usr/bin/env python3
"""The training data feed (dc_vic_amd/train/data.py, csrc/data.hip) on generated folders -- nothing can be downloaded, so the images
are made from a seed: smooth content plus noise, --count files of 1024x768 JPEG quality 90 and --count_png of 2048x1365 PNG.

Part 1, one process, the modes alternating over --rounds rounds, a host clock around --batches batches of --batch that end in a
device synchronise, images/s:
  crop_dataset     scripts/train.py's CropDataset.batch (the path before the feed), then .to(device)
  host_feed        HostFeed.batch (--data_workers 0), then .to(device)
  train_feed       TrainFeed.batch, resize off
  train_feed_rs    TrainFeed.batch, resize_range [0.5, 1.0] bicubic
each on the JPEG folder and on the PNG folder; and the launch alone (dcvic_u8_resample_crop_f32 on one packed batch of 8, resize off
and on), device events around --iters calls.
Part 2 (--step), scripts/train.py's stage-3 step rate with synthetic weights and --batch 8, the modes alternating over --rounds rounds
of --steps iterations, each a child process (samples/s between the 10th and the last iteration, from the CLI's cumulative log
lines, so the first steps' set-up is left out for every mode alike):
  real             this tree on the JPEG folder
  parent           --parent_tree DIR (a checkout of the parent commit with a built library) on the same folder; skipped without it
  synthetic        this tree with --synthetic_data
python tools/data_feed_bench.py [--dir DIR] [--count 64 --count_png 8] [--batch 8 --batches 12 --rounds 3] [--iters 200]
                                [--step --steps 50 --parent_tree DIR] [--out profiles/data_feed_bench.json]"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = os.path.join("config", "dc_vic_synthetic.yaml")


def make_folder(root, count, H, W, ext, seed):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for i in range(count):
        p = os.path.join(root, f"{i:04d}.{ext}")
        if os.path.exists(p):
            continue
        f = rng.uniform(0.002, 0.02, size=(3, 2))
        ph = rng.uniform(0, 6.28, size=(3, 2))
        a = np.stack([127.5 + 90 * np.sin(f[c, 0] * x + ph[c, 0]) * np.cos(f[c, 1] * y + ph[c, 1]) for c in range(3)], axis=2)
        a = np.clip(a + rng.normal(0, 6, size=a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(p, **({"quality": 90} if ext == "jpg" else {}))
    return root


def feed_part(a, folders):
    from dc_vic_amd.train import data as D
    spec = importlib.util.spec_from_file_location("dcvic_train_cli_bench", os.path.join(ROOT, "scripts", "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    dev = "cuda:0"
    res = {}
    for tag, root in folders.items():
        paths = D.list_train_images(root)
        n_batches = a.batches if tag == "jpeg" else max(2, a.batches // 4)
        make = {
            "crop_dataset": lambda: cli.CropDataset(root, 256, 0, 1, 0),
            "host_feed": lambda: D.HostFeed(paths, 256, 0, 1, 0),
            "train_feed": lambda: D.TrainFeed(paths, 256, 0, 1, 0, dev, workers=a.workers, depth=a.depth),
            "train_feed_rs": lambda: D.TrainFeed(paths, 256, 0, 1, 0, dev, workers=a.workers, depth=a.depth, resize_range=(0.5, 1.0)),
        }
        rates = {k: [] for k in make}
        for _ in range(a.rounds):
            for name, mk in make.items():
                f = mk()
                try:
                    f.batch(a.batch).to(dev)                 # warm-up: the first batch fills the pipeline
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n_batches):
                        f.batch(a.batch).to(dev)
                    torch.cuda.synchronize()
                    rates[name].append(round(n_batches * a.batch / (time.perf_counter() - t0), 1))
                finally:
                    if hasattr(f, "close"):
                        f.close()
        res[tag] = dict(images=len(paths), batches=n_batches, images_per_s=rates)
        print(tag, json.dumps(rates), flush=True)
    return res


def launch_part(a, root):
    from dc_vic_amd.train import data as D
    from dc_vic_amd.train import kernels as K
    paths = D.list_train_images(root)
    table = D.conversion_table().cuda()
    res = {}
    for tag, rr in (("resize_off", None), ("resize_0.5_1.0", (0.5, 1.0))):
        recs = D.CropPlanner(paths, 256, 0, 1, 0, resize_range=rr).take(a.batch)
        entries = []
        for r in recs:
            w = D.window(r, 256)
            entries.append((D.window_pixels_u8(r, w), w, r.flip))
        _, used = D.slab_layout([e[1] for e in entries], 256)
        buf = np.zeros(used, dtype=np.uint8)
        D.pack_batch(buf, entries, 256)
        slab = torch.from_numpy(buf).cuda()
        out = torch.empty((a.batch, 3, 256, 256), device="cuda")
        for _ in range(20):
            K.u8_resample_crop(slab, used, buf.ctypes.data, a.batch, 256, table, out)
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                K.u8_resample_crop(slab, used, buf.ctypes.data, a.batch, 256, table, out)
            e1.record()
            torch.cuda.synchronize()
            us.append(round(e0.elapsed_time(e1) * 1000 / a.iters, 2))
        res[tag] = dict(slab_bytes=used, us_per_launch=us)
        print("launch", tag, used, us, flush=True)
    return res


def step_part(a, root):
    base = ["--synthetic_weights", "--allow_synthetic_lpips", "--batch_size", str(a.batch), "--total_iter", str(a.steps), "--log_step", "10"]
    modes = {"real": (ROOT, ["--dataset_root", root]), "synthetic": (ROOT, ["--synthetic_data"])}
    if a.parent_tree:
        modes["parent"] = (os.path.abspath(a.parent_tree), ["--dataset_root", root])
    rates = {k: [] for k in modes}
    for _ in range(a.rounds):
        for name, (tree, extra) in modes.items():
            r = subprocess.run([sys.executable, os.path.join(tree, "scripts", "train.py"), CFG] + base + extra, cwd=tree, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: scripts/train.py failed\n{r.stderr[-2000:]}")
            # the CLI prints cumulative samples/s; the time of iteration k is batch * k / rate_k, and the rate after the 10th
            # iteration leaves the first steps' set-up (code objects, pinned slabs, allocator growth) out for every mode alike
            pts = [(int(ln.split("|")[0].split()[1]), float(ln.split("|")[1].split()[0])) for ln in r.stdout.splitlines() if ln.startswith("iter ")]
            (k0, r0), (k1, r1) = [pt for pt in pts if pt[0] >= 10][0], pts[-1]
            rates[name].append(round(a.batch * (k1 - k0) / (a.batch * k1 / r1 - a.batch * k0 / r0), 2))
            print("step", name, pts, rates[name][-1], flush=True)
    return dict(steps=a.steps, batch=a.batch, samples_per_s=rates, ms_per_step={k: [round(1000 * a.batch / v, 1) for v in vs] for k, vs in rates.items()})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dir", default=None, help="where the generated folders live (default: a temporary directory)")
    p.add_argument("--count", type=int, default=64)
    p.add_argument("--count_png", type=int, default=8)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--batches", type=int, default=12)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--workers", type=int, default=None)
    p.add_argument("--depth", type=int, default=2)
    p.add_argument("--step", action="store_true")
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--parent_tree", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_feed_bench.json"))
    a = p.parse_args()
    if a.rounds < 2:
        raise SystemExit("--rounds: at least two alternating rounds")
    assert torch.cuda.is_available(), "the benchmark needs a GPU"
    with tempfile.TemporaryDirectory() as tmp:
        base = a.dir or tmp
        folders = {"jpeg": make_folder(os.path.join(base, "jpeg_1024x768"), a.count, 768, 1024, "jpg", 0),
                   "png": make_folder(os.path.join(base, "png_2048x1365"), a.count_png, 1365, 2048, "png", 1)}
        from dc_vic_amd.io_pipeline import default_workers
        out = dict(device=torch.cuda.get_device_name(0), workers=a.workers or default_workers(), depth=a.depth, batch=a.batch, rounds=a.rounds,
                   feed=feed_part(a, folders), launch=launch_part(a, folders["jpeg"]))
        if a.step:
            out["step"] = step_part(a, folders["jpeg"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
