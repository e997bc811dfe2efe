#!/usr/bin/env python3
"""Stage 2's data path with synthetic weights on generated images -- nothing can be downloaded, so --count JPEGs of 320 x 288 are made
from a seed and scripts/build_openimage_val_dataset.py cuts the 256 x 256 selection set from them (--batch 16).

  builder   images/s of the builder's device part (upload, dcvic_u8_hwc_to_f32_nchw, vq_encode, download), decode and PNG encode
            excluded; run twice, the first run pays the code-object loads
  probe     one binary_rate_search.run_one_search over the set at batch --batch, a host clock around the call (it ends in the copy of
            the bpp values), the paths alternating in one process over --rounds rounds, medians:
              host_images   the host list without tokens: the VQGAN encoder runs in every probe
              host_tokens   the host list with tokens, the yardstick: the parent commit's loader and uploads; its tokens go through
                            dcvic_vq_token_feat_f32 too, since vq_encode is rerouted for every caller
              set_tokens    the device-resident SelectionSet with tokens
  kernel_b  dcvic_vq_token_feat_f32 on uint8 tokens (16, 32, 32), D = 4, n_e = 256, against the torch chain it replaces (long,
            embedding, permute, one_hot, cast, cat), device events around --iters calls
  kernel_a  dcvic_u8_hwc_to_f32_nchw on a resident uint8 batch (16, 256, 256, 3) against the upload of the uint8 batch plus the torch
            expression, and against the upload of the fp32 host batch (what a probe of the host list pays), a host clock around
            --iters calls that ends in a synchronise

python tools/stage2_bench.py [--count 64 --batch 16 --rounds 5 --iters 200] [--out profiles/stage2_bench.json]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
CFG = os.path.join(ROOT, "config", "dc_vic_synthetic.yaml")
DEV = "cuda:0"


def make_jpegs(root, count, H=288, W=320):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for i in range(count):
        f, ph = rng.uniform(0.002, 0.05, size=(3, 2)), rng.uniform(0, 6.28, size=(3, 2))
        a = np.stack([127.5 + 90 * np.sin(f[c, 0] * x + ph[c, 0]) * np.cos(f[c, 1] * y + ph[c, 1]) for c in range(3)], axis=2)
        Image.fromarray(np.clip(a + rng.normal(0, 6, size=a.shape), 0, 255).astype(np.uint8)).save(os.path.join(root, f"{i:04d}.jpg"), quality=90)


def events(fn, iters, rounds=3):
    for _ in range(20):
        fn()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(round(e0.elapsed_time(e1) * 1000 / iters, 2))
    return us


def clocked(fn, iters, rounds=3):
    for _ in range(5):
        fn()
    us = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        us.append(round((time.perf_counter() - t0) * 1e6 / iters, 2))
    return us


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--count", type=int, default=64)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage2_bench.json"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a GPU"
    import binary_rate_search as brs
    import build_openimage_val_dataset as B
    from dc_vic_amd import BaseConfig, build_comp_model, ops
    from dc_vic_amd.io_pipeline import u8_to_model_range
    from dc_vic_amd.selection_set import SelectionSet
    from dc_vic_amd.synth import load_synth_weights
    from dc_vic_amd.train.data import conversion_table

    out = dict(device=torch.cuda.get_device_name(0), count=a.count, batch=a.batch, rounds=a.rounds, iters=a.iters)
    with tempfile.TemporaryDirectory() as tmp:
        make_jpegs(os.path.join(tmp, "oi", "validation"), a.count)
        runs = []
        for k in range(2):
            r = B.main(["--vqgan_type", "f8-n256", "--openimage_root", os.path.join(tmp, "oi"), "--save_root", os.path.join(tmp, f"dataset{k}"),
                        "-n", str(a.count), "--batch_size", str(a.batch), "--synthetic_weights", "-d", DEV])
            runs.append(round(r["crops"] / r["device_seconds"], 1))
        out["builder"] = dict(images_per_s=runs, crops=r["crops"])
        folder = r["save_dir"]
        bare = os.path.join(tmp, "bare")
        os.makedirs(bare)
        for n in os.listdir(folder):
            if n.endswith(".png"):
                shutil.copy(os.path.join(folder, n), os.path.join(bare, n))

        model = build_comp_model(BaseConfig.fromfile(CFG, {"device": DEV}))
        load_synth_weights(model, 1234)
        paths = {"host_images": brs.load_dataset(bare), "host_tokens": brs.load_dataset(folder), "set_tokens": SelectionSet(folder, DEV, 256)}
        assert paths["set_tokens"].resident
        secs = {k: [] for k in paths}
        bpp = {}
        for rnd in range(a.rounds + 1):                         # round 0 warms every path up and is left out
            for name, items in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bpp[name] = brs.run_one_search(model, items, a.batch, 1.5, 3.0)
                dt = time.perf_counter() - t0
                if rnd:
                    secs[name].append(round(dt, 4))
        out["probe"] = dict(seconds=secs, median_seconds={k: statistics.median(v) for k, v in secs.items()}, avg_bpp=bpp,
                            same_float=len(set(bpp.values())) == 1)
        print("probe", json.dumps(out["probe"]), flush=True)

    cb = model.vq_model.quantize.embedding.weight
    tok = torch.randint(0, 256, (16, 32, 32), dtype=torch.uint8, device=DEV)

    def chain():
        idx = tok.long()
        zq = model.vq_indices_to_latent(idx)
        return zq, idx, model._index_feat(zq, idx)
    with torch.no_grad():
        assert all(torch.equal(g, r) for g, r in zip(ops.vq_token_feat(tok, cb, want_feat=True), (chain()[1], chain()[0], chain()[2])))
        out["kernel_b"] = dict(shape=[16, 32, 32], D=4, n_e=256, us_per_call=dict(kernel=events(lambda: ops.vq_token_feat(tok, cb, want_feat=True), a.iters),
                                                                                 torch_chain=events(chain, a.iters)))
    print("kernel_b", json.dumps(out["kernel_b"]), flush=True)

    u8_host = torch.randint(0, 256, (16, 256, 256, 3), dtype=torch.uint8)
    f32_host = u8_to_model_range(u8_host).contiguous()
    u8_dev, table = u8_host.to(DEV), conversion_table().to(DEV)
    assert torch.equal(ops.u8_hwc_to_f32_nchw(u8_dev, table).cpu(), f32_host)
    out["kernel_a"] = dict(shape=[16, 256, 256, 3], us_per_call=dict(
        kernel_on_resident_u8=clocked(lambda: ops.u8_hwc_to_f32_nchw(u8_dev, table), a.iters),
        upload_u8_plus_torch_expression=clocked(lambda: u8_to_model_range(u8_host.to(DEV)).contiguous(), a.iters),
        upload_f32=clocked(lambda: f32_host.to(DEV), a.iters)))
    print("kernel_a", json.dumps(out["kernel_a"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
