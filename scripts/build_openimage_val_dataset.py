#!/usr/bin/env python3
"""Build the beta-selection set of stage 2 -- the first command of the stage, with the flags, crop plan and output of the reference's
scripts/build_openimage_val_dataset.py:

    --vqgan_type f8-n256 --openimage_root ROOT [--save_root ./dataset] [-d cuda:0] [-s 0] [-n 2000]

It cuts one random 256 x 256 crop from each of the first `num_img` eligible images of the shuffled, sorted
<openimage_root>/validation/*.jpg and writes, under <save_root>/vq_f8_n256/crop_256_<num_img>_seed_<seed>/, <name>.png with the crop
and <name>.npy with its VQGAN tokens, uint8 [32, 32], for scripts/binary_rate_search.py and scripts/beta_selection.py.

The tokens are `model.vq_encode(x)` of the model that --config_path builds, the codec's own tokenizer: a stored token is the token
run_model would compute from the stored PNG.  Crops go to the device as uint8 and are converted there (dcvic_u8_hwc_to_f32_nchw);
they are tokenised --batch_size at a time, and a crop's tokens do not depend on its batch.

Added flags: --config_path (the model YAML whose subnet.vq_model is built), --vqgan_ckpt (overrides subnet.vq_model.ckpt_path),
--synthetic_weights (the deterministic synthetic weights instead of a checkpoint), --batch_size, --io_workers.
Refused before any GPU work: a --vqgan_type that is not built or disagrees with the config, a missing validation folder or one without
.jpg, a missing VQGAN checkpoint without --synthetic_weights.  Fewer eligible images than --num_img: what there is is written, and a
line says so."""
from __future__ import annotations

import argparse
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from typing import List, Sequence, Tuple

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.append(ROOT)

PATCH = 256
SAVE_DIR_NAMES = {"f8-n256": "vq_f8_n256", "f16": "vq_f16", "f8": "vq_f8"}
BUILT_TYPES = {"f8-n256": dict(n_embed=256, embed_dim=4)}


def arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument("--vqgan_type", type=str, choices=["f8-n256", "f16", "f8"])
    p.add_argument("--openimage_root", type=str)
    p.add_argument("--save_root", type=str, default="./dataset")
    p.add_argument("-d", "--device", type=str, default="cuda:0")
    p.add_argument("-s", "--seed", type=int, default=0)
    p.add_argument("-n", "--num_img", type=int, default=2000)
    p.add_argument("--config_path", type=str, default=os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"),
                   help="the model YAML whose subnet.vq_model is built")
    p.add_argument("--vqgan_ckpt", type=str, default=None, help="overrides subnet.vq_model.ckpt_path")
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--io_workers", type=int, default=0, help="JPEG decode / PNG encode threads (0: min(8, the host cores))")
    return p


def plan_crops(paths: Sequence[str], sizes: Sequence[Tuple[int, int]], seed: int, num_img: int, patch: int = PATCH) -> List[Tuple[str, int, int]]:
    """[(path, top, left)] of the reference's loop.  `paths` sorted, `sizes` their (w, h).  The list is shuffled by numpy's legacy
    generator seeded with `seed`; Python's generator, seeded with `seed`, draws top then left for every image whose shorter side
    reaches `patch` (an image below is skipped without a draw), until num_img crops are planned.  Pure: the global generators are
    left alone (RandomState(seed) and Random(seed) give the streams of np.random.seed(seed) and random.seed(seed))."""
    order = list(range(len(paths)))
    np.random.RandomState(seed).shuffle(order)        # a list's shuffle depends on its length alone
    rng = random.Random(seed)
    plan = []
    for i in order:
        if len(plan) >= num_img:
            break
        w, h = sizes[i]
        if min(w, h) < patch:
            continue
        top = rng.randint(0, h - patch)
        left = rng.randint(0, w - patch)
        plan.append((paths[i], top, left))
    return plan


def save_dir_of(save_root: str, vqgan_type: str, num_img: int, seed: int, patch: int = PATCH) -> str:
    return os.path.join(save_root, SAVE_DIR_NAMES[vqgan_type], f"crop_{patch}_{num_img}_seed_{seed}")


def check_vqgan_type(vqgan_type: str, opt) -> None:
    """SystemExit unless the type is built and agrees with the config's subnet.vq_model."""
    vq = opt["subnet"]["vq_model"]
    have = f"subnet.vq_model.n_embed {vq.get('n_embed')}, subnet.vq_model.embed_dim {vq.get('embed_dim')}"
    if vqgan_type not in BUILT_TYPES:
        raise SystemExit(f"--vqgan_type {vqgan_type} is not built: only f8-n256 (subnet.vq_model.n_embed 256, subnet.vq_model.embed_dim 4) is; the config has {have}")
    want = BUILT_TYPES[vqgan_type]
    if vq.get("n_embed") != want["n_embed"] or vq.get("embed_dim") != want["embed_dim"]:
        raise SystemExit(f"--vqgan_type {vqgan_type} means subnet.vq_model.n_embed {want['n_embed']} and subnet.vq_model.embed_dim {want['embed_dim']}, "
                         f"but the config has {have}")


def list_validation(openimage_root: str) -> List[str]:
    d = os.path.join(str(openimage_root), "validation")
    if not os.path.isdir(d):
        raise SystemExit(f"--openimage_root {openimage_root}: {d} is not a folder")
    paths = sorted(glob(os.path.join(d, "*.jpg")))
    if not paths:
        raise SystemExit(f"--openimage_root {openimage_root}: {d} holds no .jpg")
    return paths


def resolve_checkpoint(opt, vqgan_ckpt, synthetic_weights: bool) -> None:
    """Sets subnet.vq_model.ckpt_path to the file to load (None with --synthetic_weights), or SystemExit: random tokens select nothing."""
    vq = opt["subnet"]["vq_model"]
    if synthetic_weights:
        vq["ckpt_path"] = None
        return
    ck = vqgan_ckpt or vq.get("ckpt_path")
    if not ck or not os.path.exists(ck):
        raise SystemExit(f"VQGAN checkpoint {ck!r} (--vqgan_ckpt, else subnet.vq_model.ckpt_path) does not exist: tokens of a random VQGAN select "
                         "nothing; name the checkpoint, or pass --synthetic_weights")
    vq["ckpt_path"] = ck


def header_size(path: str) -> Tuple[int, int]:
    """(w, h) from the image header, without a decode."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def read_crop(path: str, top: int, left: int, patch: int = PATCH) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB").crop((left, top, left + patch, top + patch)), dtype=np.uint8).copy()


def main(argv=None) -> dict:
    """-> dict(save_dir, crops, device_seconds): what was written and the time spent on upload + convert + tokenise + download."""
    a = arg_parser().parse_args(argv)
    from dc_vic_amd import BaseConfig
    opt = BaseConfig.fromfile(a.config_path, {"device": a.device})
    if a.vqgan_type is None:
        raise SystemExit("--vqgan_type is required")
    check_vqgan_type(a.vqgan_type, opt)
    if a.batch_size < 1 or a.num_img < 1:
        raise SystemExit(f"--batch_size {a.batch_size}, --num_img {a.num_img}: both must be positive")
    paths = list_validation(a.openimage_root)
    resolve_checkpoint(opt, a.vqgan_ckpt, a.synthetic_weights)
    print(len(paths), "images")

    from dc_vic_amd.io_pipeline import AsyncWriter, default_workers, encode_png_u8
    workers = a.io_workers or default_workers()
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="dcvic-jpg") as pool:
        sizes = list(pool.map(header_size, paths))
        plan = plan_crops(paths, sizes, a.seed, a.num_img)
        if not plan:
            raise SystemExit(f"no image under {a.openimage_root}/validation has a shorter side of at least {PATCH}")
        if len(plan) < a.num_img:
            print(f"only {len(plan)} of the {len(paths)} images have a shorter side of at least {PATCH}: writing {len(plan)} crops, not {a.num_img}")
        save_dir = save_dir_of(a.save_root, a.vqgan_type, a.num_img, a.seed)
        os.makedirs(save_dir, exist_ok=True)
        print("Save to", save_dir)

        import torch
        from dc_vic_amd import build_comp_model, ops
        from dc_vic_amd.train.data import conversion_table
        device = a.device if a.device != "cuda" else f"cuda:{torch.cuda.current_device()}"
        torch.cuda.set_device(torch.device(device))
        model = build_comp_model(opt)
        if a.synthetic_weights:
            from dc_vic_amd.synth import load_synth_weights
            load_synth_weights(model, 1234)
        table = conversion_table().to(device)
        n_embed = BUILT_TYPES[a.vqgan_type]["n_embed"]

        chunks = [plan[i:i + a.batch_size] for i in range(0, len(plan), a.batch_size)]
        submit = lambda chunk: [pool.submit(read_crop, *item) for item in chunk]
        writer = AsyncWriter(workers)
        gpu_s = 0.0
        try:
            pending = submit(chunks[0])
            for k, chunk in enumerate(chunks):
                crops = [f.result() for f in pending]
                pending = submit(chunks[k + 1]) if k + 1 < len(chunks) else []          # decode ahead of the device
                t0 = time.perf_counter()
                u8 = torch.from_numpy(np.stack(crops)).to(device)
                with torch.no_grad():
                    _, idx = model.vq_encode(ops.u8_hwc_to_f32_nchw(u8, table))
                tok = idx.cpu().numpy()
                gpu_s += time.perf_counter() - t0
                if tok.min() < 0 or tok.max() >= n_embed:
                    raise RuntimeError(f"tokens outside [0, {n_embed}) from the VQGAN: [{tok.min()}, {tok.max()}]")
                tok = tok.astype(np.uint8)             # f8-n256 only: 256 codes fit a byte
                for (path, _, _), crop, t in zip(chunk, crops, tok):
                    out = os.path.join(save_dir, os.path.basename(path).replace(".jpg", ".png"))
                    writer.submit(encode_png_u8, out, crop)
                    writer.submit(np.save, out.replace(".png", ".npy"), t.copy())
        finally:
            writer.close()
    print(f"{len(plan)} crops written to {save_dir}; upload + convert + tokenise {len(plan) / max(gpu_s, 1e-9):.1f} images/s (decode and PNG encode excluded)")
    return dict(save_dir=save_dir, crops=len(plan), device_seconds=gpu_s)


if __name__ == "__main__":
    main()
