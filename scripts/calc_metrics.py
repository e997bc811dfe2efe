#!/usr/bin/env python3
"""Distortion / rate summary of a decoded directory -- the offline-computable part of the reference's
scripts/calc_metrics.py (121-171, 322-365).

Same flags (--real_dir --fake_dir -d/--device) and the same output file `<fake_dir>/_metrics.json`:
  * "bpp"  : read from `<fake_dir>/_avg_bitrate.json`, which scripts/compress.py wrote (calc_metrics.py:322-327);
  * "PSNR" : image-averaged PSNR over the sorted, name-matched *.png pairs, on RGB float32 in [0, 255]:
             20 log10(255) - 10 log10(mean squared error)  (calc_metrics.py:121-171), threads over images.
  * "FID"  : with --inception_path (pytorch-fid's pt_inception-2015-12-05-6726825d.pth): HiFiC patch FID (calc_metrics.py:220-320) --
             the 256 x 256 patches of `crop_hific_fid_patches` of both sets through FID-Inception (pool3, 2048-d) in batches of 100,
             FID(fake, real) as calculate_fid_given_paths([fake, real]) -- computed by dc_vic_amd.fid on the device -d: patches are
             cut and resized from each image uploaded once, and the fp64 feature statistics stay on the device.  Under 50 image pairs
             FID is left out with the reference's message.
  * "LPIPS": with --lpips_path (a state dict of lpips.LPIPS(net='alex'), as scripts/train.py takes): LPIPS(fake, real) per image
             on RGB in [-1, 1] (ToTensor, Normalize(.5, .5)), computed by dc_vic_amd.metrics on the device -d (calc_metrics.py:174-196);
  * "DISTS": with --dists_path (a complete DISTS() state dict, or DISTS_pytorch's weights.pt {alpha, beta} plus --vgg16_path,
             torchvision's VGG16 state dict): DISTS(fake, real) per image on RGB in [0, 1] (ToTensor) (calc_metrics.py:198-215).
  Both are image means of per-image values at full resolution; images are batched by shape, and a value does not depend on its batch.
  Weight files are loaded (torch.load weights_only=True) and checked before any image is read.  Parity with the pytorch_fid / lpips /
  DISTS_pytorch packages is unpinned (restated architectures; see dc_vic_amd/fid.py and dc_vic_amd/metrics.py).
A metric whose weights are not given is skipped with a message and absent from the json; without these flags nothing here touches
torch or the GPU.  The keys keep the reference's order: bpp, PSNR, FID, LPIPS, DISTS.  The HiFiC FID patch cropper is provided
(`crop_hific_fid_patches`, calc_metrics.py:307-320) for external FID tools; it and the device path share `hific_patch_origins`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from typing import Dict, List, Optional, Tuple

import numpy as np

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def get_real_fake_path_list(real_dir: str, fake_dir: str) -> Tuple[List[str], List[str]]:
    assert os.path.exists(real_dir), real_dir
    assert os.path.exists(fake_dir), fake_dir
    real = sorted(glob(os.path.join(real_dir, "*.png")))
    fake = sorted(glob(os.path.join(fake_dir, "*.png")))
    assert len(real) == len(fake), f"{len(real)} real vs {len(fake)} decoded images"
    for r, f in zip(real, fake):
        assert os.path.basename(r) == os.path.basename(f), (r, f)
    return real, fake


def read_img(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.float32)


def image_psnr(real_path: str, fake_path: str) -> Tuple[float, float, int]:
    a, b = read_img(real_path), read_img(fake_path)
    assert a.shape == b.shape, (real_path, a.shape, b.shape)
    sq = float(np.sum(np.square(b - a)))
    mse = sq / a.size
    return 20.0 * np.log10(255.0) - 10.0 * np.log10(mse), sq, a.size


def average_psnr(real_paths: List[str], fake_paths: List[str], workers: int = 8) -> float:
    """Mean of the per-image PSNRs (the reference reports the image average, not the pixel average)."""
    with ThreadPoolExecutor(max_workers=workers) as ex:
        vals = list(ex.map(lambda rf: image_psnr(*rf)[0], zip(real_paths, fake_paths)))
    return float(np.mean(vals))


def hific_patch_origins(H: int, W: int, patch_size: int) -> np.ndarray:
    """(y0, x0) of every HiFiC FID patch of an H x W image, in crop_hific_fid_patches' order (calc_metrics.py:307-320): the
    non-overlapping p x p blocks in row-major order, then those of the image shifted by p // 2 in both directions."""
    p = patch_size
    o = p // 2
    grids = []
    for s, h, w in ((0, H, W), (o, H - o, W - o)):
        ys, xs = np.meshgrid(s + p * np.arange(max(h, 0) // p), s + p * np.arange(max(w, 0) // p), indexing="ij")
        grids.append(np.stack([ys.ravel(), xs.ravel()], axis=1))
    return np.concatenate(grids, axis=0).astype(np.int64)


def crop_hific_fid_patches(img: np.ndarray, patch_size: int) -> np.ndarray:
    """All non-overlapping p x p blocks of the image, plus those of the image shifted by p/2 in both directions."""
    p = patch_size
    H, W = img.shape[:2]
    out = np.empty((0, p, p) + img.shape[2:], dtype=img.dtype)
    org = hific_patch_origins(H, W, p)
    return np.stack([img[y:y + p, x:x + p] for y, x in org]) if len(org) else out


def retrieve_bitrate(fake_dir: str) -> float:
    path = os.path.join(fake_dir, "_avg_bitrate.json")
    assert os.path.exists(path), f"{path} missing: run scripts/compress.py --decompress into this directory first"
    with open(path) as f:
        return json.load(f)["avg_bpp"]


# images per call: as many same-shape pairs as fit this many pixels, at most MAX_BATCH_IMAGES (at least one); x and y run as a batch of
# twice that.  Values do not depend on the batch (the kernels are batch-invariant), so these only bound memory and launch sizes.
MAX_BATCH_PIXELS = 1 << 22
MAX_BATCH_IMAGES = 16


def load_metric_models(lpips_path: Optional[str], dists_path: Optional[str], vgg16_path: Optional[str],
                       inception_path: Optional[str] = None) -> Dict[str, object]:
    """The networks of the metrics whose weights were given, on the host ({} without any: torch is not imported then)."""
    if vgg16_path and not dists_path:
        raise ValueError("--vgg16_path is only used by DISTS: give --dists_path (DISTS_pytorch's weights.pt) with it")
    models: Dict[str, object] = {}
    if inception_path:
        from dc_vic_amd.fid import FIDInception
        models["FID"] = FIDInception.from_file(inception_path)
    if lpips_path:
        import torch
        from dc_vic_amd.metrics import load_lpips
        models["LPIPS"] = load_lpips(torch.load(lpips_path, map_location="cpu", weights_only=True))
    if dists_path:
        from dc_vic_amd.metrics import DISTSVGG
        models["DISTS"] = DISTSVGG.from_files(vgg16_path=vgg16_path, dists_path=dists_path)
    return models


# HiFiC patch FID (calc_metrics.py:220-320): 256 x 256 patches, pytorch-fid batches of 100, at least 50 image pairs
FID_PATCH = 256
FID_BATCH_SIZE = 100
FID_MIN_IMAGES = 50


def read_u8(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def _prefetch(fn, items, depth: int = 4):
    """fn(item) for each item in order, up to `depth` ahead on worker threads (image decoding overlaps the device work)."""
    from collections import deque
    with ThreadPoolExecutor(max_workers=depth) as ex:
        q = deque()
        for it in items:
            q.append(ex.submit(fn, it))
            if len(q) > depth:
                yield q.popleft().result()
        while q:
            yield q.popleft().result()


def fid_statistics(model, paths: List[str], device: str, patch: int = FID_PATCH, batch: int = FID_BATCH_SIZE):
    """(mu, sigma) in fp64 of the pool3 features of every HiFiC patch of the images, computed on the device."""
    import torch
    from dc_vic_amd.fid import PatchFeatures
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    model.to(dev)

    def load(path):
        img = read_u8(path)
        return img, hific_patch_origins(img.shape[0], img.shape[1], patch)

    return PatchFeatures(model, dev, batch, patch).statistics(_prefetch(load, paths)).mu_sigma()


def fid_metric(model, real_paths: List[str], fake_paths: List[str], device: str, real_stats=None) -> Optional[float]:
    """FID(fake patches, real patches) as calculate_fid_given_paths([fake, real]) takes it; None (with the reference's message) under
    50 image pairs.  `real_stats`: the real set's (mu, sigma) when already computed."""
    from dc_vic_amd.fid import frechet_distance
    if len(real_paths) < FID_MIN_IMAGES:
        print(f"[calc_metrics] num_img (={len(real_paths)}) is too small to calc FID", file=sys.stderr)
        return None
    mu1, s1 = fid_statistics(model, fake_paths, device)
    mu2, s2 = real_stats if real_stats is not None else fid_statistics(model, real_paths, device)
    return frechet_distance(mu1, s1, mu2, s2)


def perceptual_metrics(models: Dict[str, object], real_paths: List[str], fake_paths: List[str], device: str) -> Dict[str, float]:
    """Image means of the per-image LPIPS / DISTS values, each computed as metric(fake, real) on the device."""
    import torch
    from PIL import Image
    from dc_vic_amd import metrics as M
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    for m in models.values():
        m.to(dev)
    buckets: Dict[Tuple[int, ...], List[int]] = {}
    for i, r in enumerate(real_paths):
        with Image.open(r) as im:
            buckets.setdefault((im.height, im.width), []).append(i)
    vals = {k: np.zeros(len(real_paths), dtype=np.float64) for k in models}
    for (H, W), idx in buckets.items():
        per = max(1, min(MAX_BATCH_IMAGES, MAX_BATCH_PIXELS // (H * W)))
        for b0 in range(0, len(idx), per):
            ids = idx[b0:b0 + per]
            real = np.stack([read_img(real_paths[i]) for i in ids])
            fake = np.stack([read_img(fake_paths[i]) for i in ids])
            assert real.shape == fake.shape, [fake_paths[i] for i in ids]
            # ToTensor: uint8 / 255 in fp32, HWC -> CHW
            r01 = np.ascontiguousarray((real / np.float32(255.0)).transpose(0, 3, 1, 2))
            f01 = np.ascontiguousarray((fake / np.float32(255.0)).transpose(0, 3, 1, 2))
            if "LPIPS" in models:                 # Normalize(.5, .5)
                fx = torch.from_numpy((f01 - np.float32(0.5)) / np.float32(0.5)).to(dev)
                rx = torch.from_numpy((r01 - np.float32(0.5)) / np.float32(0.5)).to(dev)
                vals["LPIPS"][ids] = M.lpips(models["LPIPS"], fx, rx).cpu().numpy()
            if "DISTS" in models:
                vals["DISTS"][ids] = M.dists(models["DISTS"], torch.from_numpy(f01).to(dev), torch.from_numpy(r01).to(dev)).cpu().numpy()
    return {k: float(np.mean(v)) for k, v in vals.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--real_dir", type=str, required=True)
    ap.add_argument("--fake_dir", type=str, required=True)
    ap.add_argument("-d", "--device", type=str, default="cuda:0")     # LPIPS / DISTS run here; PSNR runs on the host
    ap.add_argument("--lpips_path", type=str, default=None, help="state dict of lpips.LPIPS(net='alex') (torch.save'd; weights_only load)")
    ap.add_argument("--dists_path", type=str, default=None,
                    help="DISTS_pytorch weights.pt ({alpha, beta}; needs --vgg16_path) or a complete DISTS() state dict")
    ap.add_argument("--vgg16_path", type=str, default=None, help="torchvision VGG16 ImageNet state dict (features.*) for --dists_path")
    ap.add_argument("--inception_path", type=str, default=None,
                    help="pytorch-fid's FID Inception state dict (pt_inception-2015-12-05-6726825d.pth; weights_only load) for FID")
    a = ap.parse_args(argv)
    models = load_metric_models(a.lpips_path, a.dists_path, a.vgg16_path, a.inception_path)
    out = {"bpp": retrieve_bitrate(a.fake_dir)}
    real, fake = get_real_fake_path_list(a.real_dir, a.fake_dir)
    out["PSNR"] = average_psnr(real, fake)
    print(f"{len(real)} images: PSNR: {out['PSNR']:.4}")
    if "FID" in models:
        v = fid_metric(models["FID"], real, fake, a.device)
        if v is not None:
            out["FID"] = v
    perceptual = {k: m for k, m in models.items() if k != "FID"}
    if perceptual:
        out.update(perceptual_metrics(perceptual, real, fake, a.device))
    for name in ("FID", "LPIPS", "DISTS"):
        if name not in models:
            print(f"[calc_metrics] {name} skipped: its pretrained network weights cannot be fetched offline", file=sys.stderr)
    with open(os.path.join(a.fake_dir, "_metrics.json"), "w") as f:
        json.dump(out, f, indent=4)
    print(f"Results: {a.fake_dir}")
    for k, v in out.items():
        print(f"{k:>7}: {v:.4f}")
    return out


if __name__ == "__main__":
    main()
