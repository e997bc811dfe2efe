#!/usr/bin/env python3
"""Selection of (beta_rate, beta_vq) per target bitrate -- the second caller of the batched rate / reconstruction path
(SURVEY 8f-4).  Same flags, loop and output files as the reference's scripts/beta_selection.py:30-246:

    positional config_path, --model_path --search_dir --save_dir --dataset_root --beta_vq ... --target_rate ...
    --alpha --batch_size --keep_recon -d/--device

For every target rate and every beta_vq it reads the best probe of `binary_rate_search.py`
(`<search_dir>/result_beta_vq_X_target_rate_Y.csv`, skipped when its bpp error exceeds 0.001, :175-183), reconstructs the
dataset with run_model(is_train=False) at that (beta_rate, beta_vq) (:119-155), writes the PNGs (truncating uint8, as
img_utils.imwrite), `_rate_summary.csv` and `_avg_bitrate.json` per setting, scores `alpha * PSNR - FID` (Eq. 13, :205) and
writes `target_rate_*/result.csv` (sorted by score) and `beta_selection_results.csv`.

FID needs pytorch-fid's Inception weights, which cannot be fetched offline: `--inception_path` names the file
(pt_inception-2015-12-05-6726825d.pth), and FID is then computed on the device as scripts/calc_metrics.py does (HiFiC patch FID,
dc_vic_amd.fid), with the real set's statistics computed once for all settings.  Without it, or under 50 images (where the
reference would fail), the `fid` column is NaN and the score falls back to `alpha * PSNR` (a message says so).  `--fid_csv` lets
an external FID tool supply `beta_vq,target_rate,fid` rows instead, and takes precedence.  `--synthetic_weights` replaces
--model_path by the deterministic synthetic weights.
Per-image bpp comes from the kernel-side per-image bit counts (`bits_per_image`), not from a second pass over the
likelihood maps (calc_batch_bpp :96-104 computes the same quantity).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import shutil
import sys
from glob import glob

import numpy as np
import pandas as pd
import torch

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.append(os.path.dirname(os.path.abspath(__file__)))
from binary_rate_search import batches  # noqa: E402
from calc_metrics import FID_MIN_IMAGES, average_psnr, fid_metric, fid_statistics  # noqa: E402
from dc_vic_amd import BaseConfig, build_comp_model, ops  # noqa: E402
from dc_vic_amd.io_pipeline import AsyncWriter, encode_png_u8  # noqa: E402
from dc_vic_amd.selection_set import SelectionSet  # noqa: E402

SEARCH_ERROR_THRESHOLD = 0.001


def arg_parse() -> dict:
    p = argparse.ArgumentParser()
    p.add_argument("config_path", type=str)
    p.add_argument("--model_path", type=str)
    p.add_argument("--search_dir", type=str)
    p.add_argument("--save_dir", type=str)
    p.add_argument("--dataset_root", type=str)
    p.add_argument("--beta_vq", type=float, nargs="+")
    p.add_argument("--target_rate", type=float, nargs="+")
    p.add_argument("--alpha", type=float, default=2.0, help="score = alpha * PSNR - FID (Eq. 13 of the paper)")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--keep_recon", action="store_true")
    p.add_argument("-d", "--device", type=str, default="cuda:0")
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--fid_csv", type=str, default=None, help="optional csv (beta_vq,target_rate,fid) from an external FID tool")
    p.add_argument("--inception_path", type=str, default=None,
                   help="pytorch-fid's FID Inception state dict (pt_inception-2015-12-05-6726825d.pth) to compute FID on the device")
    return vars(p.parse_args())


@torch.no_grad()
def save_reconstructions(model, items, names, bs, save_dir, beta_vq, beta_rate) -> float:
    """beta_selection.py:119-155: run_model on every batch, write <name>.png + the per-image rate table.  `items`: the list of
    load_dataset, or a SelectionSet (the same batches, from device memory where the folder allows)."""
    rows = []
    writer = AsyncWriter()
    k = 0
    try:
        for x, idx in (items.batches(bs) if isinstance(items, SelectionSet) else batches(items, bs)):
            N, _, H, W = x.shape
            out = model.run_model(real_images=x, vq_indices=idx, beta_vq=beta_vq, beta_rate=beta_rate, is_train=False)
            bits = out["bits_per_image"].double().cpu().numpy()
            _, u8 = ops.crop_clamp(out["fake_images"], H, W, want_u8=True)      # truncating uint8, img_utils.py:19-44
            u8 = u8.cpu().numpy()
            for i in range(N):
                name = names[k]; k += 1
                writer.submit(encode_png_u8, os.path.join(save_dir, name), u8[i].copy())
                rows.append({"img_name": name.split(".")[0], "num_pixel": H * W, "total_bit": float(bits[i]), "bitrate": float(bits[i]) / (H * W)})
    finally:
        writer.close()
    df = pd.json_normalize(rows)
    df.to_csv(os.path.join(save_dir, "_rate_summary.csv"))
    avg_bpp = float(df["bitrate"].mean())
    with open(os.path.join(save_dir, "_avg_bitrate.json"), "w") as f:
        json.dump({"avg_bpp": avg_bpp}, f)
    return avg_bpp


def try_fid(real_paths, fake_paths, device, inception=None, real_stats=None):
    """calc_metrics.py:220-320 (HiFiC-style patch FID) on the device (scripts/calc_metrics.fid_metric); None without
    --inception_path, or under 50 images (with the reference's message).  `real_stats`: a dict that caches the real set's (mu, sigma)
    per list of real images, so it is computed once for every (target_rate, beta_vq) setting."""
    if inception is None or len(real_paths) < FID_MIN_IMAGES:
        if inception is not None:
            print(f"[beta_selection] num_img (={len(real_paths)}) is too small to calc FID", file=sys.stderr)
        return None
    key = tuple(real_paths)
    if real_stats is not None and key not in real_stats:
        real_stats[key] = fid_statistics(inception, real_paths, device)
        print(f"[beta_selection] FID: statistics of the {len(real_paths)} real images computed", flush=True)
    return fid_metric(inception, real_paths, fake_paths, device, real_stats=None if real_stats is None else real_stats[key])


def main() -> None:
    a = arg_parse()
    opt = BaseConfig.fromfile(a["config_path"], {k: v for k, v in a.items() if k not in ("synthetic_weights", "fid_csv", "inception_path")})
    ck = opt["subnet"]["vq_model"].get("ckpt_path")
    if ck and not os.path.exists(ck):
        opt["subnet"]["vq_model"]["ckpt_path"] = None
    inception = None
    if a["inception_path"]:                       # checked before any image is read or reconstructed
        from dc_vic_amd.fid import FIDInception
        inception = FIDInception.from_file(a["inception_path"])
    os.makedirs(a["save_dir"], exist_ok=True)
    assert os.path.exists(a["dataset_root"]), f'dataset_root "{a["dataset_root"]}" does not exist.'
    model = build_comp_model(opt)
    items = SelectionSet(a["dataset_root"], model.device, opt["subnet"]["vq_model"]["n_embed"])
    names = items.names
    assert len(items), f'dataset_root "{a["dataset_root"]}" holds no png'
    if a["synthetic_weights"]:
        from dc_vic_amd.synth import load_synth_weights
        load_synth_weights(model, 1234)
    else:
        model.load_learned_weight(ckpt_path=a["model_path"])
    ext_fid = {}
    if a["fid_csv"]:
        for _, r in pd.read_csv(a["fid_csv"]).iterrows():
            ext_fid[(round(float(r["beta_vq"]), 4), round(float(r["target_rate"]), 4))] = float(r["fid"])

    selection = []
    warned = False
    real_stats = {}
    for target_rate in a["target_rate"]:
        data = []
        save_dir = os.path.join(a["save_dir"], f"target_rate_{target_rate}")
        os.makedirs(save_dir, exist_ok=True)
        for beta_vq in a["beta_vq"]:
            csv = os.path.join(a["search_dir"], f"result_beta_vq_{beta_vq:.2f}_target_rate_{target_rate:.3f}.csv")
            best = pd.read_csv(csv).sort_values(by="diff").iloc[0]
            if best["diff"] > SEARCH_ERROR_THRESHOLD:
                print(f'[beta_selection] bpp difference is larger than threshold: {best["diff"]} > {SEARCH_ERROR_THRESHOLD}. Skip.', flush=True)
                continue
            beta_rate = float(best["beta_rate"])
            recon_dir = os.path.join(save_dir, f"beta_vq_{beta_vq:.2f}")
            os.makedirs(recon_dir, exist_ok=True)
            avg_bpp = save_reconstructions(model, items, names, a["batch_size"], recon_dir, beta_vq, beta_rate)
            fake = sorted(glob(os.path.join(recon_dir, "*.png")))
            real = sorted(glob(os.path.join(a["dataset_root"], "*.png")))
            psnr = average_psnr(real, fake)
            fid = ext_fid.get((round(beta_vq, 4), round(target_rate, 4)))
            if fid is None:
                fid = try_fid(real, fake, a["device"], inception, real_stats)
            if fid is None:
                if not warned:
                    print("[beta_selection] FID unavailable offline (Inception weights): score = alpha * PSNR; pass --fid_csv to add it", file=sys.stderr)
                    warned = True
                fid, score = float("nan"), a["alpha"] * psnr
            else:
                score = a["alpha"] * psnr - fid
            data.append({"beta_vq": beta_vq, "beta_rate": beta_rate, "bpp": avg_bpp, "psnr": psnr, "fid": fid, "score": score})
            if not a["keep_recon"]:
                shutil.rmtree(recon_dir)
        if not data:
            continue
        df = pd.json_normalize(data).sort_values(by="score", ascending=False)
        df.to_csv(os.path.join(save_dir, "result.csv"))
        b = df.iloc[0]
        print(f'target_rate: {target_rate}, selected beta_vq: {b["beta_vq"]}, selected beta_rate: {b["beta_rate"]}', flush=True)
        selection.append({"target_rate": target_rate, "selected_beta_vq": b["beta_vq"], "selected_beta_rate": b["beta_rate"]})
    pd.json_normalize(selection).to_csv(os.path.join(a["save_dir"], "beta_selection_results.csv"), index=False)


if __name__ == "__main__":
    main()
