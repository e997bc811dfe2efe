"""Stage 2 end to end on a real MI355X, synthetic weights: scripts/build_openimage_val_dataset.py writes a selection set from five JPEGs,
and binary_rate_search.run_one_search and beta_selection.py read it through dc_vic_amd.selection_set.SelectionSet.

The builder's crops equal the planned crop of Pillow's decode, its tokens equal model.vq_encode of each crop run alone, and a probe
returns the SAME float from the device-resident set, from the host list with tokens and from the host list without them: the first
two differ in where the bytes come from only, and the last says that a stored token is the token the codec computes from the PNG."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import tokens_ref as R
from kernel_bounds import DEV

import build_openimage_val_dataset as B            # tokens_ref puts scripts/ on sys.path
import binary_rate_search as brs
from dc_vic_amd.selection_set import SelectionSet

pytestmark = pytest.mark.gpu
CONFIG = os.path.join(R.ROOT, "config", "dc_vic_synthetic.yaml")
SIZES = {"a.jpg": (300, 280), "b.jpg": (256, 400), "c.jpg": (200, 300), "d.jpg": (256, 256), "e.jpg": (512, 300)}      # (w, h)


@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(CONFIG, {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """The builder run once: -n 3 --batch_size 2 on the five JPEGs (a batch of 2 and a batch of 1).  -> (jpeg folder, output folder, plan)"""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("stage2")
    val = tmp / "oi" / "validation"
    val.mkdir(parents=True)
    for k, (name, (w, h)) in enumerate(SIZES.items()):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 3 + yy + 40 * k) % 256, (yy * 2 + xx // 3) % 256, (xx + yy * yy // 64) % 256], axis=-1).astype(np.uint8)
        img += np.random.default_rng(k).integers(0, 24, img.shape, dtype=np.uint8) // 2
        Image.fromarray(img, mode="RGB").save(val / name, quality=92)
    B.main(["--vqgan_type", "f8-n256", "--openimage_root", str(tmp / "oi"), "--save_root", str(tmp / "dataset"), "-n", "3", "--batch_size", "2",
            "--synthetic_weights", "-d", DEV])
    paths = sorted(str(val / n) for n in SIZES)
    plan = B.plan_crops(paths, [SIZES[os.path.basename(p)] for p in paths], 0, 3)
    return val, tmp / "dataset" / "vq_f8_n256" / "crop_256_3_seed_0", plan


def test_builder_output(built, model):
    from PIL import Image
    val, out, plan = built
    names = sorted(os.path.basename(p)[:-4] for p, _, _ in plan)
    assert len(plan) == 3 and "c" not in names                                   # 200 x 300: the shorter side is under 256
    assert sorted(os.listdir(out)) == sorted([n + ".npy" for n in names] + [n + ".png" for n in names])
    for path, top, left in plan:
        name = os.path.basename(path)[:-4]
        crop = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)[top:top + 256, left:left + 256]
        png = np.asarray(Image.open(out / f"{name}.png"))
        assert png.shape == (256, 256, 3) and png.dtype == np.uint8 and np.array_equal(png, crop), name
        tok = np.load(out / f"{name}.npy")
        assert tok.dtype == np.uint8 and tok.shape == (32, 32)
        with torch.no_grad():
            _, idx = model.vq_encode(R.table_expression(torch.from_numpy(crop.copy())[None]).to(DEV))
        assert np.array_equal(tok, idx[0].cpu().numpy()), f"{name}: the stored tokens differ from vq_encode of the crop run alone"


def test_probe_is_the_same_float_on_every_path(built, model, tmp_path):
    _, out, _ = built
    s = SelectionSet(str(out), DEV, 256)
    assert s.resident and s.tokens.dtype == torch.uint8 and s.images.device == torch.device(DEV) and tuple(s.images.shape) == (3, 256, 256, 3)
    parts = list(s.batches(2))
    assert [tuple(x.shape) for x, _ in parts] == [(2, 3, 256, 256), (1, 3, 256, 256)] and [tuple(t.shape) for _, t in parts] == [(2, 32, 32), (1, 32, 32)]
    items = brs.load_dataset(str(out))
    for (x, t), (xr, tr) in zip(parts, brs.batches(items, 2)):
        assert x.dtype == torch.float32 and torch.equal(x.cpu(), xr) and torch.equal(t.cpu().long(), tr)
    bare = tmp_path / "bare"
    bare.mkdir()
    for n in os.listdir(out):
        if n.endswith(".png"):
            shutil.copy(out / n, bare / n)
    no_tokens = brs.load_dataset(str(bare))
    assert all(t is None for _, t in no_tokens)
    s_bare = SelectionSet(str(bare), DEV, 256)
    assert s_bare.resident and s_bare.tokens is None
    for beta_rate, beta_vq in ((1.5, 3.0), (0.4, 1.0)):
        from_set = brs.run_one_search(model, s, 2, beta_rate, beta_vq)
        from_list = brs.run_one_search(model, items, 2, beta_rate, beta_vq)
        from_images = brs.run_one_search(model, no_tokens, 2, beta_rate, beta_vq)
        from_image_set = brs.run_one_search(model, s_bare, 2, beta_rate, beta_vq)
        print(f"beta_rate {beta_rate} beta_vq {beta_vq}: set {from_set!r} list {from_list!r} images {from_images!r} image set {from_image_set!r}")
        assert isinstance(from_set, float) and from_set > 0
        assert from_set == from_list, "the device-resident set and the host list with tokens disagree"
        assert from_images == from_list, "token-fed and image-fed probes disagree: a stored token is not the token the codec computes"
        assert from_image_set == from_images


def test_beta_selection_reads_the_set(built, tmp_path, monkeypatch):
    import pandas as pd
    import beta_selection
    _, out, plan = built
    sdir, sel = tmp_path / "search", tmp_path / "selection"
    sdir.mkdir()
    pd.DataFrame([{"run_cnt": 1, "beta_vq": 3.0, "beta_rate": 1.5, "avg_bpp": 0.2004, "diff": 0.0004},
                  {"run_cnt": 2, "beta_vq": 3.0, "beta_rate": 2.9, "avg_bpp": 0.3, "diff": 0.1}]).to_csv(sdir / "result_beta_vq_3.00_target_rate_0.200.csv")
    monkeypatch.setattr(sys, "argv", ["beta_selection.py", CONFIG, "--search_dir", str(sdir), "--save_dir", str(sel), "--dataset_root", str(out),
                                      "--beta_vq", "3.0", "--target_rate", "0.2", "--batch_size", "2", "--keep_recon", "--synthetic_weights", "-d", DEV])
    beta_selection.main()
    res = pd.read_csv(sel / "target_rate_0.2" / "result.csv", index_col=0)
    assert list(res.columns) == ["beta_vq", "beta_rate", "bpp", "psnr", "fid", "score"] and len(res) == 1 and res.iloc[0]["beta_rate"] == 1.5
    names = sorted(os.path.basename(p)[:-4] + ".png" for p, _, _ in plan)
    assert sorted(os.listdir(sel / "target_rate_0.2" / "beta_vq_3.00")) == sorted(names + ["_avg_bitrate.json", "_rate_summary.csv"])
    rs = pd.read_csv(sel / "target_rate_0.2" / "beta_vq_3.00" / "_rate_summary.csv", index_col=0)
    assert list(rs.columns) == ["img_name", "num_pixel", "total_bit", "bitrate"] and (rs["num_pixel"] == 256 * 256).all()
    assert list(rs["img_name"]) == [n[:-4] for n in names] and (rs["bitrate"] > 0).all()
    top = pd.read_csv(sel / "beta_selection_results.csv")
    assert list(top.columns) == ["target_rate", "selected_beta_vq", "selected_beta_rate"] and len(top) == 1
