"""The training data feed on the GPU: csrc/data.hip against Pillow's own resize + crop + flip + conversion, TrainFeed against HostFeed
and CropDataset, and one scripts/train.py run on a real folder.  Every comparison is torch.equal."""
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import data_feed_ref as R
from dc_vic_amd.train import data as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "dc_vic_synthetic.yaml")
GUARD = 4096
SENTINEL = 12345.0


def run_kernel(entries, S):
    """Packs the entries into a slab, launches once into a NaN-filled output between sentinel guards -> fp32 [N, 3, S, S] on the CPU."""
    from dc_vic_amd.train import kernels as K
    N = len(entries)
    _, used = D.slab_layout([e[1] for e in entries], S)
    buf = np.zeros(used, dtype=np.uint8)
    assert D.pack_batch(buf, entries, S) == used
    slab = torch.from_numpy(buf).cuda()
    table = D.conversion_table().cuda()
    n = N * 3 * S * S
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = whole[GUARD:GUARD + n].view(N, 3, S, S)
    out.fill_(float("nan"))
    K.u8_resample_crop(slab, used, buf.ctypes.data, N, S, table, out)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all()), "the launch wrote outside its output"
    return out.cpu()


@pytest.fixture(scope="module")
def built():
    return {c: R.build_case(c) for c in R.KERNEL_CASES}


@pytest.mark.parametrize("S", sorted({c[0] for c in R.KERNEL_CASES}))
def test_kernel_equals_pillow(built, S):
    """All cases of one crop size as one batch (different windows, scales, filters and flips), then each image alone, then again."""
    cases = [c for c in R.KERNEL_CASES if c[0] == S]
    entries = [built[c][0] for c in cases]
    got = run_kernel(entries, S)
    assert not torch.isnan(got).any()
    for i, c in enumerate(cases):
        assert torch.equal(got[i], built[c][1]), c
    assert torch.equal(run_kernel(entries, S), got)                       # a second run
    for i in range(min(len(cases), 3)):                                   # alone: the bits of the batch
        assert torch.equal(run_kernel([entries[i]], S)[0], got[i]), cases[i]


def test_copy_axes_with_padded_rows():
    """Both axes "copy" with a row stride wider than the window: the plain crop path of the feed, flip on and off."""
    from dc_vic_amd.train import kernels as K
    S, stride = 37, 37 * 3 + 5
    px = R.noise(S, S, 2)
    buf = np.zeros(4096 + S * stride, dtype=np.uint8)
    d = buf[:96].view(D.DESC_DTYPE)
    for i in range(2):
        d[i] = (4096, 0, 0, S, S, stride, i, 0, 0)
    buf[4096:].reshape(S, stride)[:, :S * 3] = px.reshape(S, S * 3)
    out = torch.full((2, 3, S, S), float("nan"), device="cuda")
    K.u8_resample_crop(torch.from_numpy(buf).cuda(), buf.size, buf.ctypes.data, 2, S, D.conversion_table().cuda(), out)
    assert torch.equal(out[0].cpu(), R.to_model_range(px)) and torch.equal(out[1].cpu(), R.to_model_range(px[:, ::-1]))


# ---------------------------------------------------------------------------------------------------- the feed
S_FEED = 48


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("feed_gpu")
    return str(root), R.write_folder(str(root), S_FEED)


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("dcvic_train_cli_data_feed_gpu", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("resize", (None, (0.5, 1.0)), ids=("resize_off", "resize_0.5_1.0"))
def test_train_feed_equals_host_feed(cli, folder, resize):
    """3 batches of 4 with 2 workers from the 5-file folder (an epoch boundary, the small file, the pad-case file)."""
    root, paths = folder
    recs = D.CropPlanner(paths, S_FEED, 0, 1, 5, resize_range=resize).take(12)
    assert any(r.pad for r in recs) and any(not r.pad for r in recs)
    host = D.HostFeed(paths, S_FEED, 0, 1, 5, resize_range=resize)
    feed = D.TrainFeed(paths, S_FEED, 0, 1, 5, "cuda:0", workers=2, depth=2, resize_range=resize)
    old = cli.CropDataset(root, S_FEED, 0, 1, 5) if resize is None else None
    try:
        for _ in range(3):
            x, want = feed.batch(4), host.batch(4)
            assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (4, 3, S_FEED, S_FEED)
            assert torch.equal(x.cpu(), want)
            if old is not None:
                assert torch.equal(want, old.batch(4))
    finally:
        feed.close()
    with pytest.raises(RuntimeError, match="after close"):
        feed.batch(4)


def test_train_feed_skip_and_depth(folder):
    """skip(k) then batches = the tail of the uninterrupted stream; the batches do not depend on workers or depth."""
    _, paths = folder
    a = D.TrainFeed(paths, S_FEED, 0, 1, 8, "cuda:0", workers=1, depth=1, resize_range=(0.5, 1.0), interpolation="bilinear")
    b = D.TrainFeed(paths, S_FEED, 0, 1, 8, "cuda:0", workers=3, depth=3, resize_range=(0.5, 1.0), interpolation="bilinear")
    try:
        b.skip(3)
        xa = [a.batch(3) for _ in range(3)]
        xb = [b.batch(3) for _ in range(2)]
        assert torch.equal(xa[1], xb[0]) and torch.equal(xa[2], xb[1])
    finally:
        a.close()
        b.close()


def test_truncated_file_raises_with_its_path(tmp_path):
    from PIL import Image
    good, bad = tmp_path / "good.png", tmp_path / "bad.png"
    Image.fromarray(R.noise(80, 90, 0)).save(good)
    Image.fromarray(R.noise(80, 90, 1)).save(bad)
    raw = bad.read_bytes()
    bad.write_bytes(raw[:len(raw) // 2])                 # the header still reads, the pixel data ends early
    feed = D.TrainFeed([str(bad), str(good)], S_FEED, 0, 1, 0, "cuda:0", workers=2)
    try:
        with pytest.raises(Exception, match="bad.png"):
            for _ in range(2):
                feed.batch(2)
    finally:
        feed.close()
    assert feed.closed


# ---------------------------------------------------------------------------------------------------- the CLI
def test_train_cli_on_a_real_folder(tmp_path):
    from PIL import Image
    root = tmp_path / "images"
    os.makedirs(root)
    for i, (H, W) in enumerate(((300, 280), (257, 400), (200, 330))):
        Image.fromarray((R.ramp(H, W) // 2 + R.noise(H, W, i) // 2).astype(np.uint8)).save(root / f"{i}.jpg", quality=90)
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), CFG, "--synthetic_weights", "--allow_synthetic_lpips",
                          "--dataset_root", str(root), "--total_iter", "2", "--batch_size", "2", "--log_step", "1"], cwd=ROOT, capture_output=True,
                         text=True)
    print(f"scripts/train.py on a generated folder, 2 iterations: {time.perf_counter() - t0:.1f} s wall")
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    data = [ln for ln in lines if ln.startswith("[train] data:")]
    assert len(data) == 1 and "3 images" in data[0] and "flat" in data[0] and "crop 256" in data[0] and "resize off" in data[0] and "depth 2" in data[0]
    assert len([ln for ln in lines if ln.startswith("iter ")]) == 2
