"""MS-SSIM / PSNR yardstick and the host side of the trainer's validation (CPU, no GPU).

PARITY UNPINNED: pytorch-msssim (0.2.1, pinned in the reference's poetry.lock) is not in the reference tree and cannot be fetched.
`ms_ssim_ref` restates its ms_ssim in plain torch fp64 on the integer planes of the reference's calc_ms_ssim, `psnr_ref` the
reference's calc_psnr (src/utils/img_utils.py:104-160) with an exact integer squared-error sum; tests/test_gpu_ssim.py compares the
HIP kernels against them."""
import csv
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def int_planes(x: torch.Tensor) -> torch.Tensor:
    """calc_ms_ssim's `cvt_range_to_255(x).int()`: (x + 1) / 2 * 255 in fp32, truncated (calc_psnr's astype(uint8) is the same
    for x in [-1, 1])."""
    return ((x.detach().float().cpu() + 1.0) / 2.0 * 255.0).int()


def ssim_window() -> torch.Tensor:
    """pytorch_msssim._fspecial_gauss_1d(11, 1.5) in fp32, as the package builds it."""
    coords = torch.arange(11).to(dtype=torch.float)
    coords -= 11 // 2
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    return g


def scale_sizes(H: int, W: int):
    """Plane sizes at the 5 scales: avg_pool2d(2, padding = size % 2) turns s into s // 2 + s % 2."""
    out = [(H, W)]
    for _ in range(4):
        h, w = out[-1]
        out.append((h // 2 + h % 2, w // 2 + w % 2))
    return out


def _filter(X: torch.Tensor, win: torch.Tensor) -> torch.Tensor:
    C = X.shape[1]
    out = F.conv2d(X, win.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)      # valid, along H
    return F.conv2d(out, win.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)   # then along W


def _ssim(X: torch.Tensor, Y: torch.Tensor, win: torch.Tensor):
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    mu1, mu2 = _filter(X, win), _filter(Y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _filter(X * X, win) - mu1_sq
    s2 = _filter(Y * Y, win) - mu2_sq
    s12 = _filter(X * Y, win) - mu1_mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ms_ssim_ref(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Per image of [N, C, H, W] in [-1, 1]: pytorch_msssim.ms_ssim(data_range=255) of calc_ms_ssim's integer planes, in fp64 (the
    package's fp32 window and weights, widened), averaged over channels; -1 where min(H, W) <= 160 (the package asserts, the
    reference reports -1)."""
    X, Y = int_planes(x).double(), int_planes(y).double()
    N = X.shape[0]
    if min(X.shape[-2:]) <= 160:
        return torch.full((N,), -1.0, dtype=torch.float64)
    win = ssim_window().double()
    weights = torch.tensor(WEIGHTS, dtype=torch.float32).double()
    mcs = []
    for i in range(5):
        ssim_pc, cs = _ssim(X, Y, win)
        if i < 4:
            mcs.append(torch.relu(cs))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    vals = torch.stack(mcs + [torch.relu(ssim_pc)], dim=0) ** weights.view(-1, 1, 1)
    return torch.prod(vals, dim=0).mean(1)


def sse_ref(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Exact squared-error sum of the integer planes per image (int64)."""
    d = int_planes(x).long() - int_planes(y).long()
    return (d * d).flatten(1).sum(1)


def psnr_ref(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """calc_psnr per image: 10 log10(255^2 / mse) on the integer planes, mse from the exact integer sum; inf for identical images."""
    mse = sse_ref(x, y).double() / float(x[0].numel())
    return 10.0 * torch.log10(65025.0 / mse)


def _pair(N, H, W, seed=0, noise=0.1):
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand((N, 3, H // 8 + 1, W // 8 + 1), generator=g, dtype=torch.float64) * 2 - 1, size=(H, W), mode="bilinear",
                         align_corners=False)
    x = base.float().clamp(-1, 1)
    y = (base + noise * torch.randn((N, 3, H, W), generator=g, dtype=torch.float64)).float().clamp(-1, 1)
    return x, y


# ------------------------------------------------------------------------------------------------ the yardstick
def test_window_sums_to_one_and_matches_the_kernel_constants():
    g = ssim_window()
    assert abs(float(g.double().sum()) - 1.0) < 1e-6
    assert torch.equal(g, g.flip(0)) and int(g.argmax()) == 5
    # csrc/ssim.hip holds the same fp32 window as hex literals
    src = open(os.path.join(ROOT, "dc_vic_amd", "csrc", "ssim.hip")).read()
    body = re.search(r"c_win\[WIN\]\s*=\s*\{([^}]*)\}", src).group(1)
    lits = [float.fromhex(t.strip().rstrip("f")) for t in body.split(",")]
    assert lits == [float(v) for v in g]


def test_identical_images_give_one_and_inf():
    x, _ = _pair(2, 200, 180, seed=1)
    assert torch.equal(ms_ssim_ref(x, x), torch.ones(2, dtype=torch.float64))
    assert torch.isinf(psnr_ref(x, x)).all()


def test_symmetric():
    x, y = _pair(2, 170, 230, seed=2)
    assert torch.allclose(ms_ssim_ref(x, y), ms_ssim_ref(y, x), rtol=0, atol=1e-14)
    assert torch.equal(psnr_ref(x, y), psnr_ref(y, x))
    v = ms_ssim_ref(x, y)
    assert ((v > 0.1) & (v < 1.0)).all(), v


def test_small_image_rule_and_scale_sizes():
    for H, W in ((160, 300), (300, 160), (160, 160)):
        x, y = _pair(1, H, W, seed=3)
        assert float(ms_ssim_ref(x, y)[0]) == -1.0
    x, y = _pair(1, 161, 161, seed=4)
    assert 0.0 < float(ms_ssim_ref(x, y)[0]) < 1.0
    sizes = scale_sizes(161, 161)
    assert sizes[-1] == (11, 11)                       # the valid 11-tap map at scale 4 is 1 x 1
    assert (sizes[-1][0] - 10, sizes[-1][1] - 10) == (1, 1)


def test_pool_sizes_for_odd_sides():
    for H, W in ((163, 201), (333, 257), (161, 162)):
        X = torch.zeros((1, 1, H, W), dtype=torch.float64)
        sz = scale_sizes(H, W)
        for s in range(4):
            X = F.avg_pool2d(X, kernel_size=2, padding=(X.shape[2] % 2, X.shape[3] % 2))
            assert tuple(X.shape[2:]) == sz[s + 1]
            assert sz[s + 1] == (sz[s][0] // 2 + 1 if sz[s][0] % 2 else sz[s][0] // 2, sz[s][1] // 2 + 1 if sz[s][1] % 2 else sz[s][1] // 2)


def test_psnr_matches_the_float32_numpy_formula():
    x, y = _pair(1, 64, 48, seed=5)
    a = ((x.numpy() + 1.0) / 2.0 * 255.0).astype(np.uint8).astype(np.float32)
    b = ((y.numpy() + 1.0) / 2.0 * 255.0).astype(np.uint8).astype(np.float32)
    ref = 10.0 * math.log10(255.0 ** 2 / np.mean(np.power(a - b, 2)))
    assert abs(float(psnr_ref(x, y)[0]) - ref) < 1e-4          # np.mean in fp32 vs the exact sum


# ------------------------------------------------------------------------------------------------ validation host side
def test_msssim_workspace_bytes_host_formula():
    from dc_vic_amd import _lib
    L = _lib.lib()
    assert L.dcvic_msssim_workspace_bytes(0, 3, 512, 768) == 0 and L.dcvic_msssim_workspace_bytes(1, 3, -1, 768) == 0
    small = L.dcvic_msssim_workspace_bytes(1, 3, 160, 768)      # PSNR only: the squared-error partials
    full = L.dcvic_msssim_workspace_bytes(1, 3, 161, 768)
    assert 0 < small < full
    assert L.dcvic_msssim_workspace_bytes(3, 3, 512, 768) > 2 * L.dcvic_msssim_workspace_bytes(1, 3, 512, 768)
    # the pooled planes of scales 1-4 alone need 2 * N * C * sum(h * w) fp32 values
    sz = scale_sizes(512, 768)
    assert L.dcvic_msssim_workspace_bytes(2, 3, 512, 768) > 2 * 2 * 3 * 4 * sum(h * w for h, w in sz[1:])


def _png(path, h, w, seed):
    from PIL import Image
    a = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    Image.fromarray(a).save(path)
    return a


def test_eval_set_sorted_capped_and_size_limited(tmp_path):
    from dc_vic_amd.train.validation import eval_image_paths, load_eval_images
    names = [f"img{i:03d}.png" for i in range(101)]
    arrays = {}
    for i, n in enumerate(reversed(names)):
        arrays[n] = _png(tmp_path / n, 4, 6, i)
    (tmp_path / "notes.txt").write_text("x")
    (tmp_path / "z.jpg").write_bytes(b"")
    paths = eval_image_paths(str(tmp_path))
    assert [os.path.basename(p) for p in paths] == names[:100]
    imgs = load_eval_images(str(tmp_path), max_images=3)
    assert len(imgs) == 3 and imgs[0].shape == (1, 3, 4, 6) and imgs[0].dtype == torch.float32
    ref = (torch.from_numpy(arrays["img000.png"]).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5
    assert torch.equal(imgs[0][0], ref)
    big = tmp_path / "big"
    big.mkdir()
    _png(big / "a.png", 8, 1024, 0)
    assert load_eval_images(str(big))[0].shape == (1, 3, 8, 1024)
    _png(big / "b.png", 1025, 8, 1)
    with pytest.raises(ValueError, match="1024"):
        load_eval_images(str(big))
    with pytest.raises(ValueError, match="not a directory"):
        eval_image_paths(str(tmp_path / "missing"))
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no PNG"):
        eval_image_paths(str(empty))


def test_eval_csv_appends_and_resumes(tmp_path):
    from dc_vic_amd.train.validation import EvalCSV
    p = str(tmp_path / "eval_result.csv")
    w = EvalCSV(p)
    w.append({"iter": 2, "idx0_bpp": 0.25, "idx0_psnr": float("inf")})
    w.append({"iter": 4, "idx0_bpp": 0.125, "idx0_psnr": 31.5})
    w.append({"iter": 6, "idx0_bpp": 0.1, "idx0_psnr": 30.0})
    rows = list(csv.reader(open(p)))
    assert rows == [["iter", "idx0_bpp", "idx0_psnr"], ["2", "0.25", "inf"], ["4", "0.125", "31.5"], ["6", "0.1", "30.0"]]
    with pytest.raises(ValueError):
        w.append({"iter": 8, "idx0_bpp": 0.1})
    # resumed from the iteration-4 checkpoint into another folder: rows up to 4 carried over, then extended
    p2 = str(tmp_path / "eval2.csv")
    w2 = EvalCSV(p2, resume_from=p, start_iter=4)
    assert list(csv.reader(open(p2))) == rows[:3]
    w2.append({"iter": 6, "idx0_bpp": 0.1, "idx0_psnr": 30.0})
    assert open(p2).read() == open(p).read()
    # resumed in place: the same file is loaded and extended
    w3 = EvalCSV(p, resume_from=p, start_iter=6)
    w3.append({"iter": 8, "idx0_bpp": 0.05, "idx0_psnr": 29.0})
    assert [r[0] for r in csv.reader(open(p))] == ["iter", "2", "4", "6", "8"]
    # nothing to resume from: a fresh file once the first row comes
    w4 = EvalCSV(str(tmp_path / "e4.csv"), resume_from=str(tmp_path / "none.csv"), start_iter=4)
    assert not os.path.exists(str(tmp_path / "e4.csv"))
    w4.append({"iter": 6, "idx0_bpp": 0.1, "idx0_psnr": 30.0})
    assert list(csv.reader(open(str(tmp_path / "e4.csv")))) == [["iter", "idx0_bpp", "idx0_psnr"], ["6", "0.1", "30.0"]]


@pytest.mark.parametrize("root,words", [("missing_folder", "not a directory"), ("dc_vic_amd", "no PNG")])
def test_train_cli_rejects_bad_eval_root_before_gpu_work(root, words):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"),
                          "--synthetic_weights", "--synthetic_data", "--total_iter", "1", "--eval_step", "1", "--eval_dataset_root",
                          os.path.join(ROOT, root)], cwd=ROOT, capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode != 0 and "--eval_dataset_root" in res.stderr and words in res.stderr, res.stderr[-2000:]
    assert "Traceback" not in res.stderr, res.stderr[-2000:]
