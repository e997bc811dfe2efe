"""LPIPS / DISTS on the MI355X (dc_vic_amd.metrics, csrc/metrics.hip) against the fp64 CPU restatement of tests/test_metrics_host.py:
the L2 pool, the paired fp64 moments, both metrics end to end, and scripts/calc_metrics.py with weight files."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dc_vic_amd import metrics as M
from dc_vic_amd.metrics import DISTSVGG, hann_filter, load_lpips
from test_metrics_host import dists_ref, full_dists_sd, lpips_ref, torchvision_vgg16_sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# per-image bounds against the fp64 restatement, ~10x the worst error measured on the MI355X over the sizes below: DISTS 7.5e-8
# (fp64 moments over fp32 convs, values ~0.012-0.017); LPIPS 1.2e-10 (values ~9e-4 with the synthetic heads)
DISTS_ATOL = 1e-6
LPIPS_ATOL = 1.5e-9


@pytest.fixture(scope="module", autouse=True)
def _device():
    torch.cuda.set_device(0)


def _ulps(got: torch.Tensor, want64: torch.Tensor) -> float:
    w32 = want64.float()
    ulp = (torch.nextafter(w32.abs(), torch.tensor(float("inf"))) - w32.abs()).double()
    return float(((got.double() - want64).abs() / ulp).max())


# ------------------------------------------------------------------------------------------------ L2 pool
@pytest.mark.parametrize("hw", [(1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (97, 131), (512, 768)])
@pytest.mark.parametrize("n", [1, 3])
def test_l2pool_against_fp64(hw, n):
    H, W = hw
    C = 5 if H * W < 1000 else 4
    g = torch.Generator().manual_seed(H * 1000 + W + n)
    x = torch.randn((n, C, H, W), generator=g) * 3
    x[:, 0] = x[:, 0].abs()
    x[:, 1] = 0                                                  # dead channel: sqrt(1e-12)
    want = torch.sqrt(F.conv2d(x.double() ** 2, hann_filter().double()[None, None].repeat(C, 1, 1, 1), stride=2, padding=1, groups=C) + 1e-12)
    xd = x.to(DEV)
    y = M.l2pool(xd)
    assert y.shape == (n, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1) == want.shape
    assert _ulps(y.cpu(), want) <= 2.0
    assert torch.equal(M.l2pool(xd), y)                          # run to run
    for k in range(n):
        assert torch.equal(M.l2pool(xd[k:k + 1].contiguous()), y[k:k + 1])


# ------------------------------------------------------------------------------------------------ paired moments
def _moments_ref(f0, f1):
    a, b = f0.double().flatten(2), f1.double().flatten(2)
    mx, my = a.mean(2, keepdim=True), b.mean(2, keepdim=True)
    return torch.stack([mx[..., 0], my[..., 0], ((a - mx) ** 2).mean(2), ((b - my) ** 2).mean(2), (a * b).mean(2) - mx[..., 0] * my[..., 0]], -1)


def _check_moments(got, want, scale):
    """relative to the planes' magnitude: means against |x|, variances / covariance against |x|^2"""
    err = (got.cpu() - want).abs()
    assert float(err[..., :2].max()) <= 1e-13 * scale, float(err[..., :2].max())
    assert float(err[..., 2:].max()) <= 1e-12 * scale * scale, float(err[..., 2:].max())


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 1, 7), (1, 4, 33, 47), (3, 5, 64, 64), (1, 3, 65, 63), (2, 512, 32, 48),
                                   (1, 2, 2048, 1365)])
def test_pair_moments_against_fp64(shape):
    g = torch.Generator().manual_seed(sum(shape))
    f0 = torch.relu(torch.randn(shape, generator=g) * 2 + 0.5)
    f1 = torch.relu(f0 + 0.3 * torch.randn(shape, generator=g))
    got = M.pair_moments(f0.to(DEV), f1.to(DEV))
    want = _moments_ref(f0, f1)
    assert got.dtype == torch.float64 and got.shape == (shape[0], shape[1], 5)
    _check_moments(got, want, 4.0)
    assert torch.equal(M.pair_moments(f0.to(DEV), f1.to(DEV)), got)
    for k in range(shape[0]):
        assert torch.equal(M.pair_moments(f0[k:k + 1].to(DEV), f1[k:k + 1].to(DEV)), got[k:k + 1])


def test_pair_moments_more_planes_than_one_launch():
    """N * C = 66560 planes: more than one grid.y launch (65535) -- the batch sizes of a folder of small images."""
    g = torch.Generator().manual_seed(130)
    f0 = torch.relu(torch.randn((130, 512, 2, 2), generator=g) + 0.2)
    f1 = torch.relu(f0 + 0.5 * torch.randn(f0.shape, generator=g))
    f0d, f1d = f0.to(DEV), f1.to(DEV)
    got = M.pair_moments(f0d, f1d)
    _check_moments(got, _moments_ref(f0, f1), 4.0)
    for k in (0, 127, 128, 129):                                 # images on both sides of the launch boundary (plane 65535 is in image 127)
        assert torch.equal(M.pair_moments(f0d[k:k + 1], f1d[k:k + 1]), got[k:k + 1])
    assert torch.equal(M.pair_moments(f0d[1:], f1d[1:]), got[1:])   # shifted across the boundary


def test_pair_moments_special_planes():
    H, W = 97, 131
    g = torch.Generator().manual_seed(5)
    f0 = torch.zeros((2, 4, H, W))
    f1 = torch.zeros((2, 4, H, W))
    f0[:, 1] = 3.25; f1[:, 1] = 3.25                             # constant planes: variances and covariance exactly 0
    f0[:, 2] = 1e3 + 1e-3 * torch.randn((2, H, W), generator=g, dtype=torch.float64).float()
    f1[:, 2] = 1e3 + 1e-3 * torch.randn((2, H, W), generator=g, dtype=torch.float64).float()
    f0[:, 3] = torch.randn((2, H, W), generator=g); f1[:, 3] = -f0[:, 3]
    got = M.pair_moments(f0.to(DEV), f1.to(DEV)).cpu()
    want = _moments_ref(f0, f1)
    assert torch.equal(got[:, 0], torch.zeros_like(got[:, 0]))   # dead ReLU planes: all moments 0 -> S1 = S2 = 1
    assert torch.equal(got[:, 1, 2:], torch.zeros_like(got[:, 1, 2:])) and bool((got[:, 1, :2] == 3.25).all())
    # mean 1e3, std 1e-3 (fp32 spacing at 1e3 is 6e-5, so the planes hold ~16 levels): variances to 1e-9 relative, where a naive fp32
    # one-pass E[x^2] - mu^2 loses every digit (its rounding is ~1e6 * 6e-8 = 0.06, against variances of ~1e-6)
    rel = ((got[:, 2, 2:4] - want[:, 2, 2:4]).abs() / want[:, 2, 2:4]).max()
    assert float(rel) < 1e-9, float(rel)
    naive = (f0[:, 2].flatten(1) ** 2).mean(1) - f0[:, 2].flatten(1).mean(1) ** 2
    assert float(((naive.double() - want[:, 2, 2]).abs() / want[:, 2, 2]).max()) > 1.0
    assert float((got[:, 2, :2] - want[:, 2, :2]).abs().max()) <= 1e-10
    _check_moments(got[:, 3:], want[:, 3:], 4.0)
    # the DISTS score of these moments: S1 = S2 = 1 on a dead plane -> 1 - (alpha + beta) = 0 when all weight sits there
    alpha = torch.zeros(4, dtype=torch.float64, device=DEV); alpha[0] = 0.5
    beta = alpha.clone()
    out = torch.empty(2, dtype=torch.float64, device=DEV)
    gm = got.to(DEV).contiguous()
    from dc_vic_amd._lib import check, lib
    import ctypes as C
    from dc_vic_amd.ops import _p, _stream
    check(lib().dcvic_dists_score_f64(_p(gm), C.c_longlong(20), _p(alpha), _p(beta), 2, 4, _p(out), _stream()), "dists_score")
    assert torch.equal(out.cpu(), torch.zeros(2, dtype=torch.float64))


def test_pair_moments_rejects_bad_arguments():
    x = torch.zeros((1, 2, 4, 4), device=DEV)
    with pytest.raises(ValueError):
        M.pair_moments(x, torch.zeros((1, 2, 4, 5), device=DEV))
    with pytest.raises(ValueError):
        M.pair_moments(x, x, out=torch.empty((1, 2, 5), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        M.l2pool(x.double())


# ------------------------------------------------------------------------------------------------ metrics end to end
_CPU_CACHE = {}


def _images(H, W, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 3, H, W), generator=g)
    y = (x + 0.08 * torch.randn(x.shape, generator=g)).clamp(0, 1)
    return x, y


def _ref(kind, model, x, y, key):
    if key not in _CPU_CACHE:
        _CPU_CACHE[key] = (dists_ref if kind == "dists" else lpips_ref)(model, x, y)
    return _CPU_CACHE[key]


@pytest.fixture(scope="module")
def dists_model():
    return DISTSVGG.synthetic(0).to(DEV)


@pytest.fixture(scope="module")
def lpips_model():
    return load_lpips(None, seed=0).to(DEV)


@pytest.mark.parametrize("hw", [(64, 64), (97, 131), (512, 768)])
@pytest.mark.parametrize("n", [1, 3])
def test_dists_end_to_end(dists_model, hw, n):
    H, W = hw
    x, y = _images(H, W, 3, H + W)
    x, y = x[:n], y[:n]
    want = torch.cat([_ref("dists", dists_model, x[k:k + 1], y[k:k + 1], ("d", hw, k)) for k in range(n)])
    xd, yd = x.to(DEV), y.to(DEV)
    got = M.dists(dists_model, xd, yd)
    assert got.dtype == torch.float64 and got.shape == (n,)
    err = float((got.cpu() - want).abs().max())
    print(f"DISTS {H}x{W} n={n}: values {want.tolist()} max err {err:.3e}")
    assert err <= DISTS_ATOL, err
    assert bool((want > 1e-3).all())
    assert torch.equal(M.dists(dists_model, xd, yd), got)        # run to run
    for k in range(n):                                           # the 2N batch vs one pair at a time
        assert torch.equal(M.dists(dists_model, xd[k:k + 1].contiguous(), yd[k:k + 1].contiguous()), got[k:k + 1])
    assert float((M.dists(dists_model, yd, xd) - got).abs().max()) <= 1e-7
    assert float(M.dists(dists_model, xd, xd).abs().max()) <= 1e-6


@pytest.mark.parametrize("hw", [(64, 64), (97, 131), (99, 67), (512, 768)])   # H or W = 3 mod 4: the stem's last row / column
@pytest.mark.parametrize("n", [1, 3])
def test_lpips_end_to_end(lpips_model, hw, n):
    H, W = hw
    x, y = _images(H, W, 3, 7 * H + W)
    x, y = x[:n] * 2 - 1, y[:n] * 2 - 1
    want = torch.cat([_ref("lpips", lpips_model, x[k:k + 1], y[k:k + 1], ("l", hw, k)) for k in range(n)])
    xd, yd = x.to(DEV), y.to(DEV)
    got = M.lpips(lpips_model, xd, yd)
    assert got.dtype == torch.float64 and got.shape == (n,)
    err = float((got.cpu() - want).abs().max())
    print(f"LPIPS {H}x{W} n={n}: values {want.tolist()} max err {err:.3e}")
    assert err <= LPIPS_ATOL, err
    assert bool((want > 1e-4).all())
    assert torch.equal(M.lpips(lpips_model, xd, yd), got)
    for k in range(n):
        assert torch.equal(M.lpips(lpips_model, xd[k:k + 1].contiguous(), yd[k:k + 1].contiguous()), got[k:k + 1])
    assert float((M.lpips(lpips_model, yd, xd) - got).abs().max()) <= 1e-7
    assert torch.equal(M.lpips(lpips_model, xd, xd), torch.zeros(n, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ calc_metrics CLI
def test_calc_metrics_lpips_and_dists(tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("dcvic_calc_metrics_gpu", os.path.join(ROOT, "scripts", "calc_metrics.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    rng = np.random.default_rng(9)
    real, fake = tmp_path / "real", tmp_path / "fake"
    real.mkdir(); fake.mkdir()
    pairs = []
    for i, (H, W) in enumerate([(64, 96), (37, 53), (64, 96)]):          # one odd-sized pair: two shape buckets
        a = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int32) + rng.integers(-20, 21, size=a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(real / f"im{i}.png"); Image.fromarray(b).save(fake / f"im{i}.png")
        pairs.append((a, b))
    (fake / "_avg_bitrate.json").write_text(json.dumps({"avg_bpp": 0.25}))
    base = ["--real_dir", str(real), "--fake_dir", str(fake)]
    plain = cm.main(base)
    assert list(plain) == ["bpp", "PSNR"]

    dm, lm = DISTSVGG.synthetic(2), load_lpips(None, seed=2)
    torch.save(torchvision_vgg16_sd(dm), tmp_path / "vgg16.pth")
    torch.save({"alpha": dm.alpha.detach(), "beta": dm.beta.detach()}, tmp_path / "weights.pt")
    torch.save(full_dists_sd(dm), tmp_path / "dists_full.pt")
    torch.save(lm.state_dict(), tmp_path / "lpips.pth")
    out = cm.main(base + ["--lpips_path", str(tmp_path / "lpips.pth"), "--dists_path", str(tmp_path / "weights.pt"),
                          "--vgg16_path", str(tmp_path / "vgg16.pth"), "-d", DEV])
    js = json.loads((fake / "_metrics.json").read_text())
    assert list(js) == ["bpp", "PSNR", "LPIPS", "DISTS"] and js == out
    assert out["PSNR"] == plain["PSNR"] and out["bpp"] == 0.25
    out_full = cm.main(base + ["--dists_path", str(tmp_path / "dists_full.pt"), "-d", DEV])
    assert list(out_full) == ["bpp", "PSNR", "DISTS"] and out_full["DISTS"] == out["DISTS"]

    dmd, lmd = dm.to(DEV), lm.to(DEV)
    api_d, api_l, ref_d, ref_l = [], [], [], []
    for a, b in pairs:                                      # metric(fake, real) on ToTensor / Normalize(.5, .5) inputs
        r01 = torch.from_numpy(a.astype(np.float32) / np.float32(255)).permute(2, 0, 1)[None].contiguous()
        f01 = torch.from_numpy(b.astype(np.float32) / np.float32(255)).permute(2, 0, 1)[None].contiguous()
        api_d.append(float(M.dists(dmd, f01.to(DEV), r01.to(DEV))[0]))
        api_l.append(float(M.lpips(lmd, ((f01 - .5) / .5).to(DEV), ((r01 - .5) / .5).to(DEV))[0]))
        ref_d.append(float(dists_ref(dm, f01, r01)[0]))
        ref_l.append(float(lpips_ref(lm, (f01 - .5) / .5, (r01 - .5) / .5)[0]))
    assert out["DISTS"] == float(np.mean(api_d)) and out["LPIPS"] == float(np.mean(api_l))
    assert abs(out["DISTS"] - np.mean(ref_d)) <= DISTS_ATOL and abs(out["LPIPS"] - np.mean(ref_l)) <= LPIPS_ATOL
