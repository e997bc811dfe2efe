"""LPIPS / DISTS weight loading and the plain-torch fp64 restatement of both metrics (CPU; no GPU needed).

`dists_ref` and `lpips_ref` restate DISTS_pytorch's DISTS.forward and lpips.LPIPS(net='alex').forward in fp64 with torch's own
operators; tests/test_gpu_metrics.py measures the HIP path (dc_vic_amd.metrics) against them.  Parity with the packages themselves is
unpinned: neither is in the reference tree."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dc_vic_amd.metrics import DISTS_CHNS, VGG16_STAGES, DISTSVGG, hann_filter, load_lpips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ fp64 restatements
def _l2pool_ref(x):
    g = hann_filter().double()[None, None].repeat(x.shape[1], 1, 1, 1)
    return torch.sqrt(F.conv2d(x ** 2, g, stride=2, padding=1, groups=x.shape[1]) + 1e-12)


def dists_feats_ref(m: DISTSVGG, x):
    """[x, relu1_2, relu2_2, relu3_3, relu4_3, relu5_3] in fp64 (x: [N, 3, H, W] in [0, 1])."""
    x = x.double()
    h = (x - m.mean.double().cpu()) / m.std.double().cpu()
    feats = [x]
    for pool, convs in m.stages():
        if pool is not None:
            h = _l2pool_ref(h)
        for c in convs:
            h = F.relu(F.conv2d(h, c.weight.detach().double().cpu(), c.bias.detach().double().cpu(), padding=1))
        feats.append(h)
    return feats


def dists_ref(m: DISTSVGG, x, y):
    """DISTS(x_n, y_n) per image, fp64 (DISTS_pytorch DISTS.forward with require_grad=False)."""
    fx, fy = dists_feats_ref(m, x), dists_feats_ref(m, y)
    a, b = m.alpha.detach().double().cpu(), m.beta.detach().double().cpu()
    w_sum = a.sum() + b.sum()
    alpha = torch.split(a / w_sum, list(DISTS_CHNS), dim=1)
    beta = torch.split(b / w_sum, list(DISTS_CHNS), dim=1)
    d1 = d2 = 0
    c1 = c2 = 1e-6
    for k in range(len(DISTS_CHNS)):
        mx, my = fx[k].mean([2, 3], keepdim=True), fy[k].mean([2, 3], keepdim=True)
        S1 = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1)
        d1 = d1 + (alpha[k] * S1).sum(1, keepdim=True)
        vx = ((fx[k] - mx) ** 2).mean([2, 3], keepdim=True)
        vy = ((fy[k] - my) ** 2).mean([2, 3], keepdim=True)
        cxy = (fx[k] * fy[k]).mean([2, 3], keepdim=True) - mx * my
        S2 = (2 * cxy + c2) / (vx + vy + c2)
        d2 = d2 + (beta[k] * S2).sum(1, keepdim=True)
    return (1 - (d1 + d2)).reshape(-1)


def lpips_ref(m, x, y):
    """LPIPS v0.1 alex (linear heads, spatial average, sum of the 5 taps) per image, fp64 (x, y in [-1, 1])."""
    sh, sc = m.scaling_layer.shift.double().cpu(), m.scaling_layer.scale.double().cpu()

    def feats(t):
        h = (t.double() - sh) / sc
        out = []
        for i, conv in enumerate(m.convs()):
            if i in (1, 2):
                h = F.max_pool2d(h, 3, 2)
            st, pd = (4, 2) if i == 0 else (1, conv.padding)
            h = F.relu(F.conv2d(h, conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), stride=st, padding=pd))
            out.append(h)
        return out

    total = 0
    for k, (a, b) in enumerate(zip(feats(x), feats(y))):
        na = a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt((b ** 2).sum(1, keepdim=True)) + 1e-10)
        w = getattr(m, f"lin{k}").model[1].weight.detach().double().cpu()
        total = total + F.conv2d((na - nb) ** 2, w).mean([2, 3])
    return total.reshape(-1)


# ------------------------------------------------------------------------------------------------ state-dict layouts
def torchvision_vgg16_sd(m: DISTSVGG):
    sd = {}
    for c, i in zip(m.convs(), [i for idxs in VGG16_STAGES for i in idxs]):
        sd[f"features.{i}.weight"] = c.weight.detach().clone()
        sd[f"features.{i}.bias"] = c.bias.detach().clone()
    sd["classifier.0.weight"] = torch.zeros(4, 8)          # ignored
    return sd


def full_dists_sd(m: DISTSVGG):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _params(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_dists_layouts_load_identically(tmp_path):
    src = DISTSVGG.synthetic(3)
    torch.save(torchvision_vgg16_sd(src), tmp_path / "vgg16.pth")
    torch.save({"alpha": src.alpha.detach().clone(), "beta": src.beta.detach().clone()}, tmp_path / "weights.pt")
    torch.save(full_dists_sd(src), tmp_path / "dists_full.pt")
    a = DISTSVGG.from_files(vgg16_path=str(tmp_path / "vgg16.pth"), dists_path=str(tmp_path / "weights.pt"))
    b = DISTSVGG.from_files(dists_path=str(tmp_path / "dists_full.pt"))
    want = _params(src)
    assert sum(v.numel() for k, v in want.items() if k.endswith(".weight")) == 14710464   # VGG16 conv weights
    for got in (_params(a), _params(b)):
        assert got.keys() == want.keys()
        for k in want:
            assert torch.equal(got[k], want[k]), k
    assert sum(DISTS_CHNS) == 1475 and tuple(a.alpha.shape) == (1, 1475, 1, 1)


def test_dists_full_state_dict_maps_convs_by_order():
    """Sub-module indices inside a stage do not matter; the convs' order does."""
    src = DISTSVGG.synthetic(4)
    sd = {}
    for k, v in full_dists_sd(src).items():
        parts = k.split(".")
        if parts[0].startswith("stage") and parts[1].isdigit():
            parts[1] = str(int(parts[1]) * 10 + 7)
        sd[".".join(parts)] = v
    got = DISTSVGG.from_state_dicts(None, sd)
    for c0, c1 in zip(src.convs(), got.convs()):
        assert torch.equal(c0.weight, c1.weight) and torch.equal(c0.bias, c1.bias)


def test_dists_bad_weights_raise_valueerror():
    src = DISTSVGG.synthetic(5)
    vgg, ab = torchvision_vgg16_sd(src), {"alpha": src.alpha.detach(), "beta": src.beta.detach()}
    bad = dict(vgg); del bad["features.19.weight"]
    with pytest.raises(ValueError, match="features.19.weight"):
        DISTSVGG.from_state_dicts(bad, ab)
    with pytest.raises(ValueError, match="alpha"):
        DISTSVGG.from_state_dicts(vgg, {"alpha": torch.zeros(1, 1474, 1, 1), "beta": ab["beta"]})
    with pytest.raises(ValueError, match="beta"):
        DISTSVGG.from_state_dicts(vgg, {"alpha": ab["alpha"]})
    with pytest.raises(ValueError, match="VGG16"):
        DISTSVGG.from_state_dicts(None, ab)
    bad = dict(vgg); bad["features.0.weight"] = torch.zeros(64, 3, 5, 5)
    with pytest.raises(ValueError, match="features.0.weight"):
        DISTSVGG.from_state_dicts(bad, ab)
    full = full_dists_sd(src)
    f = dict(full); f["stage3.9.filter"] = torch.full_like(f["stage3.9.filter"], 1.0 / 9)   # a box filter, not Hann
    with pytest.raises(ValueError, match="Hann"):
        DISTSVGG.from_state_dicts(None, f)
    f = dict(full); del f["stage4.16.filter"]
    with pytest.raises(ValueError, match="filter"):
        DISTSVGG.from_state_dicts(None, f)
    f = dict(full); del f["stage5.28.bias"]
    with pytest.raises(ValueError, match="stage5.28.bias"):
        DISTSVGG.from_state_dicts(None, f)
    f = dict(full); del f["stage2.7.weight"]; del f["stage2.7.bias"]
    with pytest.raises(ValueError, match="stage2"):
        DISTSVGG.from_state_dicts(None, f)
    with pytest.raises(ValueError):
        DISTSVGG.from_state_dicts(vgg, full)         # both layouts at once is ambiguous


def test_lpips_state_dict_loads_by_key(tmp_path):
    src = load_lpips(None, seed=6)
    torch.save(src.state_dict(), tmp_path / "lpips.pth")
    got = load_lpips(torch.load(tmp_path / "lpips.pth", weights_only=True))
    want = _params(src)
    assert _params(got).keys() == want.keys()
    assert all(torch.equal(_params(got)[k], want[k]) for k in want)
    assert not torch.equal(_params(load_lpips(None, seed=0))["net.slice1.0.weight"], want["net.slice1.0.weight"])
    bad = dict(want); del bad["lin3.model.1.weight"]
    with pytest.raises(ValueError, match="lin3.model.1.weight"):
        load_lpips(bad)


def _calc_metrics_module():
    spec = importlib.util.spec_from_file_location("dcvic_calc_metrics_host", os.path.join(ROOT, "scripts", "calc_metrics.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    return cm


def test_calc_metrics_bad_weights_fail_before_images(tmp_path, monkeypatch):
    """A bad --dists_path / --lpips_path raises before any image is read and before the HIP library is touched."""
    from dc_vic_amd import _lib
    cm = _calc_metrics_module()
    real, fake = tmp_path / "real", tmp_path / "fake"
    real.mkdir(); fake.mkdir()
    (fake / "_avg_bitrate.json").write_text('{"avg_bpp": 0.5}')

    def forbidden(*a, **k):
        raise AssertionError("touched before the weights were checked")
    monkeypatch.setattr(cm, "read_img", forbidden)
    monkeypatch.setattr(cm, "retrieve_bitrate", forbidden)
    monkeypatch.setattr(cm, "get_real_fake_path_list", forbidden)
    import dc_vic_amd.metrics as M
    import dc_vic_amd.ops as O
    import dc_vic_amd.train.lpips as TL
    for mod in (_lib, M, O, TL):                  # every module that binds the library loader by name
        monkeypatch.setattr(mod, "lib", forbidden)
    src = DISTSVGG.synthetic(1)
    torch.save({"alpha": src.alpha.detach()}, tmp_path / "no_beta.pt")
    torch.save(torchvision_vgg16_sd(src), tmp_path / "vgg16.pth")
    base = ["--real_dir", str(real), "--fake_dir", str(fake)]
    with pytest.raises(ValueError, match="beta"):
        cm.main(base + ["--dists_path", str(tmp_path / "no_beta.pt"), "--vgg16_path", str(tmp_path / "vgg16.pth")])
    torch.save({"alpha": src.alpha.detach(), "beta": src.beta.detach()}, tmp_path / "weights.pt")
    with pytest.raises(ValueError, match="vgg16_path"):
        cm.main(base + ["--dists_path", str(tmp_path / "weights.pt")])
    torch.save({"net.slice1.0.weight": torch.zeros(3)}, tmp_path / "lpips_bad.pth")
    with pytest.raises(ValueError):
        cm.main(base + ["--lpips_path", str(tmp_path / "lpips_bad.pth")])
    assert not (fake / "_metrics.json").exists()


def test_dists_restatement_identity_and_symmetry():
    m = DISTSVGG.synthetic(0)
    g = torch.Generator().manual_seed(11)
    x = torch.rand((2, 3, 21, 30), generator=g, dtype=torch.float64)
    y = (x + 0.1 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    same = dists_ref(m, x, x)
    assert same.shape == (2,) and float(same.abs().max()) < 1e-12
    dxy, dyx = dists_ref(m, x, y), dists_ref(m, y, x)
    assert torch.allclose(dxy, dyx, rtol=0, atol=1e-14)
    assert float(dxy.min()) > 1e-4                          # distinct images score above zero
    # L2pool's geometry: floor((H-1)/2)+1, and a constant image pools to sqrt(sum of the filter taps inside the image) * value
    p = _l2pool_ref(torch.ones((1, 1, 5, 7), dtype=torch.float64))
    assert p.shape == (1, 1, 3, 4)
    assert abs(float(p[0, 0, 1, 1]) - 1.0) < 1e-12 and abs(float(p[0, 0, 0, 0]) - (9 / 16) ** 0.5) < 1e-12


def test_lpips_restatement_identity_and_symmetry():
    m = load_lpips(None, seed=0)
    g = torch.Generator().manual_seed(12)
    x = torch.rand((2, 3, 64, 64), generator=g, dtype=torch.float64) * 2 - 1
    y = (x + 0.2 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(-1, 1)
    assert float(lpips_ref(m, x, x).abs().max()) == 0.0
    assert torch.allclose(lpips_ref(m, x, y), lpips_ref(m, y, x), rtol=0, atol=1e-14)
    assert float(lpips_ref(m, x, y).min()) > 1e-4
    assert np.isfinite(lpips_ref(m, x, y).numpy()).all()
