"""FID pieces that need no GPU: the plain-torch fp64 FID-Inception the GPU tests compare against (`ref_features`, BatchNorm
unfolded), the state-dict loader against a manifest written out here, the BatchNorm folding, the Frechet distance, the HiFiC patch
origins, and calc_metrics' 50-image rule.  Parity with the pytorch_fid package is unpinned (it is not in the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dc_vic_amd import fid  # noqa: E402

# ------------------------------------------------------------------------------------------------ the fp64 restatement
# (name, Cin, Cout, (KH, KW), stride, (pad_h, pad_w)) of every BasicConv2d, in torchvision Inception3 naming
STEM = [("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)),
        ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)), ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)),
        ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0))]


def _block_a(cin, pf):
    return [("branch1x1", cin, 64, (1, 1), 1, (0, 0)), ("branch5x5_1", cin, 48, (1, 1), 1, (0, 0)), ("branch5x5_2", 48, 64, (5, 5), 1, (2, 2)),
            ("branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)), ("branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
            ("branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)), ("branch_pool", cin, pf, (1, 1), 1, (0, 0))]


def _block_b(cin):
    return [("branch3x3", cin, 384, (3, 3), 2, (0, 0)), ("branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            ("branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), ("branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def _block_c(cin, c7):
    return [("branch1x1", cin, 192, (1, 1), 1, (0, 0)), ("branch7x7_1", cin, c7, (1, 1), 1, (0, 0)),
            ("branch7x7_2", c7, c7, (1, 7), 1, (0, 3)), ("branch7x7_3", c7, 192, (7, 1), 1, (3, 0)),
            ("branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), ("branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
            ("branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), ("branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
            ("branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)), ("branch_pool", cin, 192, (1, 1), 1, (0, 0))]


def _block_d(cin):
    return [("branch3x3_1", cin, 192, (1, 1), 1, (0, 0)), ("branch3x3_2", 192, 320, (3, 3), 2, (0, 0)),
            ("branch7x7x3_1", cin, 192, (1, 1), 1, (0, 0)), ("branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            ("branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), ("branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def _block_e(cin):
    return [("branch1x1", cin, 320, (1, 1), 1, (0, 0)), ("branch3x3_1", cin, 384, (1, 1), 1, (0, 0)),
            ("branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), ("branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            ("branch3x3dbl_1", cin, 448, (1, 1), 1, (0, 0)), ("branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            ("branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), ("branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            ("branch_pool", cin, 192, (1, 1), 1, (0, 0))]


BLOCKS = [("Mixed_5b", _block_a(192, 32)), ("Mixed_5c", _block_a(256, 64)), ("Mixed_5d", _block_a(288, 64)), ("Mixed_6a", _block_b(288)),
          ("Mixed_6b", _block_c(768, 128)), ("Mixed_6c", _block_c(768, 160)), ("Mixed_6d", _block_c(768, 160)),
          ("Mixed_6e", _block_c(768, 192)), ("Mixed_7a", _block_d(768)), ("Mixed_7b", _block_e(1280)), ("Mixed_7c", _block_e(2048))]
CONVS = STEM + [(f"{b}.{n}", *rest) for b, convs in BLOCKS for n, *rest in convs]
CONV_SPEC = {name: (k, s, p) for name, _, _, k, s, p in CONVS}


def manifest():
    """Every key FID-Inception needs, with its shape: conv.weight and the four BatchNorm tensors of each of the 94 BasicConv2d."""
    m = {}
    for name, cin, cout, (kh, kw), _, _ in CONVS:
        m[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for t in ("weight", "bias", "running_mean", "running_var"):
            m[f"{name}.bn.{t}"] = (cout,)
    return m


def ref_conv(sd, name, x):
    """BasicConv2d in x's dtype (fp64 for the tests) as torchvision runs it: conv (no bias) -> BatchNorm2d(eps=0.001, eval) -> ReLU."""
    _, s, p = CONV_SPEC[name]
    t = lambda k: sd[f"{name}.{k}"].to(x.dtype)  # noqa: E731
    y = F.conv2d(x, t("conv.weight"), stride=s, padding=p)
    return F.relu(F.batch_norm(y, t("bn.running_mean"), t("bn.running_var"), t("bn.weight"), t("bn.bias"), training=False, eps=0.001))


def _avg(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def ref_features(sd, x, dtype=torch.float64):
    """pool3 features [N, 2048] in fp64 (or `dtype`) of network inputs x [N, 3, 299, 299] (pytorch-fid's FIDInceptionV3 blocks 0-3)."""
    c = lambda n, t: ref_conv(sd, n, t)  # noqa: E731
    h = x.to(dtype)
    h = c("Conv2d_2b_3x3", c("Conv2d_2a_3x3", c("Conv2d_1a_3x3", h)))
    h = F.max_pool2d(h, 3, 2)
    h = c("Conv2d_4a_3x3", c("Conv2d_3b_1x1", h))
    h = F.max_pool2d(h, 3, 2)
    for b in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        p = lambda n: f"{b}.{n}"  # noqa: E731
        h = torch.cat([c(p("branch1x1"), h), c(p("branch5x5_2"), c(p("branch5x5_1"), h)),
                       c(p("branch3x3dbl_3"), c(p("branch3x3dbl_2"), c(p("branch3x3dbl_1"), h))), c(p("branch_pool"), _avg(h))], 1)
    p = lambda n: f"Mixed_6a.{n}"  # noqa: E731
    h = torch.cat([c(p("branch3x3"), h), c(p("branch3x3dbl_3"), c(p("branch3x3dbl_2"), c(p("branch3x3dbl_1"), h))), F.max_pool2d(h, 3, 2)], 1)
    for b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        p = lambda n: f"{b}.{n}"  # noqa: E731
        b7 = c(p("branch7x7_3"), c(p("branch7x7_2"), c(p("branch7x7_1"), h)))
        d = h
        for i in range(1, 6):
            d = c(p(f"branch7x7dbl_{i}"), d)
        h = torch.cat([c(p("branch1x1"), h), b7, d, c(p("branch_pool"), _avg(h))], 1)
    p = lambda n: f"Mixed_7a.{n}"  # noqa: E731
    b3 = c(p("branch3x3_2"), c(p("branch3x3_1"), h))
    b7 = h
    for i in range(1, 5):
        b7 = c(p(f"branch7x7x3_{i}"), b7)
    h = torch.cat([b3, b7, F.max_pool2d(h, 3, 2)], 1)
    for b, pool in (("Mixed_7b", _avg), ("Mixed_7c", lambda t: F.max_pool2d(t, 3, 1, 1))):
        p = lambda n: f"{b}.{n}"  # noqa: E731
        t = c(p("branch3x3_1"), h)
        u = c(p("branch3x3dbl_2"), c(p("branch3x3dbl_1"), h))
        h = torch.cat([c(p("branch1x1"), h), c(p("branch3x3_2a"), t), c(p("branch3x3_2b"), t), c(p("branch3x3dbl_3a"), u),
                       c(p("branch3x3dbl_3b"), u), c(p("branch_pool"), pool(h))], 1)
    return h.mean(dim=(2, 3))


def ref_inputs(patches_u8):
    """pytorch-fid's input path in fp64 from the fp32 ToTensor values: [B, p, p, 3] u8 -> [B, 3, 299, 299]."""
    x = torch.from_numpy(np.ascontiguousarray(patches_u8)).permute(0, 3, 1, 2).float().div(255).double()
    return 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1


# ------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def synth_sd():
    return fid.FIDInception.synthetic(0).state_dict()


def test_manifest_matches_the_module():
    want = manifest()
    assert len(want) == 94 * 5
    assert dict(fid.FIDInception.manifest()) == want
    assert list(fid.FIDInception.manifest()) == list(want)        # torchvision's registration order


def test_loader_accepts_optional_keys(synth_sd):
    sd = dict(synth_sd)
    sd["fc.weight"] = torch.zeros(1008, 2048)
    sd["fc.bias"] = torch.zeros(1008)
    sd["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    m = fid.FIDInception.from_state_dict(sd)
    for k, v in m.state_dict().items():
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(v, synth_sd[k]), k
    nbt = {k: v for k, v in synth_sd.items() if not k.endswith("num_batches_tracked")}
    fid.FIDInception.from_state_dict(nbt)                         # num_batches_tracked absent


def test_loader_rejects_bad_state_dicts(synth_sd, tmp_path):
    sd = dict(synth_sd)
    del sd["Mixed_6c.branch7x7dbl_4.bn.running_var"]
    with pytest.raises(ValueError, match="Mixed_6c.branch7x7dbl_4.bn.running_var"):
        fid.FIDInception.from_state_dict(sd)
    sd = dict(synth_sd)
    sd["Mixed_7b.branch_extra.conv.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="Mixed_7b.branch_extra.conv.weight"):
        fid.FIDInception.from_state_dict(sd)
    sd = dict(synth_sd)
    sd["Mixed_6b.branch7x7_2.conv.weight"] = torch.zeros(128, 128, 7, 1)
    with pytest.raises(ValueError, match="Mixed_6b.branch7x7_2.conv.weight"):
        fid.FIDInception.from_state_dict(sd)
    with pytest.raises(ValueError):
        fid.FIDInception.from_state_dict([1, 2])
    path = tmp_path / "inc.pth"
    torch.save(dict(synth_sd), path)
    m = fid.FIDInception.from_file(str(path))
    assert torch.equal(m.Mixed_7c.branch_pool.conv.weight, synth_sd["Mixed_7c.branch_pool.conv.weight"])


def test_folded_conv_equals_conv_then_bn():
    g = torch.Generator().manual_seed(5)
    for k, p in (((3, 3), (1, 1)), ((1, 7), (0, 3)), ((7, 1), (3, 0)), ((1, 1), (0, 0))):
        bc = fid.BasicConv2d(16, 24, k, padding=p)
        bc.conv.weight.data.copy_(torch.randn(bc.conv.weight.shape, generator=g))
        bc.bn.weight.data.copy_(torch.rand(24, generator=g) + 0.5)
        bc.bn.bias.data.copy_(torch.randn(24, generator=g))
        bc.bn.running_mean.copy_(torch.randn(24, generator=g))
        bc.bn.running_var.copy_(torch.rand(24, generator=g) * 3 + 0.01)
        w, b = bc.folded()
        assert w.dtype == torch.float32 and b.dtype == torch.float32
        x = torch.randn((2, 16, 11, 13), generator=g, dtype=torch.float64)
        ref = F.batch_norm(F.conv2d(x, bc.conv.weight.double(), padding=p), bc.bn.running_mean.double(), bc.bn.running_var.double(),
                           bc.bn.weight.double(), bc.bn.bias.double(), training=False, eps=0.001)
        got = F.conv2d(x, w.double(), b.double(), padding=p)
        # the only difference is the fp32 rounding of the folded weight and bias
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
        sc = bc.bn.weight.double() / torch.sqrt(bc.bn.running_var.double() + 0.001)
        assert torch.equal(w, (bc.conv.weight.double() * sc.view(-1, 1, 1, 1)).float())
        assert torch.equal(b, (bc.bn.bias.double() - bc.bn.running_mean.double() * sc).float())


def test_synthetic_weights_keep_activations_order_one(synth_sd):
    """The synthetic network's features are O(1) (the benchmark and the GPU tests use it), and deterministic."""
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (2, 256, 256, 3), generator=g, dtype=torch.uint8).numpy()
    f = ref_features(synth_sd, ref_inputs(u8))
    assert f.shape == (2, 2048)
    assert 0.05 < float(f.abs().mean()) < 20 and float(f.abs().max()) < 200
    assert torch.equal(fid.FIDInception.synthetic(0).state_dict()["Mixed_5b.branch1x1.conv.weight"], synth_sd["Mixed_5b.branch1x1.conv.weight"])


def _spd(n, seed, cond=10.0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (q * np.geomspace(1.0, 1.0 / cond, n)) @ q.T


def test_frechet_against_the_eigenvalue_formula():
    rng = np.random.default_rng(0)
    for n in (3, 16, 64):
        s1, s2 = _spd(n, 1 + n), _spd(n, 2 + n, cond=100.0)
        mu1, mu2 = rng.standard_normal(n), rng.standard_normal(n)
        w, v = np.linalg.eigh(s1)
        r1 = (v * np.sqrt(w)) @ v.T                                # S1^1/2
        tr = float(np.sum(np.sqrt(np.linalg.eigvalsh(r1 @ s2 @ r1))))
        want = float(np.sum((mu1 - mu2) ** 2) + np.trace(s1) + np.trace(s2) - 2 * tr)
        got = fid.frechet_distance(mu1, s1, mu2, s2)
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (n, got, want)


def test_frechet_equal_statistics_is_zero():
    s = _spd(32, 7)
    mu = np.random.default_rng(3).standard_normal(32)
    assert abs(fid.frechet_distance(mu, s, mu, s)) < 1e-8


def test_frechet_eps_retry_and_complex_error(capsys):
    # sigma1 sigma2 nilpotent: sqrtm has no finite value, the eps * I retry makes it triangular with a positive diagonal
    s1, s2 = np.array([[0.0, 1.0], [0.0, 0.0]]), np.eye(2)
    mu = np.zeros(2)
    with np.errstate(all="ignore"):
        d = fid.frechet_distance(mu, s1, mu, s2)
    assert "adding 1e-06 to diagonal" in capsys.readouterr().out
    e = 1e-6
    assert np.isfinite(d) and abs(d - (0.0 + 2.0 - 2 * 2 * np.sqrt(e * (1 + e)))) < 1e-12
    # a negative eigenvalue of sigma1 sigma2: the diagonal of sqrtm is imaginary
    with pytest.raises(ValueError, match="Imaginary component"):
        fid.frechet_distance(mu, np.diag([1.0, -1.0]), mu, np.eye(2))


@pytest.mark.parametrize("shape", [(255, 255), (256, 256), (383, 383), (511, 700), (1365, 2048)])
def test_patch_origins_reproduce_the_cropper(shape):
    from calc_metrics import crop_hific_fid_patches, hific_patch_origins
    H, W = shape
    rng = np.random.default_rng(H * 7 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    p = 256
    o = hific_patch_origins(H, W, p)
    patches = crop_hific_fid_patches(img, p)
    assert o.shape == (len(patches), 2)
    for (y0, x0), q in zip(o, patches):
        assert np.array_equal(img[y0:y0 + p, x0:x0 + p], q)
    # the cropper's own rule, written out: the p x p grid of the image, then that of the image shifted by p // 2
    s = p // 2
    n = (H // p) * (W // p) + ((H - s) // p) * ((W - s) // p)
    assert len(patches) == n


def test_calc_metrics_fid_needs_50_pairs(tmp_path, capsys):
    """With --inception_path and fewer than 50 pairs, FID is left out with the reference's message and the keys keep its order."""
    from PIL import Image
    import calc_metrics
    real, fake = tmp_path / "real", tmp_path / "fake"
    real.mkdir(); fake.mkdir()
    rng = np.random.default_rng(0)
    for i in range(3):
        a = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
        Image.fromarray(a).save(real / f"{i}.png")
        Image.fromarray(np.clip(a.astype(int) + 3, 0, 255).astype(np.uint8)).save(fake / f"{i}.png")
    with open(fake / "_avg_bitrate.json", "w") as f:
        json.dump({"avg_bpp": 0.25}, f)
    w = tmp_path / "inception.pth"
    torch.save(fid.FIDInception.synthetic(0).state_dict(), w)
    out = calc_metrics.main(["--real_dir", str(real), "--fake_dir", str(fake), "--inception_path", str(w)])
    err = capsys.readouterr().err
    assert "num_img (=3) is too small to calc FID" in err
    assert list(out) == ["bpp", "PSNR"]
    with open(fake / "_metrics.json") as f:
        assert list(json.load(f)) == ["bpp", "PSNR"]
    # a bad weights file is refused before any image is read
    bad = tmp_path / "bad.pth"
    torch.save({"Conv2d_1a_3x3.conv.weight": torch.zeros(32, 3, 3, 3)}, bad)
    with pytest.raises(ValueError, match="lacks"):
        calc_metrics.main(["--real_dir", str(tmp_path / "nowhere"), "--fake_dir", str(fake), "--inception_path", str(bad)])
