"""HiFiC patch FID on the MI355X (dc_vic_amd.fid, csrc/fid.hip) against fp64: the patch resize, the Inception pools, the fp64 feature
statistics, FID-Inception's features against the plain-torch fp64 restatement of tests/test_fid_host.py, batch invariance, FID end to end
against the host pipeline, and both scripts with --inception_path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dc_vic_amd import fid
from test_fid_host import ref_features, ref_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
DEV = "cuda:0"
# features of 8 patches against the fp64 restatement, relative to max |feature|: ~10x the worst error measured on the MI355X
# (2.2e-6 absolute at max |feature| 4.0 with the synthetic weights: 5.6e-7)
FEAT_RTOL = 6e-6


@pytest.fixture(scope="module", autouse=True)
def _device():
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def model():
    return fid.FIDInception.synthetic(0).to(DEV)


def _ulps(got: torch.Tensor, want64: torch.Tensor, floor: float = 0.0) -> float:
    """Error in fp32 ulps of the fp64 value (ulps of `floor` where |value| < floor)."""
    w = torch.maximum(want64.abs(), torch.tensor(floor, dtype=torch.float64)).float()
    ulp = (torch.nextafter(w, torch.tensor(float("inf"))) - w).double()
    return float(((got.double() - want64).abs() / ulp).max())


# ------------------------------------------------------------------------------------------------ patch -> network input
@pytest.mark.parametrize("ph,pw", [(256, 256), (64, 64), (300, 300), (97, 131)])
def test_patch_resize_against_fp64(ph, pw):
    rng = np.random.default_rng(ph * 1000 + pw)
    H, W = 317, 401
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[:20, :20] = 0
    img[-20:, -20:] = 255
    org = np.array([[0, 0], [H - ph, W - pw], [7, 13], [(H - ph) // 2, 1]])
    dimg = torch.from_numpy(img).to(DEV)
    o = torch.from_numpy(fid.check_origins(org, H, W, ph, pw)).to(DEV)
    got = fid.patch_inputs(dimg, o, ph, pw).cpu()
    want = ref_inputs(np.stack([img[y:y + ph, x:x + pw] for y, x in org]))
    assert got.shape == want.shape == (4, 3, 299, 299)
    # computed in fp64 and rounded once: within one ulp of the fp64 value (ulps of 2^-20 below that, where 2 x - 1 cancels)
    assert _ulps(got, want, floor=2.0 ** -20) <= 1.0
    # a slice of a wider batch buffer: the other slots stay untouched
    buf = torch.full((7, 3, 299, 299), 7.0, device=DEV)
    fid.patch_inputs(dimg, o, ph, pw, out=buf[2:6])
    assert torch.equal(buf[2:6].cpu(), got) and bool((buf[:2] == 7).all()) and bool((buf[6:] == 7).all())
    with pytest.raises(ValueError):
        fid.check_origins(np.array([[H - ph + 1, 0]]), H, W, ph, pw)


# ------------------------------------------------------------------------------------------------ pools
_POOLS = {fid.POOL_MAX_S2: lambda x: F.max_pool2d(x, 3, 2), fid.POOL_AVG: lambda x: F.avg_pool2d(x, 3, 1, 1, count_include_pad=False),
          fid.POOL_MAX_S1: lambda x: F.max_pool2d(x, 3, 1, 1)}


@pytest.mark.parametrize("hw", [147, 71, 35, 17, 8])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("mode", sorted(_POOLS))
def test_pools_against_fp64(hw, n, mode):
    C = 6
    g = torch.Generator().manual_seed(hw * 10 + n + 100 * mode)
    x = torch.randn((n, C + 3, hw, hw), generator=g) * 2
    xd = x.to(DEV)[:, 2:2 + C]                                  # a channel slice of a wider tensor as the input
    want = _POOLS[mode](x[:, 2:2 + C].double())
    Ho = want.shape[2]
    wide = torch.full((n, C + 5, Ho, Ho), 123.0, device=DEV)
    y = fid.pool3(xd, mode, out=wide[:, 1:1 + C])               # ... and as the output
    got = y.cpu()
    if mode == fid.POOL_AVG:
        assert _ulps(got, want) <= 1.0
    else:
        assert torch.equal(got, want.float())
    w = wide.cpu()
    assert bool((w[:, :1] == 123).all()) and bool((w[:, 1 + C:] == 123).all())
    for k in range(n):                                          # per image, dense, alone
        assert torch.equal(fid.pool3(xd[k:k + 1].contiguous(), mode).cpu(), got[k:k + 1])


@pytest.mark.parametrize("hw", [8, 17, 35])
def test_global_mean_against_fp64(hw):
    g = torch.Generator().manual_seed(hw)
    x = torch.randn((3, 2048 + 4, hw, hw), generator=g).abs()
    xd = x.to(DEV)[:, 4:]
    out = torch.full((3, 2048 + 2), -1.0, device=DEV)
    y = fid.mean_hw(xd, out=out[:, 1:1 + 2048]).cpu()
    assert _ulps(y, x[:, 4:].double().mean(dim=(2, 3))) <= 1.0
    o = out.cpu()
    assert bool((o[:, 0] == -1).all()) and bool((o[:, -1] == -1).all())


# ------------------------------------------------------------------------------------------------ statistics
def test_stats_against_numpy():
    g = torch.Generator().manual_seed(11)
    batches = [torch.randn((b, 2048), generator=g).abs() * 0.7 for b in (37, 100, 1, 64, 5)]
    runs = []
    for _ in range(2):
        st = fid.FIDStats(DEV)
        for b in batches:
            wide = torch.zeros((b.shape[0], 2048 + 8), device=DEV)
            wide[:, 3:3 + 2048] = b.to(DEV)
            st.add(wide[:, 3:3 + 2048])                         # a row-strided view
        torch.cuda.synchronize()
        runs.append((st.sum.cpu(), st.gram.cpu(), st.mu_sigma()))
    allf = torch.cat(batches).double().numpy()
    mu, sigma = runs[0][2]
    assert runs[0][2][0].shape == (2048,) and sigma.shape == (2048, 2048)
    assert np.max(np.abs(mu - np.mean(allf, axis=0))) <= 1e-12 * np.max(np.abs(mu))
    ref = np.cov(allf, rowvar=False)
    assert np.max(np.abs(sigma - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert np.array_equal(sigma, sigma.T)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])     # identical bits run to run
    assert bool((torch.tril(runs[0][1], -1) == 0).all())                                  # only the upper triangle is written


# ------------------------------------------------------------------------------------------------ network
def _patches(n, seed, p=256):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, p // 8, p // 8, 3)).repeat(8, 1).repeat(8, 2)    # smooth-ish blocks plus noise, like image content
    return np.clip(base + rng.integers(-20, 21, (n, p, p, 3)), 0, 255).astype(np.uint8)


def _features(model, u8):
    x = torch.from_numpy(np.ascontiguousarray(u8)).to(DEV)
    B, p = u8.shape[0], u8.shape[1]
    img = x.reshape(B * p, p, 3)                                # the patches stacked as one tall image
    o = torch.from_numpy(fid.check_origins(np.stack([np.arange(B) * p, np.zeros(B, int)], 1), B * p, p, p, p)).to(DEV)
    return model.features(fid.patch_inputs(img.contiguous(), o, p))


def test_features_against_fp64(model):
    u8 = _patches(8, 1)
    got = _features(model, u8).cpu().double()
    want = ref_features(fid.FIDInception.synthetic(0).state_dict(), ref_inputs(u8))
    err = float((got - want).abs().max())
    scale = float(want.abs().max())
    print(f"[fid] features vs fp64: max abs err {err:.3e}, max |feature| {scale:.3e}, relative {err / scale:.3e}")
    assert err <= FEAT_RTOL * scale


def test_features_batch_invariant(model):
    u8 = _patches(100, 2)
    f100 = _features(model, u8).cpu()
    rev = _features(model, u8[::-1].copy()).cpu()
    assert torch.equal(f100, rev.flip(0))                       # every patch at another position of the batch
    for k in (0, 37, 99):
        assert torch.equal(_features(model, u8[k:k + 1]).cpu(), f100[k:k + 1])
    assert torch.equal(_features(model, u8[10:23]).cpu(), f100[10:23])


# ------------------------------------------------------------------------------------------------ end to end
def _write_pairs(tmp_path, n, seed, identical=False):
    from PIL import Image
    real, fake = tmp_path / "real", tmp_path / "fake"
    real.mkdir(); fake.mkdir()
    rng = np.random.default_rng(seed)
    for i in range(n):
        h, w = (int(v) for v in rng.integers(256, 601, 2))
        a = np.clip(rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3)).repeat(16, 0).repeat(16, 1)[:h, :w]
                    + rng.integers(-10, 11, (h, w, 3)), 0, 255).astype(np.uint8)
        b = a if identical else np.clip(a.astype(int) + rng.integers(-25, 26, a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(real / f"{i:03}.png")
        Image.fromarray(b).save(fake / f"{i:03}.png")
    (fake / "_avg_bitrate.json").write_text(json.dumps({"avg_bpp": 0.5}))
    return real, fake


def test_fid_end_to_end_against_host_pipeline(model, tmp_path):
    import calc_metrics as cm
    real, fake = _write_pairs(tmp_path, 60, 3)
    rp, fp = cm.get_real_fake_path_list(str(real), str(fake))
    got = cm.fid_metric(model, rp, fp, DEV)
    # host pipeline: features downloaded, np.mean / np.cov, the same Frechet function
    stats = []
    for paths in (fp, rp):
        feats = []
        pf = fid.PatchFeatures(model, DEV, 100, 256)
        n = pf.run(((cm.read_u8(q), cm.hific_patch_origins(*cm.read_u8(q).shape[:2], 256)) for q in paths),
                   lambda f: feats.append(f.cpu().double().numpy()))
        f = np.concatenate(feats)
        assert len(f) == n == sum(len(cm.crop_hific_fid_patches(cm.read_u8(q), 256)) for q in paths)
        stats.append((f.mean(0), np.cov(f, rowvar=False)))
    want = fid.frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1])
    print(f"[fid] end to end: device statistics {got:.10g}, host statistics {want:.10g}")
    assert abs(got - want) <= 1e-6 * abs(want)


def test_fid_identical_folders(model, tmp_path):
    import calc_metrics as cm
    real, fake = _write_pairs(tmp_path, 50, 4, identical=True)
    rp, fp = cm.get_real_fake_path_list(str(real), str(fake))
    (m1, s1), (m2, s2) = cm.fid_statistics(model, fp, DEV), cm.fid_statistics(model, rp, DEV)
    assert np.array_equal(m1, m2) and np.array_equal(s1, s2)        # same pixels, same bits
    d = fid.frechet_distance(m1, s1, m2, s2)
    # fewer patches (~150) than 2048 features: sigma is singular, and scipy's sqrtm of sigma^2 is accurate only to ~sqrt(eps) on its
    # null space, so FID is not 0 but noise of order 1e-6 of tr(sigma1) + tr(sigma2) (pytorch-fid computes the same).  Measured on the
    # MI355X: -1.55e-6 at tr(sigma) = 1.10 (7e-7 of the scale); the bound is ~10x that, relative to the scale
    print(f"[fid] identical folders: FID {d:.3e}, tr sigma {np.trace(s1):.3e}")
    assert abs(d) <= 1e-5 * (np.trace(s1) + np.trace(s2))


def test_calc_metrics_cli_with_inception(model, tmp_path):
    real, fake = _write_pairs(tmp_path, 50, 5)
    w = tmp_path / "inception.pth"
    torch.save(fid.FIDInception.synthetic(0).state_dict(), w)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "calc_metrics.py"), "--real_dir", str(real), "--fake_dir", str(fake),
           "--inception_path", str(w)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads((fake / "_metrics.json").read_text())
    assert list(out) == ["bpp", "PSNR", "FID"]
    assert np.isfinite(out["FID"]) and out["FID"] > 0
    assert "FID skipped" not in res.stderr and "LPIPS skipped" in res.stderr


def test_beta_selection_with_inception(tmp_path):
    import pandas as pd
    from PIL import Image
    root = tmp_path / "data"
    root.mkdir()
    rng = np.random.default_rng(6)
    for i in range(50):
        Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(root / f"{i:02}.png")
    sdir = tmp_path / "search"
    sdir.mkdir()
    for bv, br in {3.0: 1.5, 2.0: 0.75}.items():
        pd.DataFrame([{"run_cnt": 1, "beta_vq": bv, "beta_rate": br, "avg_bpp": 0.2004, "diff": 0.0004}]).to_csv(
            sdir / f"result_beta_vq_{bv:.2f}_target_rate_0.200.csv")
    w = tmp_path / "inception.pth"
    torch.save(fid.FIDInception.synthetic(0).state_dict(), w)
    sel = tmp_path / "selection"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "beta_selection.py"), os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"),
           "--search_dir", str(sdir), "--save_dir", str(sel), "--dataset_root", str(root), "--beta_vq", "3.0", "2.0", "--target_rate", "0.2",
           "--batch_size", "8", "--synthetic_weights", "--inception_path", str(w)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("statistics of the 50 real images computed") == 1      # once for both settings
    df = pd.read_csv(sel / "target_rate_0.2" / "result.csv", index_col=0)
    assert len(df) == 2 and np.isfinite(df["fid"]).all() and (df["fid"] > 0).all()
    assert np.allclose(df["score"], 2.0 * df["psnr"] - df["fid"], rtol=0, atol=1e-9)
