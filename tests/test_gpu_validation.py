"""The trainer's validation on the MI355X (synthetic weights, tests/golden/demo_images): run_model's out_vq_latent, the per-image rows
of HyperpriorDualCondVicModel.validation against a hand composition with the fp64 yardsticks of tests/test_ssim_host.py, validation
on the current weights, no effect on training, and scripts/train.py's --eval_step / --eval_dataset_root / eval_result.csv."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ssim import MS_SSIM_TOL  # noqa: E402
from test_ssim_host import ms_ssim_ref, psnr_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DEMO = os.path.join(ROOT, "tests", "golden", "demo_images")
CFG = os.path.join(ROOT, "config", "dc_vic_synthetic.yaml")


def _model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(CFG, {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


def _disc(seed=7):
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator
    torch.manual_seed(seed)
    D = DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, L=10, cond_ch=8,
                                              use_pi=False, include_x=True)
    g = torch.Generator().manual_seed(seed)
    for p in D.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
    return D.to(DEV)


@pytest.fixture(scope="module")
def images():
    from dc_vic_amd.train.validation import load_eval_images
    return load_eval_images(DEMO)


def test_run_model_returns_the_estimator_latent(images):
    from dc_vic_amd import ops
    m = _model()
    br, bv = 1.51, 2.25
    out = m.run_model(images[0], is_train=False, beta_rate=br, beta_vq=bv)
    x = m.img_preprocess(images[0], is_train=False)
    gt, gi, feat = m.vq_encode(x, None, want_feat=True)
    y = m.comp_encode(x, gt, gi, enc_kwargs=dict(beta_1=br, beta_2=bv), feat=feat)
    y_hat = m._entropy_encode_side(y, want_symbols=False)["y_hat"]
    N, _, yH, yW = y_hat.shape
    bufs = m.fusion_module.alloc_cat_buffers(N, 2 * yH, 2 * yW, y_hat.device)
    feat_out = {k: bufs[k][:, : m.fusion_module.fusion_modules[k].cond_ch] for k in bufs}
    feat_1, _ = m.decoder.get_feats(y_hat, beta_1=br, beta_2=bv, feat_out=feat_out)
    emb, logits = m.vq_estimator(feat_1, want_embed=True)
    assert out["out_vq_latent"].shape == out["gt_vq_latent"].shape
    assert torch.equal(out["out_vq_latent"], emb) and torch.equal(out["out_vq_logits"], logits)
    # the keys run_model returned before are unchanged: the decode without the embedding head gives the same image, indices, logits
    fake, idx, lg = m._decode(y_hat, 1.0, br, bv, want_logits=True)
    H, W = images[0].shape[2:]
    assert torch.equal(out["fake_images"], ops.crop_clamp(fake, H, W)) and torch.equal(out["out_vq_indices"], idx) and torch.equal(lg, logits)
    assert torch.equal(out["y_hat"], y_hat) and torch.equal(out["gt_vq_latent"], gt)
    assert set(out) == {"real_images", "fake_images", "y_hat", "z_hat", "bpp", "qbpp", "y_likelihood", "z_likelihood", "y_q_likelihood",
                        "z_q_likelihood", "gt_vq_latent", "gt_vq_indices", "out_vq_indices", "out_vq_logits", "out_vq_latent",
                        "vq_accuracy", "beta_rate", "beta_vq", "bits_per_image"}


def test_validation_rows_equal_a_hand_composition(images):
    m = _model()
    rows = m.validation(images, max_sample_size=100, beta_rate=2.29, beta_vq=3.0)
    assert [r["idx"] for r in rows] == [1, 2, 3]
    for img, r in zip(images, rows):
        out = m.run_model(img, is_train=False, beta_rate=2.29, beta_vq=3.0)
        real, fake = out["real_images"].cpu(), out["fake_images"].cpu()
        assert r["bpp"] == out["bpp"] and r["vq_acc"] == out["vq_accuracy"]
        assert abs(r["psnr"] - float(psnr_ref(real, fake)[0])) <= 1e-12
        assert abs(r["ms_ssim"] - float(ms_ssim_ref(real, fake)[0])) <= MS_SSIM_TOL
        d = out["out_vq_latent"].double() - out["gt_vq_latent"].double()
        ref = float((d * d).mean())
        assert abs(r["vq_mse"] - ref) <= 1e-6 * ref, (r["vq_mse"], ref)
    assert len(m.validation(images, max_sample_size=2, beta_rate=2.29, beta_vq=3.0)) == 2
    with pytest.raises(ValueError, match="1024"):
        m.validation([torch.zeros((1, 3, 64, 1040))], beta_rate=2.29, beta_vq=3.0)


def test_validation_runs_on_the_current_weights(images):
    """After 2 steps the trainer's validation equals, bit for bit, that of a fresh model loaded with the trained state dict: no stale
    packed weights, no stale graphs."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    m = _model()
    tr = DualBetaCondGanDistortionVqCodeTrainer(m, _disc(), seed=11)
    x = torch.rand((2, 3, 256, 256), generator=torch.Generator().manual_seed(91)) * 2 - 1
    v0 = tr.validation(0, images[:1])
    for it in (1, 2):
        assert tr.optimize_parameters(it, {"real_images": x}) is not None
    v2 = tr.validation(2, images[:1])
    assert list(v2) == ["idx0_bpp", "idx0_psnr", "idx0_ms_ssim", "idx0_vq_acc", "idx0_vq_mse"]
    assert v2 != v0
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m2 = _model()
    m2.load_state_dict(sd)
    v2b = DualBetaCondGanDistortionVqCodeTrainer(m2, _disc(), seed=11).validation(2, images[:1])
    assert v2b == v2


def _train(images, validate: bool, steps: int = 4):
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    m = _model()
    tr = DualBetaCondGanDistortionVqCodeTrainer(m, _disc(), seed=5)
    g = torch.Generator().manual_seed(17)
    logs = []
    for it in range(1, steps + 1):
        logs.append(tr.optimize_parameters(it, {"real_images": torch.rand((2, 3, 256, 256), generator=g) * 2 - 1}))
        if validate:
            tr.validation(it, images)
    return tr, logs


def test_validation_leaves_training_unchanged(images):
    ta, la = _train(images[:2], validate=True)
    tb, lb = _train(images[:2], validate=False)
    assert la == lb
    for grp in ("g_group", "d_group"):
        a, b = getattr(ta, grp), getattr(tb, grp)
        assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert ta.g_opt.t == tb.g_opt.t and ta.g_sched.last_epoch == tb.g_sched.last_epoch
    assert ta.rng.randint(0, 1 << 30) == tb.rng.randint(0, 1 << 30)


def test_train_cli_eval_csv_and_resume(tmp_path):
    from dc_vic_amd.train.lpips import LPIPSAlex
    lp = tmp_path / "lpips_alex.pth"
    torch.save({k: v.clone() for k, v in LPIPSAlex(seed=0).state_dict().items()}, lp)
    out, out2 = tmp_path / "run", tmp_path / "run2"
    base = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), CFG, "--synthetic_weights", "--synthetic_data", "--batch_size", "2",
            "--log_step", "1", "--total_iter", "4", "--eval_step", "2", "--eval_dataset_root", DEMO, "--lpips_path", str(lp)]
    res = subprocess.run(base + ["--save_dir", str(out), "--save_step", "2"], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert [ln.split(" (")[0] for ln in res.stdout.splitlines() if ln.startswith("validation")] == ["validation iter2", "validation iter4"]
    assert "\t idx0_ms_ssim: " in res.stdout
    rows = list(csv.reader(open(out / "eval_result.csv")))
    assert rows[0] == ["iter", "idx0_bpp", "idx0_psnr", "idx0_ms_ssim", "idx0_vq_acc", "idx0_vq_mse"]
    assert [r[0] for r in rows[1:]] == ["2", "4"]
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r[1:])
    ms = [float(r[3]) for r in rows[1:]]
    assert all(0.0 < v <= 1.0 for v in ms)
    res2 = subprocess.run(base + ["--save_dir", str(out2), "--resume", str(out / "training_state_iter0000002.pth.tar")], cwd=ROOT,
                          capture_output=True, text=True)
    assert res2.returncode == 0, res2.stderr[-2000:]
    assert open(out2 / "eval_result.csv").read() == open(out / "eval_result.csv").read()
