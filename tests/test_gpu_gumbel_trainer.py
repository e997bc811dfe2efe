"""model.gumbel_sampling in the GAN-stage trainers: the gradient the image losses send into the VQ estimator, the full G + D step,
the noise generator's place in the training state, and the CLI -- against torch autograd over the CPU oracle composed with
tests/gumbel_ref.py (tests/gumbel_step_ref.py), at test_gpu_train.py's step sizes and bounds.

The draws of the oracle comparisons are seeded on the CPU and handed to the trainer (`draw_gumbel_noise` replaced on the instance), so
that the restatement can be run alone first: for x seed 90 and noise seed 44 every sampled index of the oracle sits 0.04 or more of
logits - log e away from the runner-up at both sizes (logits reach 38 there), so no sample can legitimately differ; a difference in the
rounded symbols goes through analysis_train_ref.tie_report.  The resume and CLI tests use the trainer's own device generator."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gumbel_step_ref as S
from analysis_train_ref import tie_report
from test_gpu_oasis import _oasis_disc
from test_gpu_train import DEV, ROOT, _disc, relclose

pytestmark = pytest.mark.gpu

CASES = {"2x64x64": ((2, 3, 64, 64), [2.29, 0.62], [3.0, 1.5]), "1x64x128": ((1, 3, 64, 128), [1.51], [2.25])}
X_SEED, E_SEED = 90, 44
IMAGE_LOSSES_ONLY = dict(distortion=50.0, perceptual=1.0, gan=0.01, code_distortion=0.0, code_ce=0.0)


@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


@pytest.fixture
def restored(model):
    """The shared model, with its synthetic weights put back (and every cached plan dropped) after the test."""
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    yield model
    model.load_state_dict(before)
    for m in model.modules():
        if hasattr(m, "_plan"):
            m._plan = None
        if hasattr(m, "_qkv_plan"):
            m._qkv_plan = None
        if hasattr(m, "invalidate_caches"):
            m.invalidate_caches()


def inputs(case):
    shape, b1, b2 = CASES[case]
    x = torch.rand(shape, generator=torch.Generator().manual_seed(X_SEED)) * 2 - 1
    e = torch.empty((shape[0], 256, shape[2] // 8, shape[3] // 8)).exponential_(generator=torch.Generator().manual_seed(E_SEED))
    return x, torch.tensor(b1), torch.tensor(b2), e


def fixed_noise(tr, e):
    dev_e = e.to(DEV)

    def draw(logits):
        assert tuple(logits.shape) == tuple(dev_e.shape)
        return dev_e
    tr.draw_gumbel_noise = draw


def oracle_step(synth_sd, tr, D, x, b1, b2, e, tau, w, o):
    """The oracle's losses and gradients on the product's decisions (sampled index, rounded symbols), after tie_report has allowed
    the differences: -> (L, oo, sd, names)."""
    from oracle import train_oracle as T
    from oracle.entropy_oracle import EntropyBottleneckOracle
    eb = EntropyBottleneckOracle(synth_sd, "entropy_model_z")
    lsd = {k: v.detach().cpu().clone() for k, v in tr.lpips.state_dict().items()} if tr.lpips is not None else None
    dsd = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}

    def run(**force):
        sd = {k: v.clone() for k, v in synth_sd.items()}
        names = [k for k in sd if k.startswith(T.TRAINABLE_PREFIXES) and sd[k].is_floating_point()]
        for k in names:
            sd[k].requires_grad_(True)
        L, oo = S.generator_losses(sd, dsd, x, b1, b2, eb, e, tau, w=w, lsd=lsd, **force)
        sum(L.values()).backward()
        return L, oo, sd, names
    L, oo, sd, names = run()
    idx_p, yh_p = o["sample_idx"].cpu(), o["y_hat"].data.cpu()
    # the sampled index: a difference must sit within 1e-4 of a tie of logits - log e; the symbols: within 1e-4 of a half-integer
    n_i, worst_i, cap_i = tie_report(oo["own_sample_idx"], idx_p, oo["sample_gap"])
    d_sym = (yh_p - oo["y_hat"]).abs() > 0.5
    n_s, cap_s = int(d_sym.sum()), max(1, int(1e-5 * yh_p.numel()))
    print(f"[gumbel step] sampled indices differing from the restatement's own: {n_i} (cap {cap_i}, worst gap {worst_i:.3e}); symbols: {n_s} (cap {cap_s})")
    assert n_i <= cap_i and worst_i <= 1e-4 and n_s <= cap_s
    if n_s:
        assert float((yh_p - oo["y_hat"])[d_sym].abs().max()) <= 1.0 + 1e-4
    if n_i or n_s:
        L, oo, sd, names = run(force_y_hat=yh_p, force_sample_idx=idx_p)
    return L, oo, sd, names


def product_forward(tr, x, b1, b2):
    """generator_forward with the sampled index recorded beside the trainer's outputs."""
    from dc_vic_amd.train import autograd as A
    seen = {}
    real_op = A.gumbel_vq_latent

    def spy(*a, **k):
        idx, lat = real_op(*a, **k)
        seen["idx"] = idx
        return idx, lat
    A.gumbel_vq_latent = spy
    try:
        tr.g_group.zero_grad()
        ctx = A.Ctx([tr.g_group])
        o = tr.generator_forward(ctx, x, None, b1, b2)
    finally:
        A.gumbel_vq_latent = real_op
    o["sample_idx"] = seen["idx"]
    return ctx, o


@pytest.mark.parametrize("case", list(CASES))
def test_image_losses_reach_the_estimator(model, synth_sd, case):
    """code_ce and code_distortion at weight 0: every gradient of the VQ estimator comes from the distortion, perceptual and
    adversarial losses through the sampled latent.  With argmax it is exactly zero; here it equals torch autograd over the oracle."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    x, b1, b2, e = inputs(case)
    D = _disc().to(DEV)
    tr = DualBetaCondGanDistortionVqCodeTrainer(model, D, clip_max_norm=1.0, seed=3, loss_weights=IMAGE_LOSSES_ONLY, gumbel_sampling=True,
                                                gumbel_kwargs=dict(tau=1.0))
    fixed_noise(tr, e)
    ctx, o = product_forward(tr, x, b1, b2)
    L, oo, sd, names = oracle_step(synth_sd, tr, D, x, b1, b2, e, 1.0, IMAGE_LOSSES_ONLY, o)
    assert torch.equal(o["out_vq_indices"].cpu(), oo["out_idx"]) and torch.equal(o["sample_idx"].cpu(), oo["sample_idx"])
    assert not torch.equal(o["sample_idx"], o["out_vq_indices"])            # the draw moved some positions off the argmax
    relclose(o["fake"].data, oo["fake"], 2e-4, "fake images")
    glog = tr.calc_g_loss(ctx, o, b1, b2)
    assert float(glog["code_ce"].item()) == 0.0 and float(glog["code_distortion"].item()) == 0.0
    ctx.backward()
    own = dict(model.named_parameters())
    est = [k for k in names if k.startswith("vq_estimator.") and sd[k].grad is not None and float(sd[k].grad.abs().max()) > 0]
    assert len(est) >= 100, len(est)
    worst = 0.0
    for k in est:
        gp = tr.g_group.grad_of(own[k])
        assert float(gp.abs().max()) > 0.0, k
        worst = max(worst, relclose(gp, sd[k].grad, 3e-3, f"estimator grad {k}"))
    print(f"[gumbel step] {case}: {len(est)} estimator gradients from the image losses alone, worst relative error {worst:.3e}")
    # the same trainer with the option off: the estimator's trunk gets no gradient at all (embed_projection is not on this path either)
    off = DualBetaCondGanDistortionVqCodeTrainer(model, D, clip_max_norm=1.0, seed=3, loss_weights=IMAGE_LOSSES_ONLY)
    assert off.gumbel_sampling is False and off.gumbel_gen is None
    from dc_vic_amd.train import autograd as A
    off.g_group.zero_grad()
    c2 = A.Ctx([off.g_group])
    off.calc_g_loss(c2, off.generator_forward(c2, x, None, b1, b2), b1, b2)
    c2.backward()
    assert all(float(off.g_group.grad_of(own[k]).abs().max()) == 0.0 for k in est)


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("case", list(CASES))
def test_full_step_with_the_option_on(model, synth_sd, case, tau):
    """Every loss term within 2e-4 and every generator parameter gradient within 3e-3 of its tensor's max, with the default weights."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    from dc_vic_amd.train.trainer import DEFAULT_LOSS
    x, b1, b2, e = inputs(case)
    D = _disc().to(DEV)
    tr = DualBetaCondGanDistortionVqCodeTrainer(model, D, clip_max_norm=1.0, seed=3, gumbel_sampling=True, gumbel_kwargs=dict(tau=tau))
    assert tr.gumbel_tau == tau
    fixed_noise(tr, e)
    ctx, o = product_forward(tr, x, b1, b2)
    L, oo, sd, names = oracle_step(synth_sd, tr, D, x, b1, b2, e, tau, DEFAULT_LOSS, o)
    assert torch.equal(o["gt_vq_indices"].cpu(), oo["gt_idx"]) and torch.equal(o["out_vq_indices"].cpu(), oo["out_idx"])
    assert torch.equal(o["sample_idx"].cpu(), oo["sample_idx"])
    relclose(o["fake"].data, oo["fake"], 2e-4, "fake images")
    glog = tr.calc_g_loss(ctx, o, b1, b2)
    for k in ("distortion", "perceptual", "adv", "code_distortion", "code_ce"):
        relclose(glog[k], L[k].detach().reshape(1), 2e-4, f"loss {k}")
    ctx.backward()
    own = dict(model.named_parameters())
    worst, checked = 0.0, 0
    for k in names:
        if sd[k].grad is None:
            assert float(tr.g_group.grad_of(own[k]).abs().max()) == 0.0, k
            continue
        worst = max(worst, relclose(tr.g_group.grad_of(own[k]), sd[k].grad, 3e-3, f"grad {k}"))
        checked += 1
    assert checked >= 400, checked
    print(f"[gumbel step] {case} tau {tau:g}: {checked} parameter gradients, worst relative error {worst:.3e}")


def test_constant_noise_gives_the_argmax_paths_fake(model):
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    from dc_vic_amd.train import autograd as A
    x, b1, b2, e = inputs("2x64x64")
    D = _disc().to(DEV)
    on = DualBetaCondGanDistortionVqCodeTrainer(model, D, seed=3, gumbel_sampling=True)
    fixed_noise(on, torch.ones_like(e))
    off = DualBetaCondGanDistortionVqCodeTrainer(model, D, seed=3, gumbel_sampling=False)
    ctx, o = product_forward(on, x, b1, b2)
    o2 = off.generator_forward(A.Ctx([off.g_group]), x, None, b1, b2)
    assert torch.equal(o["sample_idx"], o2["out_vq_indices"]) and torch.equal(o["out_vq_indices"], o2["out_vq_indices"])
    assert torch.equal(o["fake"].data, o2["fake"].data)


def _three_steps(tr, x):
    logs = [tr.optimize_parameters(i + 1, {"real_images": x}) for i in range(3)]
    assert all(lg is not None and all(np.isfinite(v) for v in lg.values()) for lg in logs), logs
    return logs


def _snapshot(model, D):
    return {k: v.detach().clone() for k, v in list(model.state_dict().items()) + [("D." + k, v) for k, v in D.state_dict().items()]}


def test_option_off_changes_nothing(restored):
    """A seeded 3-step run with the trainer arguments of before this option equals, bit for bit, the same run with gumbel_sampling=False
    spelled out and with the model's attribute read (None): logs, generator and discriminator weights; no new key in the training state;
    no generator exists."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    model = restored
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(92)) * 2 - 1
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    runs = []
    for kw in (dict(), dict(gumbel_sampling=False, gumbel_kwargs=dict(tau=0.5)), dict(gumbel_sampling=None, gumbel_kwargs=None)):
        model.load_state_dict(start)
        D = _disc(7).to(DEV)
        tr = DualBetaCondGanDistortionVqCodeTrainer(model, D, seed=11, **kw)
        tr.resync_parameters()
        assert tr.gumbel_gen is None and tr.gumbel_sampling is False
        logs = _three_steps(tr, x)
        assert sorted(tr.training_state(3)) == ["d", "g", "iter", "rng"]
        runs.append((logs, _snapshot(model, D)))
    for logs, snap in runs[1:]:
        assert logs == runs[0][0]
        assert all(torch.equal(snap[k], runs[0][1][k]) for k in snap)
    assert model.gumbel_sampling is False and model.gumbel_kwargs == {}


def test_resume_vq_acc_and_validation_with_the_option_on(restored, tmp_path):
    """Save at step 2, resume in a new trainer, and step 3 has the uninterrupted run's bits; a validation call in between draws nothing
    from gumbel_gen; vq_acc is the argmax's accuracy, not the sample's."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    model = restored
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(92)) * 2 - 1
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    mk = lambda D: DualBetaCondGanDistortionVqCodeTrainer(model, D, seed=11, gumbel_sampling=True, gumbel_kwargs=dict(tau=0.5))
    # ---- uninterrupted
    D = _disc(7).to(DEV)
    tr = mk(D)
    assert tr.gumbel_gen is not None and tr.gumbel_gen.device.type == "cuda" and tr.gumbel_tau == 0.5
    logs = _three_steps(tr, x)
    want = _snapshot(model, D)
    assert "gumbel_gen" in tr.training_state(3)
    # ---- two steps, save, a validation, resume elsewhere, the third step
    model.load_state_dict(start)
    D1 = _disc(7).to(DEV)
    t1 = mk(D1)
    t1.resync_parameters()
    first = [t1.optimize_parameters(i + 1, {"real_images": x}) for i in range(2)]
    assert first == logs[:2]
    path = str(tmp_path / "training_state_iter0000002.pth.tar")
    torch.save(t1.training_state(2), path)
    saved_model, saved_d = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, {k: v.detach().cpu().clone() for k, v in D1.state_dict().items()}
    gen_state = t1.gumbel_gen.get_state().clone()
    from dc_vic_amd.train.validation import load_eval_images
    res = t1.validation(2, load_eval_images(os.path.join(ROOT, "tests", "golden", "demo_images"))[:1])
    assert res and torch.equal(t1.gumbel_gen.get_state(), gen_state)
    model.load_state_dict(start)                                            # a fresh process would start from other weights
    D2 = _disc(9).to(DEV)
    t2 = mk(D2)
    t2.gumbel_gen.manual_seed(12345)
    model.load_state_dict(saved_model)
    D2.load_state_dict(saved_d)
    t2.resync_parameters()
    assert t2.load_training_state(torch.load(path, map_location="cpu", weights_only=False)) == 2
    third = t2.optimize_parameters(3, {"real_images": x})
    assert third == logs[2]
    got = _snapshot(model, D2)
    assert all(torch.equal(got[k], want[k]) for k in want)
    # vq_acc: from the argmax of the logits
    ctx, o = product_forward(t2, x, t2.last_beta_rate, t2.last_beta_vq)
    acc = float((o["out_vq_indices"] == o["gt_vq_indices"]).float().mean().item())
    assert torch.equal(o["out_vq_indices"], o["logits"].data.argmax(1)) and not torch.equal(o["sample_idx"], o["out_vq_indices"])
    assert 0.0 <= acc <= 1.0
    # a state saved without the option cannot resume a run with it
    off = DualBetaCondGanDistortionVqCodeTrainer(model, D2, seed=11)
    with pytest.raises(ValueError, match="gumbel_gen"):
        t2.load_training_state(off.training_state(3))
    # the keywords are the trainer's contract too
    with pytest.raises(ValueError, match=r"model\.gumbel_kwargs\.hard"):
        DualBetaCondGanDistortionVqCodeTrainer(model, D2, seed=11, gumbel_sampling=True, gumbel_kwargs=dict(hard=False))


def test_trainer_reads_the_models_attributes(restored):
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    model = restored
    D = _disc(7).to(DEV)
    model.gumbel_sampling, model.gumbel_kwargs = True, dict(tau=2.0)
    try:
        tr = DualBetaCondGanDistortionVqCodeTrainer(model, D, seed=11)
        assert tr.gumbel_sampling is True and tr.gumbel_tau == 2.0 and tr.gumbel_gen is not None
        assert DualBetaCondGanDistortionVqCodeTrainer(model, D, seed=11, gumbel_sampling=False).gumbel_gen is None
    finally:
        model.gumbel_sampling, model.gumbel_kwargs = False, {}


def test_oasis_trainer_takes_a_step_with_the_option_on(restored):
    from dc_vic_amd.train import DualBetaCondOasisGanDistortionVqFusionTrainer
    model = restored
    D = _oasis_disc().to(DEV)
    tr = DualBetaCondOasisGanDistortionVqFusionTrainer(model, D, seed=3, loss_weights=IMAGE_LOSSES_ONLY, gumbel_sampling=True)
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(90)) * 2 - 1
    w0 = model.vq_estimator.out_block[1].weight.detach().clone()
    log = tr.optimize_parameters(1, dict(real_images=x, beta_rate=torch.tensor([2.29, 0.62]), beta_vq=torch.tensor([3.0, 1.5])))
    assert log is not None and all(np.isfinite(v) for v in log.values()), log
    own = dict(model.named_parameters())
    est = [k for k in own if k.startswith("vq_estimator.swin_blks") and k.endswith("weight")]
    assert est and all(float(tr.g_group.grad_of(own[k]).abs().max()) > 0.0 for k in est)
    assert bool(torch.isfinite(tr.g_group.grad).all()) and not torch.equal(model.vq_estimator.out_block[1].weight, w0)


def test_train_cli_with_gumbel_sampling(tmp_path):
    cfg = tmp_path / "gumbel_synthetic.yaml"
    cfg.write_text(f"_base_: {os.path.join(ROOT, 'config', 'dc_vic_synthetic.yaml')}\nmodel:\n  gumbel_sampling: true\n  gumbel_kwargs:\n    tau: 0.5\n"
                   "loss:\n  perceptual_loss:\n    loss_weight: 0\n")
    base = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), str(cfg), "--synthetic_weights", "--synthetic_data", "--batch_size", "2", "--log_step", "1"]
    res = subprocess.run(base + ["--total_iter", "3"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("[train] VQ sampling:")]
    assert line == ["[train] VQ sampling: gumbel-softmax (tau 0.5)"], res.stdout
    its = [ln for ln in res.stdout.splitlines() if ln.startswith("iter")]
    assert len(its) == 3 and all("vq_acc" in ln and "nan" not in ln for ln in its), res.stdout
    # a keyword the sample cannot honour ends the run before the GPU is touched
    bad_cfg = tmp_path / "gumbel_bad.yaml"
    bad_cfg.write_text(cfg.read_text().replace("    tau: 0.5\n", "    hard: false\n"))
    bad = subprocess.run([base[0], base[1], str(bad_cfg)] + base[3:] + ["--total_iter", "1"], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert bad.returncode != 0 and "model.gumbel_kwargs.hard" in bad.stderr and "Traceback" not in bad.stderr, bad.stderr[-2000:]
