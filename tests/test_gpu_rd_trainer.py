"""The stage 1-2 rate-distortion trainer (train/rd_trainer.py) on a real MI355X: one whole step against torch autograd over the CPU
restatement of tests/rd_step_ref.py (analysis side in fp64, synthesis side and LPIPS in fp32, one graph; the losses in the reference
trainer's own words), the clipped Adam update, the aux step's ordering, batch invariance, determinism, the training-state round trip,
and the stage-3 trainer on the same model afterwards.

Inputs: 2 x 64x64 and 1 x 64x128, beta_rate [2.29, 0.62], beta_vq [3.0, 1.5], config/exp1_stage1_2.yaml's trainer and loss sections
(tests/golden/reference_loss_sections.json: beta policy exp, every reduction none), the synthetic weights with the scale transforms'
last biases raised (analysis_train_ref.shifted_state; under 0.1 % of the sigmas and likelihoods at a bound, asserted).
Bounds, those of the two existing step tests: 2e-4 of max for values and loss terms, 3e-3 of the tensor's max for every parameter
gradient.  Rounded symbols and the estimator's argmax are the product's, fed to the helper; those that differ from the helper's own
are capped by analysis_train_ref.tie_report (max(1, 1e-5 x decisions), within 1e-4 of a tie).

The sign of every ReLU input of the encoder, the hyperprior, CHARM and the decoder is a decision too (the networks are piecewise linear:
gradients are comparable only on the same piece): the product's ReLU outputs are recorded, the helper multiplies by their sign in place
of its own (rd_step_ref.ReluDecisions), every ReLU call of the helper must find its product tensor, and the signs that differ are
capped by the same tie_report over all ReLU inputs of the step (about 10^7), each within 1e-4 of zero.  Without it, one input at
6.7e-8 in the fp64 helper, on the other side of zero in the product's fp32 convolution, put decoder.block3.block1.conv.0.weight at
3.3e-3 of its max at 2 x 64x64 (one output channel: 1 of 96 bias entries, 69 of 18432 weights; profiles/rd_trainer_step_errors.log).

Set DCVIC_RD_ERRLOG=<file> to have the worst errors appended there."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import analysis_train_ref as AR
import rd_step_ref as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
VAL_TOL, GRAD_TOL = 2e-4, 3e-3
BETA_RATE, BETA_VQ = [2.29, 0.62], [3.0, 1.5]
CASES = {"2x64x64": ((2, 3, 64, 64), 71), "1x64x128": ((1, 3, 64, 128), 72)}


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def _log(line):
    print(line)
    path = os.environ.get("DCVIC_RD_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def section():
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        return json.load(f)["exp1_stage1_2.yaml"]


@functools.lru_cache(maxsize=None)
def cpu_state():
    from dc_vic_amd.synth import full_synth_state_dict
    return AR.shifted_state(full_synth_state_dict(1234))


def build_model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    have = set(m.state_dict())
    m.load_state_dict({k: v for k, v in cpu_state().items() if k in have}, strict=False)
    return m


def build_trainer(m, lr=1e-4, seed=3, **kw):
    """The trainer as scripts/train.py builds it from the YAML's sections (train/build.py), under the test's lr, seed and overrides."""
    from dc_vic_amd.train import DualBetaCondRateDistortionVqCodeTrainer
    from dc_vic_amd.train.build import rd_trainer_kwargs
    from dc_vic_amd.train.losses import read_loss_section
    args = dict(rd_trainer_kwargs(section(), read_loss_section(section())), lr=lr, seed=seed)
    args.update(kw)
    return DualBetaCondRateDistortionVqCodeTrainer(m, **args)


@functools.lru_cache(maxsize=None)
def bundle():
    m = build_model()
    return m, build_trainer(m)


@functools.lru_cache(maxsize=None)
def inputs(case):
    shape, seed = CASES[case]
    return AR.analysis_inputs(cpu_state(), shape, seed)


def data_dict(I, keep=slice(None)):
    d = lambda t: t[keep].contiguous().to(DEV)
    n = I["x"][keep].shape[0]
    return dict(real_images=d(I["x"]), vq_indices=d(I["idx"]), noise_y=d(I["noise_y"]), noise_z=d(I["noise_z"]),
                beta_rate=torch.tensor(BETA_RATE)[keep][:n], beta_vq=torch.tensor(BETA_VQ)[keep][:n])


def forward_backward(tr, dd, relu_outputs=None):
    """Forward, losses and backward of one step; with `relu_outputs` (a list) every output of a convolution with a fused ReLU is
    appended to it (the tape's ReLU gradient is taken from the sign of that output)."""
    from dc_vic_amd import ops
    from dc_vic_amd.train import autograd as A
    real_conv = A.conv

    def conv(ctx, x, mod, act=ops.ACT_NONE, *a, **k):
        out = real_conv(ctx, x, mod, act, *a, **k)
        if act == ops.ACT_RELU:
            relu_outputs.append(out.data)
        return out
    tr.group.zero_grad()
    ctx = A.Ctx([tr.group])
    if relu_outputs is not None:
        A.conv = conv
    try:
        L, o = tr.forward_losses(ctx, dd["real_images"], dd["vq_indices"], dd["beta_rate"], dd["beta_vq"], dd["noise_y"], dd["noise_z"])
    finally:
        A.conv = real_conv
    ctx.backward()
    return L, o


@pytest.mark.parametrize("case", list(CASES))
def test_step_vs_cpu_restatement(case):
    """Every loss term, y_hat, the reconstruction, and the gradient of every parameter that has one in the helper (the analysis side's
    and the synthesis side's); the others are exactly zero here.  `quantiles` is outside the main group: no gradient reaches it."""
    m, tr = bundle()
    I = inputs(case)
    N = I["x"].shape[0]
    dd = data_dict(I)
    relu_outputs = []
    L, o = forward_backward(tr, dd, relu_outputs)
    relu = RS.ReluDecisions(relu_outputs)
    force = dict(y=o["symbols"]["y"].cpu(), z=o["symbols"]["z"].cpu(), out_idx=o["out_vq_indices"].cpu(), relu=relu)
    lsd = {k: v.detach().cpu().clone() for k, v in tr.lpips.state_dict().items()}
    R, vals, grads, dec = RS.step(cpu_state(), I, torch.tensor(BETA_RATE)[:N], torch.tensor(BETA_VQ)[:N], section(), lsd, force)
    assert max(vals["clamped"]) < 1e-3, vals["clamped"]
    assert not relu.unmatched and len(relu.own) >= 140, (relu.unmatched, len(relu.own))
    n_relu, worst_relu, cap_relu = AR.tie_report(*relu.report())
    relu_line = f"{n_relu} of {relu.report()[0].numel()} ReLU signs ({len(relu.own)} calls) differ (cap {cap_relu}), largest |input| among them {worst_relu:.3e}"
    assert n_relu <= cap_relu and worst_relu < 1e-4, relu_line
    for k in "yz":
        n, worst, cap = AR.tie_report(dec[k][0], force[k], dec[k][1])
        assert n <= cap and worst < 1e-4, f"{k}: {n} differing symbols (cap {cap}), largest distance from a tie {worst:.3e}"
    differ = int((dec["out_idx"] != force["out_idx"]).sum())
    assert differ <= max(1, int(1e-5 * force["out_idx"].numel())), f"{differ} argmax decisions differ"
    assert torch.equal(o["gt_vq_indices"].cpu(), vals["gt_idx"])
    worst = {}
    assert sorted(L) == sorted(R) == ["code_ce", "code_distortion", "distortion", "perceptual", "rate"]
    for k in R:
        worst[f"loss {k}"] = relerr(L[k].reshape(()), R[k])
    worst["y_hat"] = relerr(o["quantized_code"]["y"].data, vals["y_hat"])
    worst["fake"] = relerr(o["fake"].data, vals["fake"])
    for k, v in worst.items():
        assert v <= VAL_TOL, (k, v)
    assert abs(o["qbpp"] - vals["qbpp"]) <= VAL_TOL * vals["qbpp"]
    own = dict(m.named_parameters())
    in_group = {id(p) for p in tr.group.params}
    checked, zero, w_grad, w_name = 0, 0, 0.0, ""
    for k, g in grads.items():
        gp = tr.group.grad_of(own[k])
        if k.endswith(".quantiles"):
            assert gp is None and g is None and id(own[k]) not in in_group
            continue
        if g is None:
            assert float(gp.abs().max()) == 0.0, k
            zero += 1
            continue
        e = relerr(gp, g)
        assert e <= GRAD_TOL, f"grad {k}: {e:.3e}"
        checked += 1
        if e > w_grad:
            w_grad, w_name = e, k
    assert checked == 741, (checked, zero)       # 338 analysis-side tensors (339 less `quantiles`) + 403 synthesis-side
    assert tr.aux_group.numel() == own["entropy_model_z.quantiles"].numel() and float(tr.aux_group.grad.abs().max()) == 0.0
    _log(f"[rd step {case}] " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"; {checked} parameter gradients, worst {w_grad:.3e} ({w_name}); "
         f"{zero} without a gradient are zero; {relu_line}")


def test_update_is_clipped_adam_and_aux_runs_on_the_updated_parameters():
    """optimize_parameters on a fresh model, lr 1e-2 so that the main step moves the bottleneck's parameters visibly: the clipped Adam
    delta in the sign regime against oracle.train_oracle.clip_and_adam (as the stage-3 step test compares it), then the logged `aux`
    and the gradient behind the `quantiles` update against analysis_train_ref.eb_aux on the UPDATED parameters -- and not on the old
    ones, whose value is shown to lie outside the bound."""
    from oracle import train_oracle as T
    lr = 1e-2
    m = build_model()
    tr = build_trainer(m, lr=lr)
    I = inputs("2x64x64")
    dd = data_dict(I)
    sd0 = cpu_state()
    L, o = forward_backward(tr, dd)
    own = dict(m.named_parameters())
    names = [k for k, p in own.items() if tr.group.grad_of(p) is not None]
    g0 = {k: tr.group.grad_of(own[k]).detach().cpu().clone() for k in names}
    q0 = own["entropy_model_z.quantiles"].detach().cpu().clone()
    log = tr.optimize_parameters(1, dd)
    assert log is not None and sorted(log) == sorted(("rate", "distortion", "perceptual", "code_distortion", "code_ce", "total", "qbpp", "vq_acc", "lr", "aux"))
    assert abs(log["total"] - sum(float(v) for v in L.values())) <= 1e-6 * abs(log["total"]) and log["lr"] == lr
    new = T.clip_and_adam({k: sd0[k] for k in names}, g0, lr, 1.0)
    gnorm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g0.values())))
    cscale = min(1.0, 1.0 / (gnorm + 1e-6))
    n_cmp = 0
    for k in names[::5]:
        da, db = (own[k].data.cpu() - sd0[k]).double(), (new[k] - sd0[k]).double()
        big = (g0[k].abs() * cscale) >= 1e-6                 # the first Adam step is -lr * g / (|g| + 1e-8): compared where g >> eps
        assert float(da.abs().max()) <= lr * (1 + 1e-3), k
        if big.any():
            assert float((da - db)[big].abs().max()) <= 2e-2 * lr, k
            n_cmp += int(big.sum())
    assert n_cmp > 10000, n_cmp
    # the aux step: value and gradient of EntropyBottleneck.loss() at the updated parameters
    eb_keys = [k for k in sd0 if k.startswith("entropy_model_z.") and sd0[k].is_floating_point()]
    upd = {k: (own[k].detach().cpu().clone() if k in own else sd0[k]) for k in eb_keys}
    upd["entropy_model_z.quantiles"] = q0                   # the aux loss is evaluated before its own Adam step
    old = {k: sd0[k] for k in eb_keys}
    ref = {}
    for tag, s in (("updated", upd), ("old", old)):
        Lf = AR.leaf_state({k: v.double() for k, v in s.items()}, torch.float64, ["entropy_model_z.quantiles"])
        v = AR.eb_aux(Lf, torch.float64)
        v.backward()
        ref[tag] = (float(v.detach()), Lf["entropy_model_z.quantiles"].grad)
    e_new, e_old = abs(log["aux"] - ref["updated"][0]) / abs(ref["updated"][0]), abs(log["aux"] - ref["old"][0]) / abs(ref["old"][0])
    g_new, g_old = relerr(tr.aux_group.grad.view(q0.shape), ref["updated"][1]), relerr(tr.aux_group.grad.view(q0.shape), ref["old"][1])
    _log(f"[rd aux] value vs updated parameters {e_new:.3e}, vs old {e_old:.3e}; gradient vs updated {g_new:.3e}, vs old {g_old:.3e}")
    assert e_new <= VAL_TOL and g_new <= GRAD_TOL
    assert e_old > 10 * VAL_TOL, "evaluating the aux loss on the old parameters must be told apart"
    dq = (own["entropy_model_z.quantiles"].detach().cpu() - q0).double()
    gq = ref["updated"][1]
    big = gq.abs() >= 1e-6
    assert big.any() and float((dq + 1e-3 * torch.sign(gq))[big].abs().max()) <= 2e-2 * 1e-3      # first Adam step at aux_lr 1e-3
    assert tr.opt.t == 1 and tr.aux_opt.t == 1 and tr.sched.last_epoch == 1


def test_batch_invariance_and_determinism():
    """Image 0 alone and in the batch of 2 with the same noise: its bits (the rate contribution) and y_hat are bit-identical and its dy
    is the same up to the factor 1 / N of the loss weights; two identical seeded steps on two fresh models leave equal bits in every
    parameter."""
    m, tr = bundle()
    I = inputs("2x64x64")
    res = {}
    for tag, keep in (("one", torch.tensor([0])), ("two", slice(None))):
        L, o = forward_backward(tr, data_dict(I, keep))
        res[tag] = dict(bits_y=o["bits_y"].clone(), bits_z=o["bits_z"].clone(), y_hat=o["quantized_code"]["y"].data.clone(),
                        dy=o["latent_code"]["y"].grad.clone())
    for k in ("bits_y", "bits_z", "y_hat"):
        assert torch.equal(res["one"][k][0], res["two"][k][0]), k
    # every loss term of image 0 carries 1 / N (the per-sample weights, the means of the image losses): its dy in the batch of 2 is half
    # its dy alone, a power of two, so nothing but the batch-invariance of every kernel on the way separates the two
    e = relerr(2.0 * res["two"]["dy"][0], res["one"]["dy"][0])
    print(f"[rd batch invariance] dy of image 0, alone against 2 x in the batch of 2: {e:.3e}")
    assert e <= 1e-6 and torch.isfinite(res["two"]["dy"]).all()
    states = []
    for _ in range(2):
        m2 = build_model()
        t2 = build_trainer(m2, seed=11)
        x = (torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)) * 2 - 1)
        for it in (1, 2):
            assert t2.optimize_parameters(it, {"real_images": x}) is not None
        states.append({k: v.detach().cpu().clone() for k, v in m2.state_dict().items()})
    assert all(torch.equal(states[0][k], states[1][k]) for k in states[0])
    assert not torch.equal(states[0]["encoder.conv1.weight"], cpu_state()["encoder.conv1.weight"])


def test_training_state_round_trip():
    """2 steps, save, 1 step -- against a fresh model loaded with the saved weights and training state, 1 step: equal parameters, so
    both random streams (beta sampler, noise generator), both groups' moments and step counts and the scheduler continued."""
    x = [(torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(40 + i)) * 2 - 1) for i in range(3)]
    m = build_model()
    tr = build_trainer(m, seed=21, milestones=(2,))
    for it in (1, 2):
        tr.optimize_parameters(it, {"real_images": x[it - 1]})
    st = tr.training_state(2)
    weights = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    log_a = tr.optimize_parameters(3, {"real_images": x[2]})
    m2 = build_model()
    t2 = build_trainer(m2, seed=99, milestones=(2,))
    m2.load_state_dict(weights)
    t2.resync_parameters()
    assert t2.load_training_state(st) == 2
    log_b = t2.optimize_parameters(3, {"real_images": x[2]})
    assert log_a == log_b and log_a["lr"] == pytest.approx(1e-5)
    assert torch.equal(tr.last_beta_rate, t2.last_beta_rate) and torch.equal(tr.last_beta_vq, t2.last_beta_vq)
    a, b = m.state_dict(), m2.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(tr.group.m, t2.group.m) and torch.equal(tr.aux_group.v, t2.aux_group.v)
    with pytest.raises(ValueError, match="gumbel_sampling"):
        build_trainer(m2, gumbel_sampling=True)


def test_stage3_trainer_afterwards_reproduces_a_fresh_model():
    """A rate-distortion step, the weights put back, then the stage-3 trainer on the SAME model object: its losses and generator
    gradient are the bits of a freshly built model's -- no cached plan, pack or graph of the rate-distortion step leaked."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondTamingNLayerDiscriminator
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(90)) * 2 - 1
    b1, b2 = torch.tensor(BETA_RATE), torch.tensor(BETA_VQ)

    def disc():
        torch.manual_seed(5)
        return DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, L=10, cond_ch=8,
                                                     use_pi=False, include_x=True).to(DEV)
    m = build_model()
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    tr = build_trainer(m)
    assert tr.optimize_parameters(1, {"real_images": x}) is not None
    m.load_state_dict(before)
    tr.resync_parameters()
    out = []
    for model in (m, build_model()):
        g = DualBetaCondGanDistortionVqCodeTrainer(model, disc(), seed=3)
        log = g.optimize_parameters(1, dict(real_images=x, beta_rate=b1, beta_vq=b2))
        out.append((log, g.g_group.grad.clone(), {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])
    assert all(torch.equal(out[0][2][k], out[1][2][k]) for k in out[0][2])


def test_train_cli_stage_1_2_and_resume(tmp_path):
    """scripts/train.py on the synthetic model with exp1_stage1_2.yaml's trainer and loss sections: the trainer line, a finite rate,
    comp_model and training_state files and no discriminator file, and --resume to iteration 3."""
    opt = section()
    cfg = tmp_path / "stage1_2_synthetic.yaml"
    lines = [f"_base_: {os.path.join(ROOT, 'config', 'dc_vic_synthetic.yaml')}", "trainer:"]
    lines += [f"  {k}: {json.dumps(v)}" for k, v in opt["trainer"].items()]          # json.dumps quotes strings: `0_1` unquoted is YAML's integer 1
    lines += ["loss:"]
    for name, e in opt["loss"].items():
        lines += [f"  {name}:"] + [f"    {k}: {json.dumps(v)}" for k, v in e.items()]
    cfg.write_text("\n".join(lines) + "\n")
    out = tmp_path / "ckpt"
    base = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), str(cfg), "--synthetic_weights", "--synthetic_data", "--allow_synthetic_lpips",
            "--batch_size", "2", "--log_step", "1", "--save_dir", str(out)]
    res = subprocess.run(base + ["--total_iter", "2", "--save_step", "2"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("[train] rate-distortion trainer:")]
    assert len(line) == 1 and "beta_policy exp" in line[0] and "sample_beta_batch True" in line[0] and "rate 0.5" in line[0] and "code_ce 0.003" in line[0], res.stdout
    assert "rate none" in line[0] and "code_ce none" in line[0] and "GAN trainer" not in res.stdout
    its = [ln for ln in res.stdout.splitlines() if ln.startswith("iter")]
    assert len(its) == 2 and all("skipped" not in ln for ln in its), res.stdout
    kv = its[0].split("|")[2].split()
    first = dict(zip(kv[0::2], map(float, kv[1::2])))
    assert first["rate"] > 0 and first["rate"] == first["rate"] and first["rate"] < 1e4 and "aux" in first and "qbpp" in first, first
    files = sorted(os.listdir(out))
    assert files == ["comp_model_iter0000002.pth.tar", "training_state_iter0000002.pth.tar"], files
    res2 = subprocess.run(base + ["--total_iter", "3", "--save_step", "3", "--resume", str(out / "training_state_iter0000002.pth.tar")],
                          cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res2.returncode == 0, res2.stderr[-2000:]
    its2 = [ln for ln in res2.stdout.splitlines() if ln.startswith("iter")]
    assert len(its2) == 1 and its2[0].startswith("iter       3") and "skipped" not in its2[0], res2.stdout
    assert not [f for f in os.listdir(out) if f.startswith("discriminator_")] and os.path.exists(out / "comp_model_iter0000003.pth.tar")
