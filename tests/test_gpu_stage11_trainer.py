"""The stage 1-1 trainer (RateDistortionVqCodeTrainer over the unconditioned HyperpriorCharmVicModel) on a real MI355X: one whole step
against torch autograd over tests/stage11_ref.py (rd_step_ref's restatement on the neutralised dual state, unit weights), the clipped
Adam update and the aux step's ordering, the linear warm-up, resume through the training state, and the CLI with the hand-off of its
checkpoint into the dual-conditioned model of stage 1-2.

Inputs: 2 x 64x64 and 1 x 64x128, config/dc_vic_synthetic_stage1_1.yaml's `optim` and `loss` sections, the synthetic weights the two
models share with the scale transforms' last biases raised (analysis_train_ref.shifted_state).  Bounds and the treatment of decisions
(forced symbols, argmax and ReLU signs, capped by tie_report) are tests/test_gpu_rd_trainer.py's: 2e-4 of max for values and loss
terms, 3e-3 of the tensor's max for every parameter gradient.

Set DCVIC_STAGE11_ERRLOG=<file> to have the worst errors appended there."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import analysis_train_ref as AR
import rd_step_ref as RS
import stage11_ref as S11

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG11 = os.path.join(ROOT, "config", "dc_vic_synthetic_stage1_1.yaml")
DEV = "cuda:0"
VAL_TOL, GRAD_TOL = 2e-4, 3e-3
CASES = {"2x64x64": ((2, 3, 64, 64), 81), "1x64x128": ((1, 3, 64, 128), 82)}
LOG_KEYS = ("rate", "distortion", "perceptual", "code_distortion", "code_ce", "total", "qbpp", "vq_acc", "lr", "aux")
FLAT = dict(type="MultiStepLR", milestones=[300000], gamma=0.1)


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def _log(line):
    print(line)
    path = os.environ.get("DCVIC_STAGE11_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def opt11():
    from dc_vic_amd import BaseConfig
    return BaseConfig.fromfile(CFG11, {"device": DEV, "is_train": True})


@functools.lru_cache(maxsize=None)
def cpu_state():
    """The neutralised dual state the CPU restatement runs on; its shared tensors are the unconditioned model's."""
    from dc_vic_amd.synth import full_synth_state_dict
    sd = AR.shifted_state(full_synth_state_dict(1234))
    return S11.neutral_dual_state({k: v for k, v in sd.items() if not S11.is_conditioning_key(k)}, sd)


def build_model():
    from dc_vic_amd import build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(opt11())
    load_synth_weights(m, 1234)
    have = set(m.state_dict())
    m.load_state_dict({k: v for k, v in cpu_state().items() if k in have}, strict=False)
    return m


def build_trainer(m, lr=1e-4, seed=3, **kw):
    """The trainer as scripts/train.py builds it from the YAML's sections (train/build.py), under the test's lr, seed and overrides."""
    from dc_vic_amd.train import RateDistortionVqCodeTrainer
    from dc_vic_amd.train.build import rd_stage_1_1_kwargs
    from dc_vic_amd.train.losses import read_loss_section
    args = dict(rd_stage_1_1_kwargs(opt11(), read_loss_section(opt11())), lr=lr, seed=seed)
    args.update(kw)
    return RateDistortionVqCodeTrainer(m, **args)


@functools.lru_cache(maxsize=None)
def bundle():
    m = build_model()
    return m, build_trainer(m)


@functools.lru_cache(maxsize=None)
def inputs(case):
    shape, seed = CASES[case]
    return AR.analysis_inputs(cpu_state(), shape, seed)


def data_dict(I):
    d = lambda t: t.contiguous().to(DEV)
    return dict(real_images=d(I["x"]), vq_indices=d(I["idx"]), noise_y=d(I["noise_y"]), noise_z=d(I["noise_z"]))


def forward_backward(tr, dd, relu_outputs=None, ops_seen=None):
    """Forward, losses and backward of one step; with `relu_outputs` (a list) every output of a convolution with a fused ReLU is
    appended to it; with `ops_seen` (a list) every beta-conditioning call of the step is collected: ("cond_vector",), ("beta_vectors",)
    and ("chan_affine", channels of its input)."""
    from dc_vic_amd import ops
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import nets
    real_conv, real_affine, real_cond, real_vec = A.conv, A.chan_affine, nets.cond_vector, nets.beta_vectors

    def conv(ctx, x, mod, act=ops.ACT_NONE, *a, **k):
        out = real_conv(ctx, x, mod, act, *a, **k)
        if act == ops.ACT_RELU and relu_outputs is not None:
            relu_outputs.append(out.data)
        return out

    def chan_affine(ctx, x, *a, **k):
        ops_seen.append(("chan_affine", int(x.data.shape[1])))
        return real_affine(ctx, x, *a, **k)

    def cond_vector(*a, **k):
        ops_seen.append(("cond_vector",))
        return real_cond(*a, **k)

    def beta_vectors(*a, **k):
        ops_seen.append(("beta_vectors",))
        return real_vec(*a, **k)
    tr.group.zero_grad()
    ctx = A.Ctx([tr.group])
    A.conv = conv
    if ops_seen is not None:
        A.chan_affine, nets.cond_vector, nets.beta_vectors = chan_affine, cond_vector, beta_vectors
    try:
        L, o = tr.forward_losses(ctx, dd["real_images"], dd["vq_indices"], None, None, dd["noise_y"], dd["noise_z"])
    finally:
        A.conv, A.chan_affine, nets.cond_vector, nets.beta_vectors = real_conv, real_affine, real_cond, real_vec
    ctx.backward()
    return L, o


@pytest.mark.parametrize("case", list(CASES))
def test_step_vs_cpu_restatement(case):
    """Every loss term, y_hat, the reconstruction and the gradient of every non-frozen parameter; no beta conditioning is recorded."""
    from dc_vic_amd.train.rd_trainer import is_main_parameter
    m, tr = bundle()
    I = inputs(case)
    dd = data_dict(I)
    relu_outputs, seen = [], []
    L, o = forward_backward(tr, dd, relu_outputs, seen)
    assert seen == [("chan_affine", 3)] * 2, seen        # LPIPS's input scaling of the two images and nothing else: no cond_vector, no beta_vectors, no beta-FT
    relu = RS.ReluDecisions(relu_outputs)
    force = dict(y=o["symbols"]["y"].cpu(), z=o["symbols"]["z"].cpu(), out_idx=o["out_vq_indices"].cpu(), relu=relu)
    lsd = {k: v.detach().cpu().clone() for k, v in tr.lpips.state_dict().items()}
    sec = json.loads(json.dumps(dict(loss={k: dict(v) for k, v in opt11()["loss"].items()})))
    R, vals, grads, dec = S11.step(cpu_state(), I, sec, lsd, force)
    assert max(vals["clamped"]) < 1e-3, vals["clamped"]
    # the restatement runs on the neutralised DUAL state, so it still evaluates the conditioning MLPs (2 `mlp` and 18 `shared` ReLUs on
    # [N, cond_ch] vectors), whose outputs meet zero weights: the product has no such call, and they are the only unmatched ones
    cond_relu = [s for s in relu.unmatched if s[0] == I["x"].shape[0] and s[1] == 128 and (len(s) == 2 or tuple(s[2:]) == (1, 1))]
    assert len(cond_relu) == len(relu.unmatched) == 20 and len(relu.own) == 126, (relu.unmatched, len(relu.own))
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
    _log(f"[stage 1-1 step {case}] " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= VAL_TOL, (k, v)
    assert abs(o["qbpp"] - vals["qbpp"]) <= VAL_TOL * vals["qbpp"]
    own = dict(m.named_parameters())
    trainable = {k for k in own if is_main_parameter(k)}
    assert {k for k in grads if not k.endswith(".quantiles")} == trainable and {id(own[k]) for k in trainable} == {id(p) for p in tr.group.params}
    assert not [k for k in own if k.startswith("vq_model.") and tr.group.grad_of(own[k]) is not None]
    ratios, without = {}, []
    for k, g in grads.items():
        gp = tr.group.grad_of(own[k])
        if k.endswith(".quantiles"):
            assert gp is None and g is None
            continue
        if g is None:
            assert float(gp.abs().max()) == 0.0, k
            without.append(k)
            continue
        assert float(gp.abs().max()) > 0.0, k                    # every executed tensor receives a gradient
        ratios[k] = relerr(gp, g)
    top = sorted(ratios.items(), key=lambda kv: -kv[1])[:5]
    _log(f"[stage 1-1 step {case}] {len(ratios)} parameter gradients, worst " + ", ".join(f"{k} {v:.3e}" for k, v in top) + f"; without a gradient (zero): {without}; {relu_line}")
    assert sorted(without) == ["decoder.conv4.bias", "decoder.conv4.weight"]      # in the state dict, never executed
    # the dual step's 741 less the 116 conditioning tensors that receive a gradient there (122 less decoder.beta_ft_list.8's six: conv4 never runs)
    assert len(ratios) == 741 - 116 and len(ratios) + 2 == len(trainable)
    for k, e in ratios.items():
        assert e <= GRAD_TOL, f"grad {k}: {e:.3e}"
    assert tr.aux_group.numel() == own["entropy_model_z.quantiles"].numel() and float(tr.aux_group.grad.abs().max()) == 0.0


def test_update_is_clipped_adam_and_aux_runs_on_the_updated_parameters():
    """As tests/test_gpu_rd_trainer.py's test of the same name: lr 1e-2 on a flat schedule, the clipped Adam delta against
    oracle.train_oracle.clip_and_adam on the product's own gradients, then `aux` and the `quantiles` gradient on the UPDATED parameters."""
    from oracle import train_oracle as T
    lr = 1e-2
    m = build_model()
    tr = build_trainer(m, lr=lr, scheduler=FLAT)
    dd = data_dict(inputs("2x64x64"))
    sd0 = cpu_state()
    L, o = forward_backward(tr, dd)
    own = dict(m.named_parameters())
    names = [k for k, p in own.items() if tr.group.grad_of(p) is not None]
    g0 = {k: tr.group.grad_of(own[k]).detach().cpu().clone() for k in names}
    q0 = own["entropy_model_z.quantiles"].detach().cpu().clone()
    log = tr.optimize_parameters(1, dd)
    assert log is not None and tuple(log) == tuple(k for k in LOG_KEYS if k in log) and sorted(log) == sorted(LOG_KEYS)
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
    g_new = relerr(tr.aux_group.grad.view(q0.shape), ref["updated"][1])
    _log(f"[stage 1-1 aux] value vs updated parameters {e_new:.3e}, vs old {e_old:.3e}; gradient vs updated {g_new:.3e}")
    assert e_new <= VAL_TOL and g_new <= GRAD_TOL
    assert e_old > 10 * VAL_TOL, "evaluating the aux loss on the old parameters must be told apart"
    dq = (own["entropy_model_z.quantiles"].detach().cpu() - q0).double()
    gq = ref["updated"][1]
    big = gq.abs() >= 1e-6
    assert big.any() and float((dq + 1e-3 * torch.sign(gq))[big].abs().max()) <= 2e-2 * 1e-3      # first Adam step at aux_lr 1e-3
    assert tr.opt.t == 1 and tr.aux_opt.t == 1 and tr.sched.last_epoch == 1


def test_warm_up_drives_the_logged_lr_and_the_first_update():
    """warmup_iters 4, factor 0.1: the `lr` logged over 6 steps is the closed form exactly, and step 1 moves the parameters by
    0.1 x base_lr (the first Adam step is lr x g / (|g| + eps): |delta| = lr where the clipped |g| >> eps)."""
    base = 1e-3
    m = build_model()
    tr = build_trainer(m, lr=base, scheduler=dict(type="LinearWarmupScheduler", warmup_iters=4, warmup_factor=0.1))
    before = tr.group.flat.detach().clone()
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(31)) * 2 - 1
    lrs = []
    for it in range(1, 7):
        log = tr.optimize_parameters(it, {"real_images": x})
        assert log is not None
        lrs.append(log["lr"])
        if it == 1:
            g = tr.group.grad.detach().clone()
            delta = (tr.group.flat.detach() - before).abs()
            gnorm = float(torch.sqrt((g.double() ** 2).sum()))
            big = (g.abs() * min(1.0, 1.0 / (gnorm + 1e-6))) >= 1e-5         # eps / |g| <= 1e-3
            assert int(big.sum()) > 10000
            # fp32: p - step and (p_new - p) each round to an ulp of |p|
            ulp = 2 * float(torch.finfo(torch.float32).eps) * float(before.abs().max())
            assert float(delta.max()) <= 0.1 * base * (1 + 1e-3) + ulp and float(delta[big].min()) >= 0.1 * base * (1 - 2e-3) - ulp, (float(delta.max()), float(delta[big].min()), ulp)
            assert ulp < 0.02 * base, ulp                     # the bound still tells 0.1 x base_lr from base_lr, and from 0.325 x base_lr (step 2)
    want = [base * (0.1 * (1 - k / 4) + k / 4) if k < 4 else base for k in range(6)]
    assert lrs == want, (lrs, want)
    assert tr.sched.last_epoch == 6 and tr.opt.t == 6


def test_resume_and_determinism():
    """Two runs from one state give equal bits in every parameter; 2 + 2 steps through training_state / load_training_state equal 4
    steps bit for bit (both Adam groups, the scheduler's epoch inside a warm-up, the noise generator; there is no beta RNG)."""
    x = [(torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(50 + i)) * 2 - 1) for i in range(4)]
    warm = dict(type="LinearWarmupScheduler", warmup_iters=3, warmup_factor=0.1)
    snap = lambda model: {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    m = build_model()
    tr = build_trainer(m, seed=21, scheduler=warm)
    logs = []
    for it in (1, 2):
        logs.append(tr.optimize_parameters(it, {"real_images": x[it - 1]}))
    st, mid = tr.training_state(2), snap(m)
    assert sorted(st) == ["aux", "iter", "last_epoch", "main", "noise_gen"]
    for it in (3, 4):
        logs.append(tr.optimize_parameters(it, {"real_images": x[it - 1]}))
    end = snap(m)
    # a second run from the same state
    m2 = build_model()
    t2 = build_trainer(m2, seed=21, scheduler=warm)
    for it in (1, 2):
        assert t2.optimize_parameters(it, {"real_images": x[it - 1]}) == logs[it - 1]
    again = snap(m2)
    assert all(torch.equal(mid[k], again[k]) for k in mid)
    # 2 + 2: a fresh model and a trainer with another seed, the saved weights and training state
    m3 = build_model()
    t3 = build_trainer(m3, seed=99, scheduler=warm)
    m3.load_state_dict(mid)
    t3.resync_parameters()
    assert t3.load_training_state(st) == 2
    for it in (3, 4):
        assert t3.optimize_parameters(it, {"real_images": x[it - 1]}) == logs[it - 1]
    resumed = snap(m3)
    assert all(torch.equal(end[k], resumed[k]) for k in end)
    assert torch.equal(tr.group.m, t3.group.m) and torch.equal(tr.aux_group.v, t3.aux_group.v) and t3.sched.last_epoch == 4
    assert logs[3]["lr"] == 1e-4 and logs[0]["lr"] == pytest.approx(1e-5)
    assert not torch.equal(end["encoder.conv1.weight"], mid["encoder.conv1.weight"])
    val = tr.validation(4, [x[0][:1].to(DEV)])
    assert sorted(val) == ["bpp", "ms_ssim", "psnr", "vq_acc"]
    with pytest.raises(ValueError, match="gumbel_sampling"):
        build_trainer(m3, gumbel_sampling=True)
    with pytest.raises(ValueError, match="reduction"):
        build_trainer(m3, code_ce_reduction="none")


def test_cli_and_the_hand_off_into_stage_1_2(tmp_path):
    """scripts/train.py on config/dc_vic_synthetic_stage1_1.yaml for 2 iterations: the trainer line, comp_model and training_state files;
    that file loaded into the dual-conditioned model leaves every shared tensor with the checkpoint's bits and every conditioning
    tensor as it was, the report names the missing groups, and one stage 1-2 step from it returns finite terms."""
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.train import DualBetaCondRateDistortionVqCodeTrainer
    from dc_vic_amd.train.build import rd_trainer_kwargs, weight_load_report
    from dc_vic_amd.train.losses import read_loss_section
    out = tmp_path / "ckpt"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), CFG11, "--synthetic_weights", "--synthetic_data", "--allow_synthetic_lpips",
                          "--batch_size", "1", "--total_iter", "2", "--save_step", "2", "--log_step", "1", "--save_dir", str(out)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("[train] rate-distortion trainer:")]
    assert len(line) == 1 and "RateDistortionVqCodeTrainer;" in line[0] and "Dual" not in line[0], res.stdout
    for w in ("rate 0.04", "distortion 50", "perceptual 1", "code_distortion 0.1", "code_ce 0.05", "gamma 2", "LinearWarmupScheduler", "warmup_iters 50000", "warmup_factor 0.1"):
        assert w in line[0], (w, line[0])
    its = [ln for ln in res.stdout.splitlines() if ln.startswith("iter")]
    assert len(its) == 2 and all("skipped" not in ln for ln in its), res.stdout
    kv = its[0].split("|")[2].split()
    first = dict(zip(kv[0::2], map(float, kv[1::2])))
    assert tuple(first) == LOG_KEYS and 0 < first["rate"] < 1e4 and first["lr"] == pytest.approx(1e-5, rel=1e-4), first
    assert sorted(os.listdir(out)) == ["comp_model_iter0000002.pth.tar", "training_state_iter0000002.pth.tar"]
    path = str(out / "comp_model_iter0000002.pth.tar")
    ck = torch.load(path, map_location="cpu", weights_only=True)["comp_model"]
    assert not [k for k in ck if S11.is_conditioning_key(k)]
    torch.manual_seed(9)
    dual = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    before = {k: v.detach().cpu().clone() for k, v in dual.state_dict().items()}
    report = weight_load_report(dual.load_learned_weight(path))
    for grp in ("encoder.beta_ft_list 54", "encoder.mlp 4", "decoder.beta_ft_list 54", "decoder.mlp 4", "decoder.init_fuse 6"):
        assert grp in report, report
    after = {k: v.detach().cpu() for k, v in dual.state_dict().items()}
    shared = [k for k in after if k in ck and after[k].is_floating_point() and not k.startswith("entropy_model_y.")]
    assert len(shared) > 800 and all(torch.equal(after[k], ck[k]) for k in shared)
    cond = [k for k in after if S11.is_conditioning_key(k)]
    assert len(cond) == 122 and all(torch.equal(after[k], before[k]) for k in cond)
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        sec = json.load(f)["exp1_stage1_2.yaml"]
    tr = DualBetaCondRateDistortionVqCodeTrainer(dual, seed=1, **rd_trainer_kwargs(sec, read_loss_section(sec)))
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(61)) * 2 - 1
    log = tr.optimize_parameters(1, {"real_images": x})
    assert log is not None and all(v == v and abs(v) < float("inf") for v in log.values()), log
