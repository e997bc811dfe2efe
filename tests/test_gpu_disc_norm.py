"""The normalised GAN discriminators on a real MI355X: the three cases of tests/golden/disc_norm.npz (the reference's own classes in
train mode) through nets.discriminator_forward on the tape, ActNorm's one-time initialisation, one full G + D step each of the
BatchNorm PatchGAN (vanilla loss) and the BatchNorm U-Net (OASIS loss) against torch autograd over the oracle's generator composed with
tests/disc_norm_ref.py, a validation call that leaves the buffers alone, and scripts/train.py with `norm_type: batchnorm` and --resume.

Fixture bounds: the OASIS fixture test's, measured as that test measures them (tests/test_gpu_oasis.py `relclose`: max |difference| over
the fixture tensor's max) -- 2e-5 for logits, 2e-4 for d/d input, 2e-5 for parameter gradients; 2e-5 absolute for the buffers -- each
widened to 4 x the restatement's own fp32-against-fp64 spread on the same inputs where that is larger (test_disc_norm_host.fp32_spread;
for patchgan_bn the spread of d/d input is 7e-3 of max: LeakyReLU signs that sit on the fp32 rounding of a BatchNorm output).

Step bounds: the existing step tests', unwidened -- 2e-4 for values, 3e-3 of each tensor's max for gradients.  The sign of a LeakyReLU
input is a decision: the product's sign masks are recorded call by call and fed to the restatement (as the oracle takes the product's
rounded symbols and estimator argmax), and the positions whose own sign differs are itemised and capped (max(1, 1e-5 x elements) per
layer, each within 1e-4 of zero)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_norm_ref as R
from kernel_bounds import DEV
from test_disc_norm_host import CASES, case_spec, fixture, fp32_spread, grad_keys

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOORS = {"logits": 2e-5, "grad_x": 2e-4, "grad": 2e-5, "buf": 2e-5}


def _build(case):
    import dc_vic_amd.train  # noqa: F401
    from dc_vic_amd.registry import DISCRIMINATOR_REGISTRY
    d_type, kw, _, state = case_spec(case)
    D = DISCRIMINATOR_REGISTRY.get(d_type)(**kw)
    D.load_state_dict(state, strict=True)
    return D.to(DEV), d_type, kw, state


def _err(got, want, scaled):
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all()
    e = float((got - want).abs().max())
    return e / max(float(want.abs().max()), 1e-30) if scaled else e


def _buffers(D):
    return {k: v.detach().cpu().clone() for k, v in D.state_dict().items() if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked", "initialized")}


@pytest.mark.parametrize("case", CASES)
def test_fixture_cases_through_the_tape(case):
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import nets
    G, p = fixture(), case + "."
    spread = fp32_spread(case)
    D, _, _, _ = _build(case)
    assert D.training
    grp = A.ParamGroup([D], DEV)
    t = lambda k: torch.from_numpy(np.asarray(G[k])).to(DEV)
    b1, b2 = torch.from_numpy(G["beta_1"]), torch.from_numpy(G["beta_2"])

    def check(name, got, kind):
        scaled = kind != "buf"              # over the fixture tensor's maximum, as the OASIS fixture test measures logits and gradients
        own_spread = spread[name] / max(float(np.abs(G[p + name]).max()), 1e-30) if kind == "logits" else spread[name]       # (stored absolute)
        err, bound = _err(got, G[p + name], scaled), max(FLOORS[kind], 4 * own_spread)
        print(f"[disc_norm gpu] {case} {name}: err {err:.3g} bound {bound:.3g}")
        assert err <= bound, (case, name, err, bound)

    def check_buffers(tag):
        for k, v in _buffers(D).items():
            if k.endswith(("num_batches_tracked", "initialized")):
                assert int(v) == int(G[p + f"{tag}/{k}"]), (tag, k)
            else:
                check(f"{tag}/{k}", v, "buf")

    ctx = A.Ctx([grp])
    xv = A.Var(t("x"))
    l1 = nets.discriminator_forward(ctx, D, xv, b1, b2)
    check("logits1", l1.data, "logits")
    check_buffers("buf1")
    A.acc(l1, t(p + "cot"))
    ctx.backward()
    check("grad_x", xv.grad, "grad_x")
    params = dict(D.named_parameters())
    for k in grad_keys(case):
        check("grad/" + k, grp.grad_of(params[k]).reshape(G[p + "grad/" + k].shape), "grad")
    l2 = nets.discriminator_forward(A.Ctx([]), D, A.const(t("x")), b1, b2)
    check("logits2", l2.data, "logits")
    check_buffers("buf2")


def test_actnorm_initialises_once_and_not_after_a_loaded_state():
    from dc_vic_amd.layers import ActNorm
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import nets
    D, _, _, state = _build("patchgan_an")
    norms = [m for m in D.modules() if isinstance(m, ActNorm)]
    assert len(norms) == 3 and all(int(m.initialized) == 0 for m in norms)
    G = fixture()
    x = torch.from_numpy(G["x"]).to(DEV)
    b1, b2 = torch.from_numpy(G["beta_1"]), torch.from_numpy(G["beta_2"])
    loc0 = norms[0].loc.detach().clone()
    nets.discriminator_forward(A.Ctx([]), D, A.const(x), b1, b2)
    loc1, scale1 = norms[0].loc.detach().clone(), norms[0].scale.detach().clone()
    assert not torch.equal(loc0, loc1) and all(int(m.initialized) == 1 for m in norms)
    nets.discriminator_forward(A.Ctx([]), D, A.const(x * 0.5 + 0.1), b1, b2)             # another batch: nothing is re-initialised
    assert torch.equal(norms[0].loc, loc1) and torch.equal(norms[0].scale, scale1)
    # the flag was read from the device once per module, whatever the number of calls
    for _ in range(3):
        nets.discriminator_forward(A.Ctx([]), D, A.const(x), b1, b2)
    assert [m.flag_reads for m in norms] == [1, 1, 1]
    # a loaded, initialised state: read once more, no initialisation
    sd = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    D2, _, _, _ = _build("patchgan_an")
    D2.load_state_dict(sd)
    n2 = [m for m in D2.modules() if isinstance(m, ActNorm)]
    nets.discriminator_forward(A.Ctx([]), D2, A.const(x * 0.5 + 0.1), b1, b2)
    assert torch.equal(n2[0].loc, loc1) and [m.flag_reads for m in n2] == [1, 1, 1]
    D2.load_state_dict(sd)
    nets.discriminator_forward(A.Ctx([]), D2, A.const(x), b1, b2)
    assert torch.equal(n2[0].loc, loc1) and [m.flag_reads for m in n2] == [2, 2, 2]
    # eval mode never initialises
    D3, _, _, _ = _build("patchgan_an")
    D3.eval()
    nets.discriminator_forward(A.Ctx([]), D3, A.const(x), b1, b2)
    assert all(int(m.initialized) == 0 for m in D3.modules() if isinstance(m, ActNorm))


@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


def relclose(a, b, tol, what):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)
    assert err <= tol, f"{what}: max |diff| / max |ref| = {err:.3g} > {tol:g}"
    return err


class SignRecorder:
    """The sign decisions of every LeakyReLU of every discriminator call, in call order: wraps nets.discriminator_forward and the tape
    ops it fuses LeakyReLU(0.2) into, and keeps `y > 0` of their outputs (one list of masks per call)."""

    def __init__(self, monkeypatch):
        from dc_vic_amd import ops
        from dc_vic_amd.train import autograd as A
        from dc_vic_amd.train import nets
        self.calls, self._rec = [], None

        def tap(fn):
            def wrapped(*a, **k):
                out = fn(*a, **k)
                if self._rec is not None and k.get("act", ops.ACT_NONE) == ops.ACT_LRELU02:
                    self._rec.append((out.data > 0).cpu())
                return out
            return wrapped
        for name in ("conv", "batch_norm", "act_norm"):
            monkeypatch.setattr(A, name, tap(getattr(A, name)))
        forward = nets.discriminator_forward

        def recorded(*a, **k):
            self._rec = []
            try:
                return forward(*a, **k)
            finally:
                self.calls.append(self._rec)
                self._rec = None
        monkeypatch.setattr(nets, "discriminator_forward", recorded)


def check_flips(Dr, what):
    """analysis_train_ref.tie_report's rule per LeakyReLU: at most max(1, 1e-5 x elements) positions whose own sign differs from the
    product's decision, each within 1e-4 of zero."""
    total = 0
    for n, far, numel in Dr.signs.flips:
        assert n <= max(1, int(1e-5 * numel)) and far < 1e-4, f"{what}: {n} of {numel} signs differ, the farthest {far:.3g} from zero"
        total += n
    assert not Dr.signs.masks, f"{what}: {len(Dr.signs.masks)} recorded sign masks were not consumed"
    Dr.signs.flips.clear()
    return total


@pytest.mark.parametrize("case", ["patchgan_bn", "unet_bn"])
def test_generator_and_discriminator_step_vs_oracle(model, synth_sd, case, monkeypatch):
    """One full optimisation step (2 x 64 x 64, per-sample beta pairs) with a normalised discriminator -- the BatchNorm PatchGAN under the
    vanilla loss, the BatchNorm U-Net under the OASIS loss -- against torch autograd over the CPU oracle's generator composed with
    disc_norm_ref: generator_losses with w['gan'] = 0 plus w_gan * loss(D_ref(fake)), then the D step on D_ref(real) and
    D_ref(fake.detach()).  The oracle runs on the product's integer decisions, and the restated LeakyReLUs on the product's sign
    decisions, which are itemised and capped.  Compared: the fake images and every loss within 2e-4, every generator parameter gradient
    through the frozen D and every discriminator parameter gradient within 3e-3 of its tensor's max, the Adam updates of both sides as
    the existing step tests compare them, and the norm buffers after the real step's calls within 2e-4 of max."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondOasisGanDistortionVqFusionTrainer, nets
    from dc_vic_amd.train import autograd as A
    from oracle import train_oracle as T
    from oracle.entropy_oracle import EntropyBottleneckOracle
    oasis = case == "unet_bn"
    sd_before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        D, d_type, kw, state = _build(case)
        tr = (DualBetaCondOasisGanDistortionVqFusionTrainer if oasis else DualBetaCondGanDistortionVqCodeTrainer)(
            model, D, lr_g=1e-4, lr_d=1e-4, clip_max_norm=1.0, seed=3)
        w_gan = tr.w["gan"]
        signs = SignRecorder(monkeypatch)
        x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(90)) * 2 - 1
        b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
        # ---- product: forward + losses + backward (no optimizer yet); discriminator call 1, with frozen parameters
        tr.g_group.zero_grad()
        ctx = A.Ctx([tr.g_group])
        o = tr.generator_forward(ctx, x, None, b1, b2)
        glog = tr.calc_g_loss(ctx, o, b1, b2)
        ctx.backward()
        assert len(signs.calls) == 1
        # ---- oracle generator on the product's integer decisions, composed with the restated D on the product's sign decisions
        sd = {k: v.clone() for k, v in synth_sd.items()}
        names = [k for k in sd if k.startswith(T.TRAINABLE_PREFIXES) and sd[k].is_floating_point()]
        for k in names:
            sd[k].requires_grad_(True)
        plain = {k: v.detach().clone() for k, v in nets.DualBetaCondTamingNLayerDiscriminator(max_beta_1=3.0, max_beta_2=3.5).state_dict().items()}
        eb = EntropyBottleneckOracle(synth_sd, "entropy_model_z")
        lsd = {k: v.detach().cpu().clone() for k, v in tr.lpips.state_dict().items()}
        L, oo = T.generator_losses(sd, plain, x, b1, b2, eb, w=dict(T.LOSS_W, gan=0.0), lsd=lsd, force_y_hat=o["y_hat"].data.cpu(),
                                   force_out_idx=o["out_vq_indices"].cpu())        # its own discriminator term carries weight 0
        assert torch.equal(o["gt_vq_indices"].cpu(), oo["gt_idx"]), "ground-truth VQ indices differ"
        Dr = R.build(d_type, kw, state, torch.float32)

        def loss(logits, is_real, weight):
            if oasis:
                return weight * F.cross_entropy(logits, oo["gt_idx"] + 1 if is_real else torch.zeros_like(oo["gt_idx"]))
            return weight * F.binary_cross_entropy_with_logits(logits, torch.full_like(logits, 1.0 if is_real else 0.0))

        def d_ref(img, call):
            Dr.signs.masks = list(signs.calls[call])
            out = Dr(img, b1, b2)
            check_flips(Dr, f"{case} discriminator call {call + 1}")
            return out
        L["adv"] = loss(d_ref(oo["fake"], 0), True, w_gan)
        total = sum(L.values())
        total.backward()
        relclose(o["fake"].data, oo["fake"], 2e-4, "fake images")
        for k in ("distortion", "perceptual", "adv", "code_distortion", "code_ce"):
            relclose(glog[k], L[k].detach().reshape(1), 2e-4, f"loss {k}")
        own = dict(model.named_parameters())
        worst, checked = 0.0, 0
        for k in names:
            if sd[k].grad is not None:
                worst = max(worst, relclose(tr.g_group.grad_of(own[k]), sd[k].grad, 3e-3, f"grad {k}"))
                checked += 1
        assert checked >= 400, checked
        print(f"[disc_norm step] {case}: {checked} generator parameter gradients through the frozen D, worst error / max {worst:.3g}")
        # ---- the real step: calls 2 (generator side, the same fake), 3 (real) and 4 (detached fake)
        new = T.clip_and_adam({k: synth_sd[k] for k in names if sd[k].grad is not None}, {k: sd[k].grad for k in names if sd[k].grad is not None}, 1e-4, 1.0)
        log = tr.optimize_parameters(0, dict(real_images=x, beta_rate=b1, beta_vq=b2))
        assert len(signs.calls) == 4
        assert log is not None and abs(log["total"] - float(total.detach())) < 2e-4 * abs(float(total.detach()))
        gnorm = float(torch.sqrt(sum((sd[k].grad.double() ** 2).sum() for k in new)))
        cscale = min(1.0, 1.0 / (gnorm + 1e-6))
        n_cmp = 0
        for k in list(new)[::5]:
            da, db = (own[k].data.cpu() - synth_sd[k]).double(), (new[k] - synth_sd[k]).double()
            big = (sd[k].grad.abs() * cscale) >= 1e-6
            assert float(da.abs().max()) <= 1e-4 * (1 + 1e-3)
            if big.any():
                assert float((da - db)[big].abs().max()) <= 2e-2 * 1e-4, k
                n_cmp += int(big.sum())
        assert n_cmp > 10000, n_cmp
        with torch.no_grad():
            d_ref(oo["fake"].detach(), 1)                       # the step's own generator pass: batch statistics and buffers once more
        Dr.zero_grad()
        d_real, d_fake = d_ref(x, 2), d_ref(oo["fake"].detach(), 3)
        l_real, l_fake = loss(d_real, True, 0.5), loss(d_fake, False, 0.5)
        (l_real + l_fake).backward()
        assert abs(log["d_real"] - float(l_real.detach())) < 1e-4 and abs(log["d_fake"] - float(l_fake.detach())) < 1e-4
        # every discriminator parameter gradient (still in the trainer's flat buffer), then the updates
        dparams, dgrads = dict(Dr.named_parameters()), {}
        dead = {f"{n}.{i}.bias" for n, seq in Dr.named_modules() if isinstance(seq, torch.nn.Sequential) for i, (a, b) in
                enumerate(zip(list(seq), list(seq)[1:])) if isinstance(a, torch.nn.Conv2d) and a.bias is not None and isinstance(b, torch.nn.BatchNorm2d)}
        assert dead == ({"up_blocks.0.1.bias"} if oasis else set())
        worst_d = 0.0
        for k, p in D.named_parameters():
            got, dgrads[k] = tr.d_group.grad_of(p).reshape(dparams[k].shape), dparams[k].grad
            if k in dead:       # a bias in front of a BatchNorm: its gradient is exactly 0, fp32 leaves noise; held to the bound at the layer's weight gradient
                assert float(got.abs().max()) <= 3e-3 * float(dparams[k[:-4] + "weight"].grad.abs().max()), k
            else:
                worst_d = max(worst_d, relclose(got, dgrads[k], 3e-3, f"D grad {k}"))
        print(f"[disc_norm step] {case}: {len(dgrads)} discriminator parameter gradients, worst error / max {worst_d:.3g}")
        newd = T.clip_and_adam({k: state[k] for k in dgrads}, dgrads, 1e-4, None)
        after = D.state_dict()
        for k in dgrads:
            da, db = (after[k].cpu() - state[k]).double(), (newd[k] - state[k]).double()
            big = dgrads[k].abs() >= 1e-6
            assert float(da.abs().max()) <= 1e-4 * (1 + 1e-3), k
            if big.any() and k not in dead:
                assert float((da - db)[big].abs().max()) <= 2e-2 * 1e-4, k
        bufs, ref = _buffers(D), R.norm_buffers(Dr)
        assert bufs and set(bufs) == set(ref)
        for k, v in bufs.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(ref[k]) == 3 + 4, k
            else:
                relclose(v, ref[k], 2e-4, f"buffer {k}")
        # ---- a validation call touches no buffer
        tr.validation(0, [torch.rand((1, 3, 256, 256), generator=torch.Generator().manual_seed(5)) * 2 - 1])
        now = _buffers(D)
        assert all(torch.equal(bufs[k], now[k]) for k in bufs)
    finally:
        model.load_state_dict(sd_before)               # the fixture is shared: put the synthetic weights back
        for m in model.modules():
            if hasattr(m, "_plan"):
                m._plan = None
            if hasattr(m, "_qkv_plan"):
                m._qkv_plan = None
            if hasattr(m, "invalidate_caches"):
                m.invalidate_caches()


def test_train_cli_batchnorm_three_iterations_and_resume(tmp_path):
    """scripts/train.py with `norm_type: batchnorm` over the synthetic model: the discriminator line, three finite iterations, the buffers
    in discriminator_iter*.pth.tar, and --resume from iteration 2 ending with the uninterrupted run's bits at iteration 3."""
    cfg = tmp_path / "bn_synthetic.yaml"
    lines = [f"_base_: {os.path.join(ROOT, 'config', 'dc_vic_synthetic.yaml')}", "discriminator:", "  type: DualBetaCondTamingNLayerDiscriminator",
             "  input_nc: 11", "  n_layers: 3", "  ndf: 64", "  norm_type: batchnorm", "  max_beta_1: 3.0", "  max_beta_2: 3.5", "  L: 10", "  cond_ch: 8",
             "  use_pi: false", "  include_x: true", "loss:", "  perceptual_loss:", "    loss_weight: 0"]
    cfg.write_text("\n".join(lines) + "\n")
    out, out2 = tmp_path / "ckpt", tmp_path / "ckpt2"
    base = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), str(cfg), "--synthetic_weights", "--synthetic_data", "--batch_size", "2", "--log_step", "1"]
    res = subprocess.run(base + ["--total_iter", "3", "--save_dir", str(out), "--save_step", "1"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    dl = [ln for ln in res.stdout.splitlines() if ln.startswith("[train] discriminator:")]
    assert dl == ["[train] discriminator: DualBetaCondTamingNLayerDiscriminator, n_layers 3, norm batchnorm (eps 1e-05, momentum 0.1)"], res.stdout
    its = [ln for ln in res.stdout.splitlines() if ln.startswith("iter")]
    assert len(its) == 3 and all("nan" not in ln.lower() for ln in its), res.stdout
    d3 = torch.load(out / "discriminator_iter0000003.pth.tar", map_location="cpu", weights_only=True)["discriminator"]
    assert int(d3["main.3.num_batches_tracked"]) == 9 and d3["main.3.num_batches_tracked"].dtype == torch.int64          # three calls per step
    assert float(d3["main.6.running_var"].min()) > 0 and not torch.equal(d3["main.6.running_mean"], torch.zeros(256))
    res2 = subprocess.run(base + ["--total_iter", "3", "--save_dir", str(out2), "--save_step", "3", "--resume", str(out / "training_state_iter0000002.pth.tar")],
                          cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res2.returncode == 0, res2.stderr[-2000:]
    its2 = [ln for ln in res2.stdout.splitlines() if ln.startswith("iter")]
    assert len(its2) == 1 and its2[0].split("|")[2] == its[2].split("|")[2], (its2, its[2:])
    d3b = torch.load(out2 / "discriminator_iter0000003.pth.tar", map_location="cpu", weights_only=True)["discriminator"]
    assert set(d3) == set(d3b) and all(torch.equal(d3[k], d3b[k]) for k in d3)
    ck, ck2 = (torch.load(d / "comp_model_iter0000003.pth.tar", map_location="cpu", weights_only=True)["comp_model"] for d in (out, out2))
    assert all(torch.equal(ck[k], ck2[k]) for k in ck)
    # a refusal ends the run before the GPU is touched
    bad_cfg = tmp_path / "bad.yaml"
    bad_cfg.write_text("\n".join(lines).replace("norm_type: batchnorm", "norm_type: groupnorm") + "\n")
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), str(bad_cfg), "--synthetic_weights", "--synthetic_data", "--total_iter", "1"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert bad.returncode != 0 and "discriminator.norm_type: groupnorm is not built" in bad.stderr and "Traceback" not in bad.stderr, bad.stderr[-2000:]
