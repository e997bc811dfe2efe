"""OASIS GAN training on a real MI355X: the loss kernel (csrc/chan_ce.hip) against an fp64 restatement, its determinism and
argument checks, the 257-class discriminator + loss against the reference's own modules (tests/golden/oasis.npz), the 512 -> 257
convolution's gradients, one full G + D step against torch autograd over the CPU oracle, and the CLI with --resume."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def relerr(a, b):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def relclose(a, b, tol, what=""):
    err = relerr(a, b)
    assert err <= tol, f"{what}: max |diff| / max |ref| = {err:.3e} > {tol}"
    return err


def oasis_fp64(logits, idx, is_real, weight):
    """(loss, d loss / d logits, mean(logits[:, 1:])) in torch fp64 on the CPU."""
    lg = logits.detach().cpu().double().requires_grad_(True)
    tgt = idx.cpu().long() + 1 if is_real else torch.zeros_like(idx.cpu().long())
    N, C = lg.shape[:2]
    loss = weight * F.cross_entropy(lg.reshape(N, C, -1), tgt.reshape(N, -1))
    loss.backward()
    return loss.detach().reshape(1), lg.grad, lg.detach()[:, 1:].mean().reshape(1)


# (N, C, H, W, what, logits scale or None for "max |x| = 80"): the trainer's shape, the fixture's, one position, ragged tails below
# and above one 64-position workgroup, the streaming path (C > 272), the smallest C
CASES = [(8, 257, 32, 32, "trainer", 2.0), (2, 257, 8, 8, "fixture shape", 2.0), (1, 257, 1, 1, "one position", 2.0), (3, 5, 7, 11, "ragged 77", 2.0),
         (2, 1000, 10, 13, "ragged 130, streaming", 2.0), (2, 2, 5, 9, "C = 2", 2.0), (2, 257, 8, 8, "+-80", None), (2, 1000, 3, 5, "+-80 streaming", None),
         (2, 272, 9, 9, "last cached C", 2.0), (2, 273, 9, 9, "first streaming C", 2.0)]
VALUE_TOL, GRAD_TOL = 1e-6, 1e-5           # the bounds tests/test_gpu_train.py::test_losses_and_adam holds dcvic_cross_entropy_f32 to
SCORE_TOL = 1e-6                           # the score is summed in fp64 and rounded to fp32 once (2^-24 = 6e-8): 10x that, rounded up


@pytest.mark.parametrize("case", CASES, ids=[c[4] for c in CASES])
def test_oasis_ce_kernel_vs_fp64(case):
    from dc_vic_amd.train import kernels as K
    N, C, H, W, what, scale = case
    lg = rnd(N, C, H, W, seed=300 + C + H)
    lg = lg * scale if scale is not None else lg * (80.0 / float(lg.abs().max()))
    idx = torch.randint(0, C - 1, (N, H, W), generator=torch.Generator().manual_seed(301))
    idx.view(-1)[0], idx.view(-1)[-1] = 0, C - 2                                  # both ends of the codebook
    ld, td = lg.to(DEV), idx.to(DEV)
    weight = 0.5
    for is_real in (True, False):
        ref_l, ref_g, ref_s = oasis_fp64(lg, idx, is_real, weight)
        loss, dl, score = K.oasis_ce(ld, td, is_real, weight / (N * H * W), want_grad=True, want_score=True)
        assert torch.isfinite(loss).all() and torch.isfinite(dl).all() and torch.isfinite(score).all()
        # the path this kernel replaces, on the shifted targets, against the same fp64 values in the same run
        shifted = (td + 1) if is_real else torch.zeros_like(td)
        nll, dl_old = K.cross_entropy(ld, shifted, weight / (N * H * W), want_grad=True)
        old = K.reduce_loss(3, nll, None, weight / (N * H * W))
        ev, eg, es = relerr(loss, ref_l), relerr(dl, ref_g), relerr(score, ref_s)
        print(f"[oasis_ce] {what} is_real={is_real}: value {ev:.3e} (cross_entropy_f32 {relerr(old, ref_l):.3e}), gradient {eg:.3e} "
              f"(cross_entropy_f32 {relerr(dl_old, ref_g):.3e}), score {es:.3e}")
        assert ev <= VALUE_TOL and eg <= GRAD_TOL and es <= SCORE_TOL, (what, is_real, ev, eg, es)
        # value only / value + score / value + gradient: the same bits
        l2, d2, s2 = K.oasis_ce(ld, td, is_real, weight / (N * H * W), want_grad=False, want_score=False)
        assert d2 is None and s2 is None and torch.equal(l2, loss)
        l3, d3, s3 = K.oasis_ce(ld, td, is_real, weight / (N * H * W), want_grad=False, want_score=True)
        assert d3 is None and torch.equal(l3, loss) and torch.equal(s3, score)
        l4, d4, s4 = K.oasis_ce(ld, td, is_real, weight / (N * H * W), want_grad=True, want_score=False)
        assert s4 is None and torch.equal(l4, loss) and torch.equal(d4, dl)


def test_oasis_ce_is_bit_reproducible_and_ignores_buffer_contents():
    import ctypes as C
    from dc_vic_amd._lib import check, lib
    from dc_vic_amd.ops import _p, _stream
    from dc_vic_amd.train import kernels as K
    for N, Cc, H, W in ((8, 257, 32, 32), (2, 1000, 10, 13)):
        ld = (rnd(N, Cc, H, W, seed=310) * 2).to(DEV)
        td = torch.randint(0, Cc - 1, (N, H, W), generator=torch.Generator().manual_seed(311)).to(DEV)
        a = K.oasis_ce(ld, td, True, 0.01 / (N * H * W), want_grad=True, want_score=True)
        b = K.oasis_ce(ld, td, True, 0.01 / (N * H * W), want_grad=True, want_score=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        # every output and the workspace pre-filled with NaN
        need = int(lib().dcvic_oasis_ce_workspace_doubles(N, H * W))
        ws = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)
        loss, score = torch.full((1,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
        dl = torch.full_like(ld, float("nan"))
        check(lib().dcvic_oasis_ce_f32(_p(ld), _p(td), 1, C.c_double(0.01 / (N * H * W)), _p(loss), _p(dl), _p(score), _p(ws), N, Cc, H * W, _stream()),
              "oasis_ce")
        assert torch.equal(loss, a[0]) and torch.equal(dl, a[1]) and torch.equal(score, a[2])
        assert not torch.isnan(ws).any()


def test_oasis_ce_rejects_bad_calls_without_a_launch():
    import ctypes as C
    from dc_vic_amd._lib import DcvicError, check, lib
    from dc_vic_amd.ops import _p, _stream
    from dc_vic_amd.train import kernels as K
    td = torch.zeros((2, 4, 4), dtype=torch.int64, device=DEV)
    with pytest.raises(DcvicError, match="oasis_ce.*C=1"):
        K.oasis_ce(torch.zeros((2, 1, 4, 4), device=DEV), td, True, 1.0)
    with pytest.raises(DcvicError, match="oasis_ce.*empty"):
        K.oasis_ce(torch.zeros((2, 5, 0, 4), device=DEV), torch.zeros((2, 0, 4), dtype=torch.int64, device=DEV), True, 1.0)
    one, ws = torch.zeros(1, device=DEV), torch.zeros(64, dtype=torch.float64, device=DEV)
    rc = lib().dcvic_oasis_ce_f32(None, _p(td), 1, C.c_double(1.0), _p(one), None, None, _p(ws), 2, 5, 16, _stream())
    assert rc < 0
    with pytest.raises(DcvicError, match="oasis_ce.*null pointer"):
        check(rc, "oasis_ce")
    rc = lib().dcvic_oasis_ce_f32(_p(one), None, 1, C.c_double(1.0), _p(one), None, None, _p(ws), 2, 5, 16, _stream())
    assert rc < 0 and b"null target" in lib().dcvic_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ against the reference's own modules
@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "oasis.npz"))


def test_oasis_discriminator_and_losses_vs_reference_modules(G):
    """tests/golden/oasis.npz through the calls the OASIS trainer makes (calc_adv_loss / run_discriminator / calc_d_loss), at the
    bounds test_discriminator_and_losses_vs_reference_modules applies to the PatchGAN fixture."""
    from conftest import train_golden_disc_state
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator, OasisGANLoss, nets
    from dc_vic_amd.train import autograd as A
    D = DualBetaCondTamingNLayerDiscriminator(**json.loads(str(G["d_kwargs"])))
    sd = train_golden_disc_state(G)
    assert {k: tuple(v.shape) for k, v in D.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    D.load_state_dict(sd, strict=True)
    D = D.to(DEV)
    t = lambda k: torch.from_numpy(np.asarray(G[k])).to(DEV)
    real, fake, idx, b1, b2 = t("real"), t("fake"), t("vq_indices"), torch.from_numpy(G["beta_1"]), torch.from_numpy(G["beta_2"])
    gan = OasisGANLoss(float(G["gan_loss_weight"]))
    grp = A.ParamGroup([D], DEV)
    ctx = A.Ctx([])
    fv = A.Var(fake)
    g_fake = nets.discriminator_forward(ctx, D, fv, b1, b2)
    assert tuple(g_fake.data.shape) == (2, 257, 8, 8)
    relclose(g_fake.data, G["d_fake_logits"], 2e-5, "D(fake) logits")
    adv = gan(ctx, g_fake, idx, is_disc=False, is_real=True)
    relclose(adv, np.asarray(G["adv_loss"]).reshape(1), 2e-5, "adv loss")
    ctx.backward()
    relclose(fv.grad, G["adv_grad_fake"], 2e-4, "d(adv)/d(fake)")
    dctx = A.Ctx([grp])
    d_real = nets.discriminator_forward(dctx, D, A.const(real), b1, b2)
    d_fake = nets.discriminator_forward(dctx, D, A.const(fake), b1, b2)
    relclose(d_real.data, G["d_real_logits"], 2e-5, "D(real) logits")
    l_real, s_real = gan(dctx, d_real, idx, is_disc=True, is_real=True, weight=0.5, want_score=True)
    l_fake, s_fake = gan(dctx, d_fake, idx, is_disc=True, is_real=False, weight=0.5, want_score=True)
    relclose(l_real, np.asarray(G["d_loss_real"]).reshape(1), 2e-5, "d_real loss")
    relclose(l_fake, np.asarray(G["d_loss_fake"]).reshape(1), 2e-5, "d_fake loss")
    relclose(d_real.grad, G["d_loss_real_grad_logits"], 2e-5, "d(d_real loss)/d(logits)")
    relclose(d_fake.grad, G["d_loss_fake_grad_logits"], 2e-5, "d(d_fake loss)/d(logits)")
    # the logged scores: against the fixture as far as the logits agree (2e-5 of max |logit| per element bounds the mean's shift; the
    # means themselves are ~1e-3 of the logits' magnitude), and at SCORE_TOL against fp64 means of the product's own logits
    for sc, key, lk in ((s_real, "out_d_real", "d_real_logits"), (s_fake, "out_d_fake", "d_fake_logits")):
        assert abs(float(sc.item()) - float(G[key])) <= 2e-5 * float(np.abs(G[lk]).max()), key
    relclose(s_real, d_real.data.double()[:, 1:].mean().reshape(1), SCORE_TOL, "out_d_real")
    relclose(s_fake, d_fake.data.double()[:, 1:].mean().reshape(1), SCORE_TOL, "out_d_fake")
    dctx.tape = []
    ds = nets.discriminator_forward(A.Ctx([]), D, A.const(real), 1.51, 2.25)
    relclose(ds.data, G["d_real_logits_scalar_beta"], 2e-5, "D(real) logits, scalar betas")


@pytest.mark.parametrize("N,H,W", [(2, 8, 8), (1, 32, 32), (3, 7, 9)])
def test_conv_512_to_257_grads(N, H, W):
    """The OASIS discriminator's last layer (3 x 3, 512 -> 257, an odd channel count: a third 128-channel tile with one live row)
    through the forward, data-gradient and weight-gradient kernels vs torch CPU autograd, at test_conv_wgrad_and_dgrad's bounds."""
    from dc_vic_amd.layers import Conv2d
    from dc_vic_amd.train import autograd as A
    x, w, b = rnd(N, 512, H, W, seed=1), rnd(257, 512, 3, 3, seed=2, scale=0.1), rnd(257, seed=3, scale=0.1)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br, stride=1, padding=1)
    g = rnd(*y.shape, seed=4)
    y.backward(g)
    mod = Conv2d(512, 257, 3, 1, 1).to(DEV)
    mod.weight.data.copy_(w); mod.bias.data.copy_(b)
    grp = A.ParamGroup([mod], DEV)
    ctx = A.Ctx([grp])
    xv = A.Var(x.to(DEV))
    out = A.conv(ctx, xv, mod)
    relclose(out.data, y, 1e-5, "conv forward")
    out.grad = g.to(DEV)
    ctx.backward()
    relclose(grp.grad_of(mod.weight), wr.grad, 2e-5, "dW")
    relclose(grp.grad_of(mod.bias), br.grad, 2e-5, "db")
    relclose(xv.grad, xr.grad, 2e-5, "dX")
    # the generator step's view of the layer: D not trainable, only the data gradient
    ctx = A.Ctx([]); xv = A.Var(x.to(DEV)); out = A.conv(ctx, xv, mod); out.grad = g.to(DEV); ctx.backward()
    relclose(xv.grad, xr.grad, 2e-5, "dX, frozen layer")


# ------------------------------------------------------------------------------------------------ one full step vs the oracle
@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


def _oasis_disc(seed=5):
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator
    torch.manual_seed(seed)
    D = DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, out_nc=257, keep_shape=True, norm_type="none", max_beta_1=3.0,
                                              max_beta_2=3.5, L=10, cond_ch=8, use_pi=False, include_x=True)
    g = torch.Generator().manual_seed(seed)
    for p in D.parameters():          # deterministic, a bit larger than N(0, 0.02) so the logits carry signal
        p.data.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
    return D


def test_oasis_generator_and_discriminator_step_vs_oracle(model, synth_sd):
    """One full OASIS optimisation step (2 x 64 x 64, per-sample beta pairs) against torch autograd over the CPU oracle:
    generator_losses with w['gan'] = 0 plus w_gan * CE(D(fake), gt_idx + 1); the D step 0.5 * CE(D(real), gt_idx + 1) +
    0.5 * CE(D(fake.detach()), 0).  The oracle is evaluated on the product's integer decisions (rounded symbols, estimator argmax).
    Bounds: those of test_generator_and_discriminator_step_vs_oracle."""
    from dc_vic_amd.train import DualBetaCondOasisGanDistortionVqFusionTrainer
    from dc_vic_amd.train import autograd as A
    from oracle import train_oracle as T
    from oracle.entropy_oracle import EntropyBottleneckOracle
    sd_before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        D = _oasis_disc().to(DEV)
        dsd0 = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
        tr = DualBetaCondOasisGanDistortionVqFusionTrainer(model, D, lr_g=1e-4, lr_d=1e-4, clip_max_norm=1.0, seed=3)
        w_gan = tr.w["gan"]
        x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(90)) * 2 - 1
        b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
        # ---- product: forward + losses + backward (no optimizer yet)
        tr.g_group.zero_grad()
        ctx = A.Ctx([tr.g_group])
        o = tr.generator_forward(ctx, x, None, b1, b2)
        glog = tr.calc_g_loss(ctx, o, b1, b2)
        ctx.backward()
        # ---- oracle on the product's integer decisions
        sd = {k: v.clone() for k, v in synth_sd.items()}
        names = [k for k in sd if k.startswith(T.TRAINABLE_PREFIXES) and sd[k].is_floating_point()]
        for k in names:
            sd[k].requires_grad_(True)
        dsd = {k: v.clone().requires_grad_(True) for k, v in dsd0.items()}
        eb = EntropyBottleneckOracle(synth_sd, "entropy_model_z")
        lsd = {k: v.detach().cpu().clone() for k, v in tr.lpips.state_dict().items()}
        w0 = dict(T.LOSS_W, gan=0.0)
        L, oo = T.generator_losses(sd, dsd, x, b1, b2, eb, w=w0, lsd=lsd, force_y_hat=o["y_hat"].data.cpu(), force_out_idx=o["out_vq_indices"].cpu())
        assert torch.equal(o["gt_vq_indices"].cpu(), oo["gt_idx"]), "ground-truth VQ indices differ"
        L["adv"] = w_gan * F.cross_entropy(T.discriminator(dsd, oo["fake"], b1, b2), oo["gt_idx"] + 1)
        total = sum(L.values())
        total.backward()
        relclose(o["fake"].data, oo["fake"], 2e-4, "fake images")
        for k in ("distortion", "perceptual", "adv", "code_distortion", "code_ce"):
            relclose(glog[k], L[k].detach().reshape(1), 2e-4, f"loss {k}")
        own = dict(model.named_parameters())
        worst, checked = 0.0, 0
        for k in names:
            gref = sd[k].grad
            if gref is None:
                continue
            worst = max(worst, relclose(tr.g_group.grad_of(own[k]), gref, 3e-3, f"grad {k}"))
            checked += 1
        assert checked >= 400, checked
        print(f"[oasis train parity] {checked} generator parameter gradients, worst relative error {worst:.6e}")
        # ---- the real step, then the updated parameters and the D step
        new = T.clip_and_adam({k: synth_sd[k] for k in names if sd[k].grad is not None}, {k: sd[k].grad for k in names if sd[k].grad is not None}, 1e-4, 1.0)
        log = tr.optimize_parameters(0, dict(real_images=x, beta_rate=b1, beta_vq=b2))
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
        for p in dsd.values():
            p.grad = None
        d_real, d_fake = T.discriminator(dsd, x, b1, b2), T.discriminator(dsd, oo["fake"].detach(), b1, b2)
        l_real = 0.5 * F.cross_entropy(d_real, oo["gt_idx"] + 1)
        l_fake = 0.5 * F.cross_entropy(d_fake, torch.zeros_like(oo["gt_idx"]))
        (l_real + l_fake).backward()
        assert abs(log["d_real"] - float(l_real.detach())) < 1e-4 and abs(log["d_fake"] - float(l_fake.detach())) < 1e-4
        assert abs(log["out_d_real"] - float(d_real.detach().double()[:, 1:].mean())) < 1e-4
        assert abs(log["out_d_fake"] - float(d_fake.detach().double()[:, 1:].mean())) < 1e-4
        # every discriminator parameter gradient is behind the Adam update: compare the updates as the PatchGAN step test does
        newd = T.clip_and_adam(dsd0, {k: dsd[k].grad for k in dsd0}, 1e-4, None)
        for k, p in D.state_dict().items():
            da, db = (p.cpu() - dsd0[k]).double(), (newd[k] - dsd0[k]).double()
            big = dsd[k].grad.abs() >= 1e-6
            if big.any():
                assert float((da - db)[big].abs().max()) <= 2e-2 * 1e-4, k
    finally:
        model.load_state_dict(sd_before)               # the fixture is shared: put the synthetic weights back
        for m in model.modules():
            if hasattr(m, "_plan"):
                m._plan = None
            if hasattr(m, "_qkv_plan"):
                m._qkv_plan = None
            if hasattr(m, "invalidate_caches"):
                m.invalidate_caches()


def test_oasis_discriminator_parameter_gradients_vs_oracle(G):
    """Every discriminator parameter gradient of the OASIS D step (the fixture's weights and images) within 3e-3 of its tensor's max."""
    from conftest import train_golden_disc_state
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator, OasisGANLoss, nets
    from dc_vic_amd.train import autograd as A
    from oracle import train_oracle as T
    sd = train_golden_disc_state(G)
    D = DualBetaCondTamingNLayerDiscriminator(**json.loads(str(G["d_kwargs"])))
    D.load_state_dict(sd, strict=True)
    D = D.to(DEV)
    t = lambda k: torch.from_numpy(np.asarray(G[k]))
    real, fake, idx, b1, b2 = t("real"), t("fake"), t("vq_indices"), t("beta_1"), t("beta_2")
    dsd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    (0.5 * F.cross_entropy(T.discriminator(dsd, real, b1, b2), idx + 1) + 0.5 * F.cross_entropy(T.discriminator(dsd, fake, b1, b2), torch.zeros_like(idx))).backward()
    grp = A.ParamGroup([D], DEV)
    dctx = A.Ctx([grp])
    gan = OasisGANLoss(0.01)
    d_real = nets.discriminator_forward(dctx, D, A.const(real.to(DEV)), b1, b2)
    d_fake = nets.discriminator_forward(dctx, D, A.const(fake.to(DEV)), b1, b2)
    gan(dctx, d_real, idx.to(DEV), is_disc=True, is_real=True, weight=0.5)
    gan(dctx, d_fake, idx.to(DEV), is_disc=True, is_real=False, weight=0.5)
    dctx.backward()
    for k, p in D.named_parameters():
        relclose(grp.grad_of(p), dsd[k].grad, 3e-3, f"D grad {k}")


# ------------------------------------------------------------------------------------------------ CLI
def test_train_cli_oasis_and_resume(G, tmp_path):
    """scripts/train.py on a config equal to config/dc_vic_oasis.yaml's discriminator section over the synthetic model (perceptual
    weight 0): the choice line, cross-entropy-sized losses, discriminator checkpoints with the fixture's manifest, and --resume from
    the middle ending with bit-identical files."""
    cfg = tmp_path / "oasis_synthetic.yaml"
    dk = json.loads(str(G["d_kwargs"]))
    lines = [f"_base_: {os.path.join(ROOT, 'config', 'dc_vic_synthetic.yaml')}", "discriminator:", "  type: DualBetaCondTamingNLayerDiscriminator"]
    lines += [f"  {k}: {json.dumps(v) if not isinstance(v, str) else v}" for k, v in dk.items()]
    lines += ["loss:", "  perceptual_loss:", "    loss_weight: 0"]
    cfg.write_text("\n".join(lines) + "\n")
    out, out2 = tmp_path / "ckpt", tmp_path / "ckpt2"
    base = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), str(cfg), "--synthetic_weights", "--synthetic_data", "--batch_size", "2", "--log_step", "1"]
    res = subprocess.run(base + ["--total_iter", "4", "--save_dir", str(out), "--save_step", "2"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    choice = [ln for ln in res.stdout.splitlines() if ln.startswith("[train] GAN trainer:")]
    assert len(choice) == 1 and "oasis" in choice[0] and "DualBetaCondOasisGanDistortionVqFusionTrainer" in choice[0] and "out_nc: 257" in choice[0], res.stdout
    assert "0.01" in choice[0] and "default" in choice[0], choice[0]
    its = [ln for ln in res.stdout.splitlines() if ln.startswith("iter")]
    assert len(its) == 4 and all("adv" in ln and "d_total" in ln and "out_d_real" in ln for ln in its), res.stdout
    kv = its[0].split("|")[2].split()
    first = dict(zip(kv[0::2], map(float, kv[1::2])))
    # N(0, 0.02) initial weights -> logits near 0 -> every CE is near ln 257 = 5.549: d_real = d_fake = 0.5 * 5.549, adv = 0.01 * 5.549 (a BCE
    # over the same logits would be 0.5 * ln 2 = 0.347 and 0.01 * ln 2)
    ln257 = float(np.log(257.0))
    assert abs(first["d_real"] - 0.5 * ln257) < 0.05 and abs(first["d_fake"] - 0.5 * ln257) < 0.05 and abs(first["adv"] - 0.01 * ln257) < 0.001, first
    dk4 = torch.load(out / "discriminator_iter0000004.pth.tar", map_location="cpu", weights_only=True)
    assert dk4["iter"] == 4
    assert {k: list(v.shape) for k, v in dk4["discriminator"].items()} == json.loads(str(G["d_manifest"]))
    res2 = subprocess.run(base + ["--total_iter", "4", "--save_dir", str(out2), "--save_step", "4", "--resume", str(out / "training_state_iter0000002.pth.tar")],
                          cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res2.returncode == 0, res2.stderr[-2000:]
    its2 = [ln for ln in res2.stdout.splitlines() if ln.startswith("iter")]
    assert len(its2) == 2 and [ln.split("|")[2] for ln in its2] == [ln.split("|")[2] for ln in its[2:]], (its2, its[2:])
    ck, ck2 = (torch.load(d / "comp_model_iter0000004.pth.tar", map_location="cpu", weights_only=True) for d in (out, out2))
    dk2 = torch.load(out2 / "discriminator_iter0000004.pth.tar", map_location="cpu", weights_only=True)
    assert all(torch.equal(ck["comp_model"][k], ck2["comp_model"][k]) for k in ck["comp_model"])
    assert all(torch.equal(dk4["discriminator"][k], dk2["discriminator"][k]) for k in dk4["discriminator"])
    # a choice that cannot be right ends before the GPU is touched
    bad = subprocess.run(base + ["--total_iter", "1", "--gan", "vanilla"], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert bad.returncode != 0 and "--gan vanilla" in bad.stderr and "out_nc: 257" in bad.stderr and "Traceback" not in bad.stderr, bad.stderr[-2000:]
