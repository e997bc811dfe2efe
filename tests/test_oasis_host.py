"""OASIS GAN training, host side (no GPU): the meaning of tests/golden/oasis.npz (outputs of the reference's own
DualBetaCondTamingNLayerDiscriminator with config/dc_vic_oasis.yaml's kwargs and of its OasisGANLoss, tools/gen_oasis_golden.py),
the registry names, the loss module's argument checks, the C ABI of the loss kernel and scripts/train.py's trainer choice."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oasis_ce_fp64(logits, idx, is_real, weight):
    """The loss restated in plain torch fp64: weight * mean over N*H*W of CE(logits[:, :, p], idx + 1 if is_real else 0)."""
    lg = torch.as_tensor(logits).double()
    tgt = torch.as_tensor(idx).long()
    tgt = tgt + 1 if is_real else torch.zeros_like(tgt)
    N, C = lg.shape[:2]
    return weight * F.cross_entropy(lg.reshape(N, C, -1), tgt.reshape(N, -1))


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "oasis.npz"))


def close(a, b, rtol, atol=0.0, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.all(np.abs(a - b) <= atol + rtol * np.abs(b)), f"{what}: max |diff| {np.abs(a - b).max():.3e}"


def test_fixture_is_the_fp64_restatement(G):
    """Losses and scores rtol 1e-6, gradients rtol 1e-4 / atol 1e-9 (the bounds train.npz is held to)."""
    w = float(G["gan_loss_weight"])
    idx = G["vq_indices"]
    assert idx.shape == (2, 8, 8) and idx.dtype == np.int64 and idx.min() == 0 and idx.max() == 255
    assert G["d_fake_logits"].shape == (2, 257, 8, 8) and float(np.abs(G["d_fake_logits"]).max()) > 1.0
    close(oasis_ce_fp64(G["d_fake_logits"], idx, True, w), G["adv_loss"], 1e-6, what="adv loss")
    for key, lk, real in (("d_loss_real", "d_real_logits", True), ("d_loss_fake", "d_fake_logits", False)):
        lg = torch.from_numpy(G[lk]).double().requires_grad_(True)
        l = oasis_ce_fp64(lg, idx, real, 0.5)
        l.backward()
        close(l.detach(), G[key], 1e-6, what=key)
        close(lg.grad, G[key + "_grad_logits"], 1e-4, 1e-9, what=key + " gradient")


def test_fixture_scores_are_the_fp64_mean(G):
    """out_d_real / out_d_fake (mean over channels 1:) at rtol 1e-6, the bound set for the fixture's losses and scores.  The
    synthetic discriminator's logits nearly cancel (means 4.9e-4 and -1.2e-3 of values with mean magnitude 1.07), so an fp32 sum of
    them misses the exact mean by a few 1e-6 of the mean, whatever its order; tools/gen_oasis_golden.py therefore accumulates the
    expression in fp64 and rounds once.  The plain fp32 torch.mean is stored beside it (`*_fp32`: 4.2e-6 and 1.7e-7 relative) and is
    held to the forward error of a blocked fp32 sum, (log2(n) + 1) * 2^-24 of the summands' mean magnitude."""
    for key, lk in (("out_d_real", "d_real_logits"), ("out_d_fake", "d_fake_logits")):
        x = torch.from_numpy(G[lk]).double()[:, 1:]
        ref, mag = float(x.mean()), float(x.abs().mean())
        for k in (key, key + "_fp32"):
            got = float(G[k])
            print(f"[oasis fixture] {k}: stored {got:.9e}, fp64 {ref:.9e}, |diff| {abs(got - ref):.3e}, relative {abs(got - ref) / abs(ref):.3e}, "
                  f"relative to mean |x| {abs(got - ref) / mag:.3e}")
        assert G[key].dtype == np.float32
        close(G[key], ref, 1e-6, what=key)
        close(G[key + "_fp32"], ref, 0.0, (np.log2(x.numel()) + 1) * 2.0 ** -24 * mag, what=key + "_fp32")


def test_oracle_discriminator_reproduces_fixture_logits(G):
    from conftest import train_golden_disc_state
    from oracle import train_oracle as T
    dsd = train_golden_disc_state(G)
    kw = json.loads(str(G["d_kwargs"]))
    assert kw["out_nc"] == 257 and kw["keep_shape"] is True
    assert tuple(dsd["main.11.weight"].shape) == (257, 512, 3, 3)
    real, fake = torch.from_numpy(G["real"]), torch.from_numpy(G["fake"])
    b1, b2 = torch.from_numpy(G["beta_1"]), torch.from_numpy(G["beta_2"])
    with torch.no_grad():
        close(T.discriminator(dsd, fake, b1, b2), G["d_fake_logits"], 1e-5, 1e-6, "D(fake)")
        close(T.discriminator(dsd, real, b1, b2), G["d_real_logits"], 1e-5, 1e-6, "D(real)")
        close(T.discriminator(dsd, real, 1.51, 2.25), G["d_real_logits_scalar_beta"], 1e-5, 1e-6, "D(real), scalar betas")


def test_product_discriminator_has_the_fixture_manifest(G):
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator
    D = DualBetaCondTamingNLayerDiscriminator(**json.loads(str(G["d_kwargs"])))
    assert {k: list(v.shape) for k, v in D.state_dict().items()} == json.loads(str(G["d_manifest"]))


def test_registry_names_resolve():
    import dc_vic_amd.train as T
    from dc_vic_amd.registry import LOSS_REGISTRY, TRAINER_REGISTRY
    assert LOSS_REGISTRY.get("OasisGANLoss") is T.OasisGANLoss
    oasis = TRAINER_REGISTRY.get("DualBetaCondOasisGanDistortionVqFusionTrainer")
    base = TRAINER_REGISTRY.get("DualBetaCondGanDistortionVqCodeTrainer")
    assert oasis is T.DualBetaCondOasisGanDistortionVqFusionTrainer and issubclass(oasis, base) and oasis is not base


def test_oasis_gan_loss_argument_checks():
    """The reference's ValueErrors (oasis_gan_loss.py:17-28, :60-61), raised before any kernel call."""
    from dc_vic_amd.train import OasisGANLoss
    from dc_vic_amd.train.autograd import Ctx
    loss = OasisGANLoss(0.01)
    assert loss.lamb_gan == 0.01
    with pytest.raises(ValueError, match="Only expect 4-dimensional logits."):
        loss(Ctx([]), torch.zeros(2, 257, 64), torch.zeros(2, 64, dtype=torch.long), is_disc=True, is_real=True)
    with pytest.raises(ValueError, match="expected target numel to be 128, but found 126"):
        loss(Ctx([]), torch.zeros(2, 257, 8, 8), torch.zeros(2, 7, 9, dtype=torch.long), is_disc=True, is_real=True)
    with pytest.raises(ValueError, match="Expected target to have dtype torch.long."):
        loss(Ctx([]), torch.zeros(2, 257, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int32), is_disc=False, is_real=True)


def test_oasis_trainer_rejects_a_discriminator_that_is_not_the_token_classifier():
    """Construction fails before any GPU work when out_nc != n_embed + 1 or keep_shape is off (what guarantees index + 1 < C)."""
    from types import SimpleNamespace as NS
    from dc_vic_amd.train import DualBetaCondOasisGanDistortionVqFusionTrainer as Tr
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator as Disc
    model = NS(vq_model=NS(quantize=NS(embedding=NS(weight=torch.zeros(256, 4)))))
    with pytest.raises(ValueError, match="out_nc is 1, .* n_embed \\+ 1 = 257"):
        Tr(model, Disc(out_nc=1, keep_shape=True, ndf=8, max_beta_1=3.0, max_beta_2=3.5))
    with pytest.raises(ValueError, match="out_nc is 256"):
        Tr(model, Disc(out_nc=256, keep_shape=True, ndf=8, max_beta_1=3.0, max_beta_2=3.5))
    with pytest.raises(ValueError, match="keep_shape"):
        Tr(model, Disc(out_nc=257, keep_shape=False, ndf=8, max_beta_1=3.0, max_beta_2=3.5))


def test_oasis_kernel_is_declared_and_exported():
    from dc_vic_amd import _lib
    txt = open(os.path.join(ROOT, "include", "dcvic.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.lib()
    for name in ("dcvic_oasis_ce_f32", "dcvic_oasis_ce_workspace_doubles"):
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} not declared in include/dcvic.h"
        assert hasattr(L, name) and name in _lib.SYMBOLS
    # the host-side size query: two doubles per 64-position workgroup, nothing for an empty tensor
    assert L.dcvic_oasis_ce_workspace_doubles(8, 1024) == 2 * 8 * 16 and L.dcvic_oasis_ce_workspace_doubles(3, 77) == 2 * 3 * 2
    assert L.dcvic_oasis_ce_workspace_doubles(0, 64) == 0 and L.dcvic_oasis_ce_workspace_doubles(2, 0) == 0


# ------------------------------------------------------------------------------------------------ scripts/train.py's choice rule
@pytest.fixture(scope="module")
def choose():
    spec = importlib.util.spec_from_file_location("dcvic_train_cli", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.choose_gan_trainer


VAN, OAS = "DualBetaCondGanDistortionVqCodeTrainer", "DualBetaCondOasisGanDistortionVqFusionTrainer"


def _opt(out_nc=None, keep_shape=None, trainer=None, gan_loss=None, mc=None, n_embed=256):
    d = {"type": "DualBetaCondTamingNLayerDiscriminator"}
    if out_nc is not None:
        d["out_nc"] = out_nc
    if keep_shape is not None:
        d["keep_shape"] = keep_shape
    o = {"subnet": {"vq_model": {"n_embed": n_embed}}, "discriminator": d}
    if trainer is not None or mc is not None:
        o["trainer"] = {}
        if trainer is not None:
            o["trainer"]["type"] = trainer
        if mc is not None:
            o["trainer"]["mc_sampling"] = mc
    if gan_loss is not None:
        o["loss"] = {"gan_loss": {"type": gan_loss, "loss_weight": 0.01}}
    return o


@pytest.mark.parametrize("opt,flag,kind,by", [
    (_opt(), None, "vanilla", "out_nc"),                                                   # out_nc absent -> 1
    (_opt(out_nc=1), None, "vanilla", "out_nc"),
    (_opt(out_nc=257, keep_shape=True), None, "oasis", "out_nc"),                          # config/dc_vic_oasis.yaml
    (_opt(out_nc=257, keep_shape=True, gan_loss="OasisGANLoss"), None, "oasis", "loss.gan_loss.type"),
    (_opt(out_nc=1, gan_loss="VanillaGANLoss"), None, "vanilla", "loss.gan_loss.type"),
    (_opt(out_nc=257, keep_shape=True, trainer=OAS, gan_loss="OasisGANLoss"), None, "oasis", "trainer.type"),
    (_opt(trainer=VAN, gan_loss="VanillaGANLoss", mc=False), None, "vanilla", "trainer.type"),    # config/exp1_stage3.yaml
    (_opt(out_nc=257, keep_shape=True, trainer=VAN), "oasis", "oasis", "--gan"),           # the flag wins over the YAML
    (_opt(out_nc=1, trainer=OAS), "vanilla", "vanilla", "--gan"),
    (_opt(out_nc=65, keep_shape=True, n_embed=64), None, "oasis", "out_nc"),
])
def test_trainer_choice_table(choose, opt, flag, kind, by):
    k, name, reason = choose(opt, flag)
    assert k == kind and name == (OAS if kind == "oasis" else VAN) and by in reason, (k, name, reason)


@pytest.mark.parametrize("opt,flag,words", [
    (_opt(out_nc=1), "oasis", ("--gan oasis", "out_nc: 1")),                                # OASIS with out_nc: 1
    (_opt(out_nc=1, trainer=OAS), None, (OAS, "out_nc: 1")),
    (_opt(out_nc=257, keep_shape=True), "vanilla", ("--gan vanilla", "out_nc: 257")),      # vanilla with out_nc: 257
    (_opt(out_nc=257, keep_shape=True, gan_loss="VanillaGANLoss"), None, ("VanillaGANLoss", "out_nc: 257")),
    (_opt(out_nc=257, keep_shape=True, trainer="NoSuchTrainer"), None, ("trainer.type", "NoSuchTrainer")),     # unknown types
    (_opt(out_nc=257, keep_shape=True, gan_loss="HingeGANLoss"), None, ("loss.gan_loss.type", "HingeGANLoss")),
    (_opt(out_nc=3), None, ("out_nc: 3", "257")),
    (_opt(out_nc=257, keep_shape=False), None, ("out_nc: 257", "keep_shape")),
    (_opt(out_nc=257, keep_shape=True, trainer=OAS, gan_loss="VanillaGANLoss"), None, (OAS, "VanillaGANLoss")),
    (_opt(out_nc=257, keep_shape=True, trainer=OAS, mc=True), None, ("mc_sampling", "not built")),
    (_opt(out_nc=1, mc=True), "vanilla", ("mc_sampling", "not built")),
])
def test_trainer_choice_errors_name_both_settings(choose, opt, flag, words):
    with pytest.raises(SystemExit) as e:
        choose(opt, flag)
    msg = str(e.value)
    for w in words:
        assert w in msg, msg


def test_synthetic_config_still_trains_the_patchgan(choose):
    from dc_vic_amd import BaseConfig
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"is_train": True})
    assert choose(opt, None)[:2] == ("vanilla", VAN)
