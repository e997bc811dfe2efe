"""Stage 1-1 on the host: the unconditioned sub-networks through the unchanged oracle against the reference's own classes
(tests/golden/uncond.npz, tools/gen_uncond_golden.py), the LinearWarmupScheduler, the readers of `optim`, the CLI's choice, the
registries, the state-dict keys, the initialisation a run without a checkpoint starts from, and the hand-off report into stage 1-2."""
import json
import math
import os

import numpy as np
import pytest
import torch

import stage11_ref as S11
from oracle import dcvic_oracle as O
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG11 = os.path.join(ROOT, "config", "dc_vic_synthetic_stage1_1.yaml")
RD11, RD12, MODEL11 = "RateDistortionVqCodeTrainer", "DualBetaCondRateDistortionVqCodeTrainer", "HyperpriorCharmVicModel"
TOL = dict(rtol=2e-4, atol=2e-4)          # tests/test_oracle_golden.py's, for its encoder stage
DEC_TOL = dict(rtol=1e-3, atol=1e-3)      # and for its decoder features


@pytest.fixture(scope="module")
def uncond_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "uncond.npz"))


@pytest.fixture(scope="module")
def opt11():
    from dc_vic_amd import BaseConfig
    return BaseConfig.fromfile(CFG11, {"device": "cpu", "is_train": True})


@pytest.fixture(scope="module")
def model11(opt11):
    from dc_vic_amd import build_comp_model
    return build_comp_model(opt11)


def uncond_state(synth_sd):
    """The unconditioned model's synthetic state as the product restricts it (dc_vic_amd.synth.load_synth_weights)."""
    from dc_vic_amd.synth import is_conditioning_key
    return {k: v for k, v in synth_sd.items() if not is_conditioning_key(k)}


# ---------------------------------------------------------------------------------------------------- the oracle against the fixture
def test_oracle_on_the_neutralised_state_equals_the_reference_classes(uncond_golden, synth_sd):
    G = uncond_golden
    neutral = S11.neutral_dual_state(uncond_state(synth_sd), synth_sd)
    # what "neutralised" means, and that nothing else moved
    assert float(neutral["decoder.init_fuse.scale.bias"].min()) == float(neutral["decoder.init_fuse.scale.bias"].max()) == -1.0
    assert all(float(neutral[k].abs().max()) == 0.0 for k in neutral if ".beta_ft_list." in k and k.split(".")[-2] in ("scale", "shift"))
    assert torch.equal(neutral["encoder.mlp.0.weight"], synth_sd["encoder.mlp.0.weight"]) and torch.equal(neutral["encoder.conv1.weight"], synth_sd["encoder.conv1.weight"])
    x = torch.from_numpy(G["x_u8"]).float() / 127.5 - 1.0
    idx = torch.from_numpy(G["vq_indices"].astype(np.int64))
    with torch.no_grad():
        zq, own_idx = O.vq_encode(neutral, x)
        assert torch.equal(own_idx, idx)
        y = O.elic_encoder(neutral, x, O.onehot_feat(neutral, zq, idx), S11.BETA, S11.BETA)
        f1, fd = O.elic_decoder_feats(neutral, torch.from_numpy(G["y_hat"]), S11.BETA, S11.BETA)
    np.testing.assert_allclose(y.numpy(), G["y"], **TOL)
    np.testing.assert_allclose(f1.numpy(), G["feat_1"], **DEC_TOL)
    np.testing.assert_allclose(fd["block_1_8"].numpy(), G["feat_1"], **DEC_TOL)
    np.testing.assert_allclose(fd["block_1_4"].numpy(), G["block_1_4"], **DEC_TOL)
    np.testing.assert_allclose(fd["block_1_2"].numpy(), G["block_1_2"], **DEC_TOL)
    worst = max(float(np.abs(y.numpy() - G["y"]).max()), float(np.abs(fd["block_1_2"].numpy() - G["block_1_2"]).max()))
    print(f"[stage 1-1 oracle] largest difference from the reference's classes {worst:.3e} (y max {np.abs(G['y']).max():.3f})")
    # any other beta pair gives the same values: the conditioning is switched off, not tuned
    with torch.no_grad():
        assert torch.equal(O.elic_encoder(neutral, x, O.onehot_feat(neutral, zq, idx), 2.29, 3.0), y)


def test_state_dict_keys_are_the_dual_manifests_minus_the_conditioning(model11, manifest, uncond_golden):
    own = model11.state_dict()
    for tag in ("encoder", "decoder"):
        want = {k: shape for k, (shape, _) in manifest.items() if k.startswith(tag + ".") and not S11.is_conditioning_key(k)}
        have = {k: list(v.shape) for k, v in own.items() if k.startswith(tag + ".")}
        assert have == want, sorted(set(have) ^ set(want))[:5]
        ref = {f"{tag}.{k}": v for k, v in json.loads(str(uncond_golden[f"{tag}_manifest"])).items()}       # the reference classes' own keys
        assert have == ref
    assert sum(k.startswith("encoder.") for k in own) == 140 and sum(k.startswith("decoder.") for k in own) == 138
    assert not [k for k in own if S11.is_conditioning_key(k)] and "decoder.conv4.weight" in own
    # every other module is the dual model's
    rest = {k for k in manifest if not k.startswith(("encoder.", "decoder."))}
    assert rest <= set(own)


def test_synthetic_weights_are_the_dual_state_restricted(model11, synth_sd):
    from dc_vic_amd.synth import is_conditioning_key, load_synth_weights
    sd = load_synth_weights(model11, 1234)
    assert set(sd) == {k for k in synth_sd if not is_conditioning_key(k)} and all(is_conditioning_key(k) == S11.is_conditioning_key(k) for k in synth_sd)
    own = model11.state_dict()
    assert all(torch.equal(own[k], synth_sd[k]) for k in sd)


# ---------------------------------------------------------------------------------------------------- registries and refusals
def test_classes_and_trainer_resolve_by_name():
    import dc_vic_amd.train as T
    from dc_vic_amd import comp_model, elic
    from dc_vic_amd.registry import DECODER_REGISTRY, ENCODER_REGISTRY, MODEL_REGISTRY, TRAINER_REGISTRY
    from dc_vic_amd.train.rd_trainer import RateDistortionStep
    assert ENCODER_REGISTRY.get("ElicVqCatScEncoder") is elic.ElicVqCatScEncoder
    assert DECODER_REGISTRY.get("ElicFeatFusionDecoder") is elic.ElicFeatFusionDecoder
    assert MODEL_REGISTRY.get(MODEL11) is comp_model.HyperpriorCharmVicModel
    cls, dual = TRAINER_REGISTRY.get(RD11), TRAINER_REGISTRY.get(RD12)
    assert cls is T.RateDistortionVqCodeTrainer and not issubclass(cls, dual) and not issubclass(dual, cls)
    # the step body exists once
    for name in ("forward_losses", "optimize_parameters", "optimize_aux_parameters", "resync_parameters", "checkpoint_modules"):
        assert getattr(cls, name) is getattr(dual, name) is getattr(RateDistortionStep, name), name
    # the model shares decode and tiling with the dual class
    for name in ("_decode", "decode_split", "vq_encode", "_entropy_encode_side"):
        assert getattr(comp_model.HyperpriorCharmVicModel, name) is getattr(comp_model.HyperpriorCharmDualCondVicModel, name), name
    assert not hasattr(comp_model.HyperpriorCharmVicModel, "compress") and not hasattr(comp_model.HyperpriorCharmVicModel, "decompress")


def test_sub_network_refusals(opt11):
    from dc_vic_amd import build_comp_model
    from dc_vic_amd.elic import ElicFeatFusionDecoder, ElicVqCatScEncoder
    with pytest.raises(NotImplementedError, match="proj_pos: conv4.*H/8"):
        ElicVqCatScEncoder(proj_pos="conv4")
    with pytest.raises(ValueError, match="proj_pos"):
        ElicVqCatScEncoder(proj_pos="conv5")
    kw = dict(fusion_layer_dict={"block1": "block_1_8"}, feat_layer_name="block1")
    for bad in (dict(pixel_shuffle=True), dict(res_in_res=True)):
        with pytest.raises(AssertionError):
            ElicFeatFusionDecoder(**kw, **bad)
    with pytest.raises(AssertionError):
        ElicVqCatScEncoder(res_in_res=True)
    dec = ElicFeatFusionDecoder(**kw)
    with pytest.raises(NotImplementedError):
        dec.forward(torch.zeros(1, 192, 2, 2))
    with pytest.raises(ValueError, match="unconditioned"):
        dec.get_feats(torch.zeros(1, 192, 2, 2), beta_1=1.0, beta_2=None)
    enc = ElicVqCatScEncoder(input_feat_ch=260, proj_init=True, proj_init_std=0.01)
    assert float(enc.projection.bias.abs().max()) == 0.0 and float(enc.projection.weight.abs().max()) <= 2 * 0.01
    o2 = json.loads(json.dumps(opt11.to_dict() if hasattr(opt11, "to_dict") else dict(opt11)))
    o2["subnet"]["residual_predictor"] = {"type": "Anything"}
    with pytest.raises(NotImplementedError, match="Residual Predictor"):
        build_comp_model(o2)


def test_model_refuses_training_mode_and_compress_cli_refuses_the_type(model11, tmp_path):
    import subprocess
    import sys
    with pytest.raises(NotImplementedError):
        model11.run_model(torch.zeros(1, 3, 64, 64), is_train=True)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compress.py"), "--config_path", CFG11, "--img_dir", str(tmp_path),
                          "--save_dir", str(tmp_path / "out"), "-q", "0", "-d", "cpu", "--synthetic_weights"], capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "HyperpriorCharmVicModel has no bitstream" in res.stderr and "Traceback" not in res.stderr, res.stderr[-800:]


# ---------------------------------------------------------------------------------------------------- the schedule
def closed_form(base_lr, k, iters, factor):
    return base_lr * (factor * (1 - k / iters) + k / iters) if k < iters else base_lr


@pytest.mark.parametrize("iters,factor,base", [(5, 0.1, 1e-4), (4, 0.1, 1e-4), (50000, 0.1, 1e-4), (3, 0.25, 3e-4), (0, 0.1, 1e-4)])
def test_linear_warmup_schedule_equals_the_closed_form_and_torch(iters, factor, base, uncond_golden):
    from dc_vic_amd.train.trainer import LinearWarmupScheduler, MultiStepLR
    s = LinearWarmupScheduler(base, iters, factor)
    assert {"lr", "step", "last_epoch"} <= set(dir(s)) and {"lr", "step", "last_epoch"} <= set(dir(MultiStepLR(base, [3], 0.1)))
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=base)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: (factor * (1 - float(k) / iters) + float(k) / iters) if k < iters else 1.0)
    got = []
    for k in range(min(iters, 6) + 4):
        assert s.last_epoch == k
        got.append(s.lr())
        assert s.lr() == closed_form(base, k, iters, factor) == opt.param_groups[0]["lr"], (k, s.lr(), opt.param_groups[0]["lr"])
        opt.step(); lam.step(); s.step()
    assert (iters > 6 or got[-1] == base) and (iters == 0 or got[0] == base * factor)
    if iters > 6:                                     # far into and past a long warm-up
        for k in (iters // 2, iters - 1, iters, iters + 7):
            s.last_epoch = k
            assert s.lr() == closed_form(base, k, iters, factor)
    if (iters, factor, base) == (5, 0.1, 1e-4) and "warmup_lr" in uncond_golden.files:       # the reference's class, where it imported
        assert got[:8] == [float(v) for v in uncond_golden["warmup_lr"]]
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="warmup_iters"):
            LinearWarmupScheduler(base, bad, factor)


def test_read_g_scheduler():
    from dc_vic_amd.train.build import read_g_scheduler
    assert read_g_scheduler({}) == dict(type="MultiStepLR", milestones=[300000], gamma=0.1)
    assert read_g_scheduler(dict(optim=dict(g_scheduler=dict(milestones=[10, 20], gamma=0.5)))) == dict(type="MultiStepLR", milestones=[10, 20], gamma=0.5)
    assert read_g_scheduler(dict(optim=dict(g_scheduler=dict(type="MultiStepLR", milestones=[7], gamma=0.2)))) == dict(type="MultiStepLR", milestones=[7], gamma=0.2)
    w = dict(type="LinearWarmupScheduler", warmup_iters=50000, warmup_factor=0.1)
    assert read_g_scheduler(dict(optim=dict(g_scheduler=dict(w)))) == w
    for sec, words in ((dict(type="LinearWarmupMultiStepLR", warmup_iters=5, warmup_factor=0.1, milestones=[9], gamma=0.1), ("optim.g_scheduler.type", "LinearWarmupMultiStepLR")),
                       (dict(type="CosineAnnealingLR"), ("optim.g_scheduler.type", "CosineAnnealingLR")),
                       (dict(w, milestones=[3]), ("optim.g_scheduler.milestones", "[3]")),
                       (dict(type="LinearWarmupScheduler", warmup_factor=0.1), ("optim.g_scheduler.warmup_iters", "missing")),
                       (dict(w, warmup_iters=2.5), ("optim.g_scheduler.warmup_iters", "2.5")),
                       (dict(w, warmup_factor="tenth"), ("optim.g_scheduler.warmup_factor", "tenth"))):
        with pytest.raises(SystemExit) as e:
            read_g_scheduler(dict(optim=dict(g_scheduler=sec)))
        assert all(wd in str(e.value) for wd in words), str(e.value)


def test_read_rd_optimizers():
    from dc_vic_amd.train.build import read_rd_optimizers
    assert read_rd_optimizers({}) == dict(lr=1e-4, aux_lr=1e-3)
    assert read_rd_optimizers(dict(optim=dict(g_optimizer=dict(type="Adam", lr=2e-4), aux_optimizer=dict(lr=5e-3)))) == dict(lr=2e-4, aux_lr=5e-3)
    for sec, words in ((dict(g_optimizer=dict(type="AdamW", lr=1e-4)), ("optim.g_optimizer.type", "AdamW")),
                       (dict(g_optimizer=dict(type="Adam", lr=1e-4, weight_decay=0.01)), ("optim.g_optimizer.weight_decay", "0.01")),
                       (dict(aux_optimizer=dict(type="Adam", lr=1e-3, paramwise_opt={})), ("optim.aux_optimizer.paramwise_opt",)),
                       (dict(aux_optimizer=dict(type="SGD")), ("optim.aux_optimizer.type", "SGD")),
                       (dict(g_optimizer=dict(lr=0)), ("optim.g_optimizer.lr", "0"))):
        with pytest.raises(SystemExit) as e:
            read_rd_optimizers(dict(optim=sec))
        assert all(wd in str(e.value) for wd in words), str(e.value)


# ---------------------------------------------------------------------------------------------------- the CLI's choice
def as_dict(opt):
    return json.loads(json.dumps(opt.to_dict() if hasattr(opt, "to_dict") else dict(opt)))


def test_choose_trainer_on_the_project_config(opt11):
    from dc_vic_amd.train.build import build_rd_stage_1_1_trainer, choose_trainer, rd_stage_1_1_kwargs, rd_trainer_kwargs  # noqa: F401
    from dc_vic_amd.train.losses import read_loss_section
    kind, name, reason = choose_trainer(opt11)
    assert (kind, name) == ("rd", RD11) and "trainer.type" in reason and MODEL11 in reason
    kw = rd_stage_1_1_kwargs(opt11, read_loss_section(opt11))
    assert kw == dict(lr=1e-4, aux_lr=1e-3, scheduler=dict(type="LinearWarmupScheduler", warmup_iters=50000, warmup_factor=0.1), clip_max_norm=1.0,
                      loss_weights=dict(rate=0.04, distortion=50.0, perceptual=1.0, code_distortion=0.1, code_ce=0.05), rate_reduction="mean",
                      code_ce_gamma=2.0, code_ce_reduction="mean", code_distortion_reduction="mean", distortion_factor=0.25, distortion_type="MSELoss",
                      gumbel_sampling=False)
    o = as_dict(opt11)
    for flag in ("vanilla", "oasis"):
        with pytest.raises(SystemExit) as e:
            choose_trainer(o, flag)
        assert f"--gan {flag}" in str(e.value) and RD11 in str(e.value)
    for m_type in ("HyperpriorCharmDualCondVicModel", None):
        o2 = as_dict(opt11)
        if m_type is None:
            del o2["model"]
        else:
            o2["model"]["type"] = m_type
        with pytest.raises(SystemExit) as e:
            choose_trainer(o2)
        for w in (RD11, "not built", MODEL11, "LinearWarmupScheduler", "ElicVqCatScEncoder", "ElicFeatFusionDecoder", f"model.type: {m_type}"):
            assert w in str(e.value), str(e.value)
    for change, words in ((("model", "gumbel_sampling", True), ("model.gumbel_sampling", "not built")),
                          (("loss", "code_ce_loss", dict(type="FocalCrossEntropyLoss", gamma=2.0, loss_weight=0.05, reduction="none")), ("loss.code_ce_loss.reduction", "none")),
                          (("loss", "rate_loss", dict(type="RateLoss", loss_weight=0.04, reduction="none")), ("loss.rate_loss.reduction", "none")),
                          (("loss", "gan_loss", dict(type="VanillaGANLoss", loss_weight=0.01)), ("loss.gan_loss",)),
                          (("optim", "g_scheduler", dict(type="LinearWarmupMultiStepLR")), ("optim.g_scheduler.type", "LinearWarmupMultiStepLR")),
                          (("optim", "g_optimizer", dict(type="Adam", lr=1e-4, weight_decay=0.1)), ("optim.g_optimizer.weight_decay",))):
        o2 = as_dict(opt11)
        o2[change[0]][change[1]] = change[2]
        with pytest.raises(SystemExit) as e:
            choose_trainer(o2)
        assert all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.skipif(not os.path.isdir(os.path.join(ref_loader.REF, "config")), reason="reference tree absent (GPU box)")
def test_choose_trainer_on_the_reference_yaml(opt11):
    from dc_vic_amd import BaseConfig
    from dc_vic_amd.train.build import choose_trainer, rd_stage_1_1_kwargs
    from dc_vic_amd.train.losses import read_loss_section
    opt = BaseConfig.fromfile(os.path.join(ref_loader.REF, "config", "exp1_stage1_1.yaml"), {"device": "cpu", "is_train": True})
    assert choose_trainer(opt)[:2] == ("rd", RD11)
    assert rd_stage_1_1_kwargs(opt, read_loss_section(opt)) == rd_stage_1_1_kwargs(opt11, read_loss_section(opt11))
    # the project's flattened config is the reference's, but for the VQGAN checkpoint
    a, b = as_dict(opt), as_dict(opt11)
    for sec in ("model", "trainer", "optim", "loss"):
        assert a[sec] == b[sec], sec
    a["subnet"]["vq_model"]["ckpt_path"] = None
    a["subnet"].pop("_delete_", None)                 # the base model file's own marker, left in place by every stage's YAML
    assert a["subnet"] == b["subnet"]


def test_from_scratch_start_needs_the_vqgan(opt11, tmp_path):
    from dc_vic_amd.train.build import from_scratch_vqgan
    with pytest.raises(SystemExit, match="subnet.vq_model.ckpt_path is absent.*--synthetic_weights"):
        from_scratch_vqgan(opt11)
    o = as_dict(opt11)
    o["subnet"]["vq_model"]["ckpt_path"] = str(tmp_path / "nowhere.ckpt")
    with pytest.raises(SystemExit, match="nowhere.ckpt does not exist"):
        from_scratch_vqgan(o)
    (tmp_path / "vq.ckpt").write_bytes(b"x")
    o["subnet"]["vq_model"]["ckpt_path"] = str(tmp_path / "vq.ckpt")
    assert from_scratch_vqgan(o) == str(tmp_path / "vq.ckpt")


# ---------------------------------------------------------------------------------------------------- the initialisation
TRUNC_STD_RATIO = math.sqrt(1 - 2 * 2 * math.exp(-2.0) / math.sqrt(2 * math.pi) / math.erf(math.sqrt(2.0)))     # std of N(0, 1) cut at +-2: 0.8796


def std_within(t, std_rule, kurt_excess):
    """|sample std - rule's| within 4 standard errors: se(s) = std * sqrt((kurtosis - 1) / (4 n)) for n draws, to first order."""
    n = t.numel()
    se = std_rule * math.sqrt((kurt_excess + 2.0) / (4.0 * n))
    got = float(t.double().pow(2).mean().sqrt())            # the mean is 0 by the rule
    return abs(got - std_rule) <= 4 * se, got, se


def test_reference_init_rules_bounds_and_determinism(opt11):
    from dc_vic_amd import build_comp_model
    from dc_vic_amd.train.init import reference_init_
    from dc_vic_amd.train.rd_trainer import is_main_parameter
    torch.manual_seed(0)
    m = build_comp_model(opt11)
    frozen = {k: v.clone() for k, v in m.state_dict().items() if k.startswith("vq_model.")}
    rules = reference_init_(m, torch.Generator().manual_seed(7))
    own = dict(m.named_parameters())
    assert set(rules) == {k for k in own if not k.startswith("vq_model.")} and {k for k in rules if is_main_parameter(k)} | {"entropy_model_z.quantiles"} == set(rules)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in frozen.items())
    # the families: which rule where
    assert rules["encoder.conv1.weight"] == rules["decoder.conv1.bias"] == rules["hyperdecoder.hd_mu.conv1.weight"] == "torch"
    assert rules["encoder.projection.weight"] == "torch" and rules["fusion_module.fusion_modules.block_1_8.scale.0.weight"] == "torch"     # proj_init: false, no weight_init
    assert rules["vq_estimator.swin_blks.0.residual_group.blocks.0.attn.relative_position_bias_table"] == "table"
    assert rules["vq_estimator.swin_blks.0.residual_group.blocks.0.norm1.weight"] == "norm" and rules["entropy_model_z._bias0"] == "bottleneck"
    n_checked = {"torch": 0, "table": 0, "norm": 0}
    for k, rule in rules.items():
        p = own[k].detach()
        if rule == "torch":
            w = own[k.rsplit(".", 1)[0] + ".weight"]
            fan_in = w.shape[1] * (w[0, 0].numel() if w.dim() > 2 else 1)
            bound = 1.0 / math.sqrt(fan_in)
            assert float(p.abs().max()) <= float(np.float32(bound)), (k, float(p.abs().max()), bound)       # the draws are fp32: the bound as fp32 holds it
            if p.numel() >= 64:
                ok, got, se = std_within(p, bound / math.sqrt(3.0), 1.8 - 3.0)          # a uniform's kurtosis is 9/5
                assert ok, (k, got, bound / math.sqrt(3.0), se)
            n_checked["torch"] += 1
        elif rule == "table":
            assert float(p.abs().max()) <= 2 * 0.02, k
            ok, got, se = std_within(p, 0.02 * TRUNC_STD_RATIO, 2.3655 - 3.0)            # kurtosis of N(0, 1) cut at +-2
            assert ok, (k, got, 0.02 * TRUNC_STD_RATIO, se)
            n_checked["table"] += 1
        elif rule == "norm":
            assert bool((p == (1.0 if k.endswith(".weight") else 0.0)).all()), k
            n_checked["norm"] += 1
    assert n_checked["torch"] > 500 and n_checked["table"] == 9 and n_checked["norm"] == 60, n_checked
    # ConvTranspose2d: fan_in is out_ch x k x k, as torch computes it from weight.shape[1]
    assert float(own["decoder.conv4.weight"].abs().max()) <= float(np.float32(1 / math.sqrt(3 * 25))) and float(own["decoder.conv4.weight"].abs().max()) > 1 / math.sqrt(192 * 25)
    # the bottleneck's own values
    eb = m.entropy_model_z
    scale = 10 ** (1 / 5)
    for i, f in enumerate((3, 3, 3, 3, 1)):
        assert bool((getattr(eb, f"_matrix{i}").detach() == float(np.log(np.expm1(1 / scale / f)))).all())
        b = getattr(eb, f"_bias{i}").detach()
        assert float(b.abs().max()) <= 0.5 and std_within(b, 0.5 / math.sqrt(3.0), 1.8 - 3.0)[0]
        if i < 4:
            assert float(getattr(eb, f"_factor{i}").detach().abs().max()) == 0.0
    assert torch.equal(eb.quantiles.detach(), torch.tensor([-10.0, 0.0, 10.0]).repeat(192, 1, 1))
    # equal seeds, equal bits; another seed, other bits
    first = {k: v.detach().clone() for k, v in own.items()}
    reference_init_(m, torch.Generator().manual_seed(7))
    assert all(torch.equal(first[k], own[k].detach()) for k in first)
    reference_init_(m, torch.Generator().manual_seed(8))
    assert not torch.equal(first["encoder.conv1.weight"], own["encoder.conv1.weight"].detach())


def test_reference_init_honours_the_trunc_normal_options_and_refuses_the_dual_model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.train.init import reference_init_
    opt = BaseConfig.fromfile(CFG11, {"device": "cpu", "is_train": True})
    o = as_dict(opt)
    o["subnet"]["encoder"].update(proj_init=True, proj_init_std=0.01)
    o["subnet"]["fusion_module"].update(weight_init=True, weight_init_std=0.03)
    m = build_comp_model(o)
    rules = reference_init_(m, torch.Generator().manual_seed(1))
    own = dict(m.named_parameters())
    assert rules["encoder.projection.weight"] == "trunc:0.01" and rules["encoder.conv3.weight"] == "torch"
    w = own["encoder.projection.weight"].detach()
    assert float(w.abs().max()) <= 2 * 0.01 and std_within(w, 0.01 * TRUNC_STD_RATIO, 2.3655 - 3.0)[0] and float(own["encoder.projection.bias"].abs().max()) == 0.0
    fus = [k for k in rules if k.startswith("fusion_module.")]
    assert fus
    for k in fus:
        if rules[k] == "norm":
            continue
        assert rules[k] == "trunc:0.03", k
        p = own[k].detach()
        if k.endswith(".bias"):
            assert float(p.abs().max()) == 0.0, k
        else:
            assert float(p.abs().max()) <= 2 * 0.03 and std_within(p, 0.03 * TRUNC_STD_RATIO, 2.3655 - 3.0)[0], k
    dual = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": "cpu"}))
    with pytest.raises(ValueError, match="unconditioned"):
        reference_init_(dual, torch.Generator().manual_seed(1))


# ---------------------------------------------------------------------------------------------------- the hand-off into stage 1-2
def test_hand_off_report_and_load(model11, synth_sd, tmp_path):
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    from dc_vic_amd.train.build import weight_load_report
    load_synth_weights(model11, 1234)
    ck11 = {k: v.detach().clone() + (0.5 if k == "encoder.conv1.bias" else 0.0) for k, v in model11.state_dict().items()}
    path = str(tmp_path / "comp_model_iter0000002.pth.tar")
    torch.save({"iter": 2, "comp_model": ck11}, path)
    torch.manual_seed(3)
    dual = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": "cpu"}))
    before = {k: v.detach().clone() for k, v in dual.state_dict().items()}
    rep = dual.load_learned_weight(path)
    line = weight_load_report(rep)
    assert line.startswith(f"weights: {len(ck11)} tensors loaded; missing in the checkpoint")
    for grp in ("encoder.beta_ft_list 54", "encoder.mlp 4", "decoder.beta_ft_list 54", "decoder.mlp 4", "decoder.init_fuse 6", "unexpected in the checkpoint (dropped): none"):
        assert grp in line, line
    assert "\n" not in line and sorted(rep["missing"]) == sorted(k for k in before if S11.is_conditioning_key(k))
    after = dual.state_dict()
    for k in after:
        if S11.is_conditioning_key(k):
            assert torch.equal(after[k], before[k]), k                      # the constructor's initialisation
        elif k in ck11 and not k.startswith(("entropy_model_z._q", "entropy_model_z._o", "entropy_model_z._c", "entropy_model_y.")):
            assert torch.equal(after[k], ck11[k]), k
    assert not torch.equal(after["encoder.conv1.bias"], before["encoder.conv1.bias"])
    # the other way round names the unexpected groups; equal key sets print nothing
    rep2 = model11.load_learned_weight(_save(tmp_path, dual))
    assert "unexpected in the checkpoint (dropped): encoder.beta_ft_list 54" in weight_load_report(rep2) and "kept as initialised): none" in weight_load_report(rep2)
    assert weight_load_report(model11.load_learned_weight(path)) is None


def _save(tmp_path, model):
    p = str(tmp_path / "dual.pth.tar")
    torch.save({"iter": 1, "comp_model": {k: v.detach().clone() for k, v in model.state_dict().items()}}, p)
    return p


def test_cli_refuses_a_from_scratch_start_without_the_vqgan_before_any_gpu_work():
    """scripts/train.py on the project config (vq_model.ckpt_path: null) with neither --model_path nor --synthetic_weights ends with
    the refusal, on a machine without a GPU."""
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), CFG11, "--synthetic_data", "--allow_synthetic_lpips"],
                         capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert res.returncode != 0 and "subnet.vq_model.ckpt_path is absent" in res.stderr and "Traceback" not in res.stderr, res.stderr[-800:]
