"""Stage 1-2 training, host side (no GPU): the trainer's registry name and scripts/train.py's choice of it, the per-sample weight vector of the code losses against `apply_loss_weight` restated in
torch fp64, the meaning of tests/golden/sample_loss.npz (the reference's own losses, tools/gen_sample_loss_golden.py), the sixth
public header include/dcvic_sample_loss.h against _lib.SAMPLE_LOSS_SIGNATURES, and the host-side argument checks of its two entry
points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_cabi
from dc_vic_amd import _lib
from test_focal_host import loss_header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCTIONS = ("none", "mean", "sum")
RD, RD_1_1 = "DualBetaCondRateDistortionVqCodeTrainer", "RateDistortionVqCodeTrainer"


# ---------------------------------------------------------------------------------------------------- the trainer and the CLI's choice
@pytest.fixture(scope="module")
def cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dcvic_train_cli_rd", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def sections():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        return json.load(f)


def test_trainer_resolves_from_the_registry():
    import dc_vic_amd.train as T
    from dc_vic_amd.registry import TRAINER_REGISTRY
    from dc_vic_amd.train.trainer import BetaPairTrainerBase
    cls = TRAINER_REGISTRY.get(RD)
    assert cls is T.DualBetaCondRateDistortionVqCodeTrainer and issubclass(cls, BetaPairTrainerBase)
    gan = TRAINER_REGISTRY.get("DualBetaCondGanDistortionVqCodeTrainer")
    assert issubclass(gan, BetaPairTrainerBase) and not issubclass(cls, gan)
    # validation, the beta samplers and LPIPS loading are the shared base's, not copies
    for name in ("validation", "validation_beta_pairs", "sample_beta_pair", "sample_selected_beta_pair", "load_lpips_state"):
        assert getattr(cls, name) is getattr(gan, name) is getattr(BetaPairTrainerBase, name), name


def test_cli_chooses_the_rate_distortion_trainer(cli, sections):
    kind, name, reason = cli.choose_trainer(sections["exp1_stage1_2.yaml"])
    assert (kind, name) == ("rd", RD) and "trainer.type" in reason
    # every other config goes to choose_gan_trainer unchanged
    for cfg in ("exp1_stage1_3.yaml", "exp1_stage3.yaml"):
        assert cli.choose_trainer(sections[cfg]) == cli.choose_gan_trainer(sections[cfg])
        assert cli.choose_trainer(sections[cfg], "vanilla") == cli.choose_gan_trainer(sections[cfg], "vanilla")
    from dc_vic_amd.train.losses import read_loss_section
    r = read_loss_section(sections["exp1_stage1_2.yaml"])
    assert r["rate"] == dict(loss_weight=0.5, reduction="none") and r["per_sample"] and r["code_distortion_reduction"] == "none"
    assert read_loss_section(sections["exp1_stage3.yaml"])["rate"] is None


@pytest.mark.parametrize("change,flag,words", [
    (dict(trainer=dict(type=RD_1_1)), None, (RD_1_1, "not built", "HyperpriorCharmVicModel", "LinearWarmupScheduler")),
    ({}, "oasis", ("--gan oasis", RD)),
    ({}, "vanilla", ("--gan vanilla", RD)),
    (dict(model=dict(gumbel_sampling=True)), None, ("model.gumbel_sampling", "not built")),
    (dict(trainer=dict(type=RD, beta_policy="cosine")), None, ("trainer.beta_policy", "cosine")),
])
def test_cli_refusals_before_any_gpu_work(cli, sections, change, flag, words):
    opt = dict(sections["exp1_stage1_2.yaml"], **change)
    with pytest.raises(SystemExit) as e:
        cli.choose_trainer(opt, flag)
    for w in words:
        assert w in str(e.value), str(e.value)
    with pytest.raises(SystemExit):                          # stage 1-1 as the reference ships it
        cli.choose_trainer(sections["exp1_stage1_1.yaml"])


# the four fall-back values of a config without an `optim` section (the golden sections hold `loss` and `trainer` only)
OPTIM_DEFAULTS = dict(milestones=[300000], gamma=0.1, clip_max_norm=1.0)      # and lr 1e-4, under each trainer's own name


def test_rd_trainer_kwargs_of_the_stage_1_2_section(cli, sections):
    """train/build.py's mapping against the arguments scripts/train.py's build_rd_trainer, tools/train_bench.py's rd_trainer and
    tests/test_gpu_rd_trainer.py's build_trainer each spelt before it existed (the three agreed, defaults filled in), written out."""
    from dc_vic_amd.train.build import build_rd_trainer, rd_trainer_kwargs
    from dc_vic_amd.train.losses import read_loss_section
    opt = sections["exp1_stage1_2.yaml"]
    assert rd_trainer_kwargs(opt, read_loss_section(opt)) == dict(
        lr=1e-4, aux_lr=1e-3, **OPTIM_DEFAULTS,
        loss_weights=dict(distortion=50.0, perceptual=1.0, code_distortion=0.006, code_ce=0.003, rate=0.5),
        beta_policy="exp", beta_offset=1.0, sample_beta_batch=True, rate_reduction="none", code_ce_gamma=2.0, code_ce_reduction="none",
        code_distortion_reduction="none", distortion_factor=0.25, distortion_type="MSELoss", gumbel_sampling=False)
    # an `optim` section is read, not defaulted over
    o2 = dict(opt, optim=dict(g_optimizer=dict(lr=2e-4), aux_optimizer=dict(lr=5e-3), g_scheduler=dict(milestones=[10, 20], gamma=0.5), clip_max_norm=None))
    kw = rd_trainer_kwargs(o2, read_loss_section(o2))
    assert (kw["lr"], kw["aux_lr"], kw["milestones"], kw["gamma"], kw["clip_max_norm"]) == (2e-4, 5e-3, [10, 20], 0.5, None)
    assert cli.build_rd_trainer is build_rd_trainer          # the CLI's names are the package's, not wrappers


@pytest.mark.parametrize("cfg", ["exp1_stage3.yaml", "exp1_stage1_3.yaml", "dc_vic_oasis.yaml", "dc_vic_patchgan.yaml", "focal"])
def test_gan_trainer_kwargs_of_the_gan_sections(cli, sections, cfg):
    """The arguments scripts/train.py's main() passed to the GAN trainers, written out: the two stage configs give every weight and a
    CrossEntropyLoss object, the two discriminator configs (no `loss` section) leave the trainer's defaults; "focal" is stage 1-3 with
    the FocalCrossEntropyLoss entry the reference's stage 1-1 file carries, mean -> sum."""
    from dc_vic_amd.train.build import gan_trainer_kwargs, read_gumbel_options
    from dc_vic_amd.train.losses import CrossEntropyLoss, FocalCrossEntropyLoss, read_loss_section
    opt = sections["exp1_stage1_3.yaml" if cfg == "focal" else cfg]
    if cfg == "focal":
        opt = dict(opt, loss=dict(opt["loss"], code_ce_loss=dict(type="FocalCrossEntropyLoss", loss_weight=0.05, gamma=2.0, reduction="sum")),
                   model=dict(gumbel_sampling=True, gumbel_kwargs=dict(tau=0.5)))
    assert cli.read_gumbel_options is read_gumbel_options
    kw = gan_trainer_kwargs(opt, read_loss_section(opt), read_gumbel_options(opt))
    ce = kw.pop("code_ce_loss")
    has_loss = opt.get("loss") is not None
    lw = dict(distortion=50.0, perceptual=1.0, gan=0.01, code_distortion=1.0, code_ce=0.05 if cfg == "focal" else 0.5) if has_loss else {}
    assert kw == dict(lr_g=1e-4, lr_d=1e-4, **OPTIM_DEFAULTS, loss_weights=lw, sample_beta_batch=True, d_milestones=None, d_gamma=None,
                      distortion_factor=0.25, code_distortion_reduction="mean", gumbel_sampling=cfg == "focal",
                      gumbel_kwargs=dict(tau=0.5 if cfg == "focal" else 1.0))
    if cfg == "focal":
        assert type(ce) is FocalCrossEntropyLoss and (ce.loss_weight, ce.gamma, ce.reduction) == (0.05, 2.0, "sum")
    elif has_loss:
        assert type(ce) is CrossEntropyLoss and ce.loss_weight == 0.5
    else:
        assert ce is None
    # the discriminator's schedule is its own YAML entry
    o2 = dict(opt, optim=dict(d_optimizer=dict(lr=3e-4), d_scheduler=dict(milestones=[7], gamma=0.3)))
    kw = gan_trainer_kwargs(o2, read_loss_section(o2), read_gumbel_options(o2))
    assert (kw["lr_g"], kw["lr_d"], kw["d_milestones"], kw["d_gamma"], kw["milestones"]) == (1e-4, 3e-4, [7], 0.3, [300000])


def test_main_parameter_rule_and_beta_weights():
    from dc_vic_amd.train.rd_trainer import DEFAULT_RD_LOSS, LOG_KEYS, beta_loss_weights, is_main_parameter
    assert is_main_parameter("encoder.conv1.weight") and is_main_parameter("entropy_model_z._matrix0") and is_main_parameter("fusion_module.x.weight")
    assert not is_main_parameter("vq_model.decoder.conv_in.weight") and not is_main_parameter("entropy_model_z.quantiles")
    b_vq, b_rate = torch.tensor([3.0, 1.5]), torch.tensor([2.29, 0.62])
    for policy in ("linear", "exp"):
        vq, rate = beta_loss_weights(policy, 1.0, b_vq, b_rate)
        assert torch.equal(vq, beta_weight(policy, b_vq)) and torch.equal(rate, beta_weight(policy, b_rate))
    with pytest.raises(ValueError, match="beta_policy"):
        beta_loss_weights("cosine", 1.0, b_vq, b_rate)
    assert DEFAULT_RD_LOSS == dict(rate=0.5, distortion=50.0, perceptual=1.0, code_distortion=0.006, code_ce=0.003)
    assert LOG_KEYS == ("rate", "distortion", "perceptual", "code_distortion", "code_ce", "total", "qbpp", "vq_acc", "lr", "aux")


# ---------------------------------------------------------------------------------------------------- the weight vector
def apply_loss_weight(loss, weight):
    """dual_cond_rate_distortion_vq_code_trainer.py:92-98."""
    assert weight.ndim == 1
    if loss.ndim > 1:
        loss = loss.mean(dim=tuple(range(1, loss.ndim)))
    return (loss * weight).mean()


def beta_weight(policy, beta, offset=1.0):
    """calc_vq_rate_loss_weight, :71-78."""
    return beta + offset if policy == "linear" else torch.exp(beta)


def focal_map(lg, tgt, gamma):
    ce = F.cross_entropy(lg, tgt, reduction="none")
    pt = F.softmax(lg, dim=1).gather(1, tgt.unsqueeze(1)).squeeze(1)
    return ((1 - pt) ** gamma) * ce


def reduce_map(m, reduction):
    return m if reduction == "none" else m.mean() if reduction == "mean" else m.sum()


@pytest.mark.parametrize("n_beta", ["N", "1"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("policy", ["linear", "exp"])
@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_sample_loss_weights_are_apply_loss_weight(reduction, policy, N, n_beta):
    """sum_n w[n] * S[n] against the reference's expression in torch fp64, within 1e-12 relative (w itself kept in fp64 for the
    comparison: its rounding to fp32 is one ulp per image and is checked apart), for a focal map [N, H, W] and a squared-error map
    [N, C, H, W]."""
    from dc_vic_amd.train.losses import sample_loss_weights
    g = torch.Generator().manual_seed(7 + N)
    beta = torch.rand(N if n_beta == "N" else 1, generator=g, dtype=torch.float64) * 3
    bw = beta_weight(policy, beta, 1.0)
    lg, tgt = torch.randn((N, 6, 3, 5), generator=g, dtype=torch.float64), torch.randint(0, 6, (N, 3, 5), generator=g)
    a, b = torch.randn((N, 4, 3, 5), generator=g, dtype=torch.float64), torch.randn((N, 4, 3, 5), generator=g, dtype=torch.float64)
    for lw, m in ((0.05, focal_map(lg, tgt, 2.0)), (1.0, (a - b) ** 2)):
        want = apply_loss_weight(lw * reduce_map(m, reduction), bw)
        S = m.reshape(N, -1).sum(dim=1)
        elems = m[0].numel()
        w = sample_loss_weights(lw, reduction, N, elems, bw.float())
        assert w.dtype == torch.float32 and tuple(w.shape) == (N,) and w.is_contiguous()
        # the same expression before the rounding of beta_weight and w to fp32
        if reduction == "none":
            w64 = (bw * (lw / (N * elems))).expand(N)
        else:
            w64 = (bw.mean() * (lw / (N * elems if reduction == "mean" else 1))).expand(N)
        got = float((w64 * S).sum())
        assert abs(got - float(want)) <= 1e-12 * abs(float(want)), (reduction, policy, N, got, float(want))
        assert float((w.double() - w64).abs().max()) <= 2.0 ** -22 * float(w64.abs().max())       # beta_weight.float(), then w: two roundings
    with pytest.raises(ValueError, match="beta_weight"):
        sample_loss_weights(1.0, reduction, N, 4, torch.ones(N + 1))
    with pytest.raises(ValueError, match="reduction"):
        sample_loss_weights(1.0, "batchmean", N, 4, torch.ones(N))


def test_sample_loss_weights_and_rate_weights_are_the_same_three_cases():
    """RateLoss.sample_weights (bits[n] / num_pixel per image) and sample_loss_weights on a map of num_pixel elements state one rule:
    equal bits for none and mean; for sum the rate term alone keeps its division by num_pixel (it sums bpp, not bits)."""
    from dc_vic_amd.train.losses import RateLoss, sample_loss_weights
    bw = torch.tensor([1.5, 4.0, 0.25])
    for red in ("none", "mean"):
        assert torch.equal(RateLoss(0.7, reduction=red).sample_weights(3, 4096, bw), sample_loss_weights(0.7, red, 3, 4096, bw)), red
    assert torch.equal(RateLoss(0.7, reduction="sum").sample_weights(3, 4096, bw) * 4096, sample_loss_weights(0.7, "sum", 3, 4096, bw))     # 4096 = 2^12: exact


# ---------------------------------------------------------------------------------------------------- the fixture
def test_fixture_is_the_fp64_restatement_and_the_weight_vector():
    """tests/golden/sample_loss.npz against the expressions above in fp64 (value within 2e-6 relative, gradient within 2e-5 of its max,
    the bounds test_focal_host.py holds focal.npz to), and sum_n w[n] * S[n] with sample_loss_weights' w against the fixture's values."""
    from dc_vic_amd.train.losses import sample_loss_weights
    G = np.load(os.path.join(ROOT, "tests", "golden", "sample_loss.npz"))
    assert G["logits"].shape == (3, 64, 4, 4) and G["logits"].dtype == np.float32 and G["target"].dtype == np.int64
    assert G["target"].min() == 0 and G["target"].max() == 63 and G["latent"].shape == (3, 4, 4, 4)
    assert list(G["policies"]) == ["linear", "exp"] and list(G["reductions"]) == list(REDUCTIONS) and list(G["beta_vq"]) == [3.0, 0.0, 1.5]
    ce_w, gamma, mse_w, off = float(G["ce_weight"]), float(G["gamma"]), float(G["mse_weight"]), float(G["beta_offset"])
    assert (ce_w, gamma, mse_w, off) == (0.05, 2.0, 1.0, 1.0)
    tgt = torch.from_numpy(G["target"])
    for policy in ("linear", "exp"):
        bw = beta_weight(policy, torch.from_numpy(G["beta_vq"]).double(), off)
        for red in REDUCTIONS:
            lg = torch.from_numpy(G["logits"]).double().requires_grad_(True)
            fm = focal_map(lg, tgt, gamma)
            val = apply_loss_weight(ce_w * reduce_map(fm, red), bw)
            val.backward()
            lt = torch.from_numpy(G["latent"]).double().requires_grad_(True)
            sm = (torch.from_numpy(G["gt_latent"]).double() - lt) ** 2
            val2 = apply_loss_weight(mse_w * reduce_map(sm, red), bw)
            val2.backward()
            for name, v, grad, m, lw in (("ce", val, lg.grad, fm.detach(), ce_w), ("mse", val2, lt.grad, sm.detach(), mse_w)):
                got_v, got_g = float(G[f"{name}_{policy}_{red}"]), torch.from_numpy(G[f"{name}_grad_{policy}_{red}"]).double()
                ev = abs(got_v - float(v.detach())) / abs(float(v.detach()))
                eg = float((got_g - grad).abs().max()) / float(grad.abs().max())
                S = m.reshape(3, -1).sum(dim=1)
                w = sample_loss_weights(lw, red, 3, m[0].numel(), bw.float()).double()
                ew = abs(float((w * S).sum()) - got_v) / abs(got_v)
                print(f"[sample_loss fixture] {name} {policy} {red}: value {got_v:.9e} rel err {ev:.2e}, gradient err / max {eg:.2e}, sum w S err {ew:.2e}")
                assert ev <= 2e-6 and eg <= 2e-5 and ew <= 2e-6, (name, policy, red, ev, eg, ew)


# ---------------------------------------------------------------------------------------------------- the sixth header
def test_sample_loss_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_sample_loss.h"))
    P, I, Q, D = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    assert protos == {
        "dcvic_focal_ce_sample_workspace_doubles": (Q, [I, I]),
        "dcvic_focal_ce_sample_f32": (I, [P, P, P, D, P, P, P, P, I, I, I, P]),
        "dcvic_sq_err_sample_workspace_doubles": (Q, [I, Q]),
        "dcvic_sq_err_sample_f32": (I, [P, Q, P, P, P, P, P, P, I, Q, P]),
    }
    assert test_cabi.signature_mismatches(_lib.SAMPLE_LOSS_SIGNATURES, protos) == []
    others = set()
    for h in ("dcvic.h", "dcvic_loss.h", "dcvic_rate.h", "dcvic_train.h", "dcvic_vq.h"):
        others |= set(loss_header_prototypes(os.path.join(ROOT, "include", h)))
    assert not set(protos) & others
    tables = set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.RATE_SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VQ_SIGNATURES)
    assert not set(_lib.SAMPLE_LOSS_SIGNATURES) & tables and not set(_lib.SAMPLE_LOSS_SIGNATURES) & set(_lib.SYMBOLS)
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the comparison catches a double declared as float, a missing parameter and a narrowed M
    for name, sig in (("dcvic_focal_ce_sample_f32", "i:pppfppppiiip"), ("dcvic_focal_ce_sample_f32", "i:pppdpppiiip"), ("dcvic_sq_err_sample_f32", "i:pqppppppiip"),
                      ("dcvic_sq_err_sample_workspace_doubles", "q:ii")):
        bad = test_cabi.signature_mismatches(dict(_lib.SAMPLE_LOSS_SIGNATURES, **{name: sig}), protos)
        assert len(bad) == 1 and bad[0].startswith(name + ":"), (sig, bad)
    # the host-side size queries: one double per 64-position workgroup; one per 2048 elements up to 64 per image, then a grid stride
    assert L.dcvic_focal_ce_sample_workspace_doubles(8, 1024) == 8 * 16 == L.dcvic_focal_ce_workspace_doubles(8, 1024)
    assert L.dcvic_focal_ce_sample_workspace_doubles(3, 77) == 3 * 2 and L.dcvic_focal_ce_sample_workspace_doubles(0, 64) == 0
    sq = L.dcvic_sq_err_sample_workspace_doubles
    assert sq(1, 1) == 1 and sq(3, 2048) == 3 and sq(3, 2049) == 6 and sq(8, 4096) == 16 and sq(2, 64 * 2048) == 128 and sq(2, 64 * 2048 + 1) == 128
    assert sq(2, 1 << 33) == 128 and sq(0, 5) == 0 and sq(2, 0) == 0 and sq(-1, 5) == 0


# Every case breaks one rule and keeps the others valid (see test_cabi._NO_GPU_PRELUDE: every GPU hidden, dummy non-null addresses).
# focal_ce_sample(logits, target, w, gamma, loss, dlogits, per_sample, workspace, N, C, HW, stream); baseline N = 2, C = 4, HW = 16
# sq_err_sample(a, a_bs, b, w, loss, da, per_sample, workspace, N, M, stream); baseline N = 2, M = 48, a_bs = 64
_SAMPLE_ARG_CHECKS = r"""
D = C.c_double
def fc(logits=P, target=P, w=P, gamma=2.0, loss=P, dl=P, per=P, ws=P, N=2, Cc=4, HW=16):
    return L.dcvic_focal_ce_sample_f32(logits, target, w, D(gamma), loss, dl, per, ws, N, Cc, HW, None)
for kw in (dict(N=0), dict(Cc=0), dict(HW=0)):
    err(fc(**kw), "focal_ce_sample", "empty")
err(fc(Cc=1), "focal_ce_sample", "C=1")
err(fc(gamma=0.5), "focal_ce_sample", "gamma=0.5")
err(fc(gamma=-1.0), "focal_ce_sample", "gamma=-1")
err(fc(gamma=float("nan")), "focal_ce_sample", "gamma")
for kw in (dict(logits=None), dict(target=None), dict(w=None), dict(loss=None), dict(ws=None)):
    err(fc(**kw), "focal_ce_sample", "null pointer")
    err(fc(dl=None, per=None, **kw), "focal_ce_sample", "null pointer")           # the value-only call checks the same
err(fc(Cc=1 << 20, HW=1 << 12), "focal_ce_sample", "too large")

def sq(a=P, a_bs=64, b=P, w=P, loss=P, da=P, per=P, ws=P, N=2, M=48):
    return L.dcvic_sq_err_sample_f32(a, LL(a_bs), b, w, loss, da, per, ws, N, LL(M), None)
for kw in (dict(N=0), dict(M=0), dict(N=-1)):
    err(sq(**kw), "sq_err_sample", "empty")
err(sq(a_bs=47), "sq_err_sample", "batch stride")
err(sq(a_bs=0), "sq_err_sample", "batch stride")
for kw in (dict(a=None), dict(b=None), dict(w=None), dict(loss=None), dict(ws=None)):
    err(sq(**kw), "sq_err_sample", "null pointer")
    err(sq(da=None, per=None, **kw), "sq_err_sample", "null pointer")
err(sq(N=1 << 30, M=1 << 20, a_bs=1 << 20), "sq_err_sample", "too large")
err(sq(N=1, M=(1 << 40) + 1, a_bs=1 << 41), "sq_err_sample", "too large")
print("CHECKS_OK")
"""


def test_sample_loss_argument_checks_without_gpu():
    """Both entry points reject zero sizes, C = 1, a gamma in (0, 1) or below 0, every required null pointer (w among them) and a batch
    stride below the map with a message that starts with their name, before any launch."""
    test_cabi._run_without_gpu(_SAMPLE_ARG_CHECKS)
