"""Stage 1-3 training, host side (no GPU): the beta grid sampler, scripts/train.py's reading of the YAML's `loss` section, the
meaning of tests/golden/focal.npz (the reference's own FocalCrossEntropyLoss, tools/gen_focal_golden.py), the second public header
include/dcvic_loss.h against _lib.LOSS_SIGNATURES, and the focal kernel's host-side argument checks."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_cabi
from dc_vic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the beta grid sampler
def numpy_grid(rng, max_beta, num_levels, n):
    i = rng.randint(0, num_levels + 1, n)
    return np.float32(max_beta) * (i.astype(np.float32) / np.float32(num_levels))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("max_beta", [3.0, 3.5])
def test_sampler_is_the_numpy_expression(seed, n, max_beta):
    from dc_vic_amd.train.trainer import sample_beta_grid
    a, b = np.random.RandomState(seed), np.random.RandomState(seed)
    for _ in range(5):
        got, want = sample_beta_grid(a, max_beta, 100, n), numpy_grid(b, max_beta, 100, n)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (n,)
        assert np.array_equal(got.numpy(), want) and want.dtype == np.float32
        k = np.rint(got.numpy().astype(np.float64) * 100 / max_beta)
        assert np.array_equal(got.numpy(), np.float32(max_beta) * (k.astype(np.float32) / np.float32(100))) and k.min() >= 0 and k.max() <= 100


@pytest.mark.parametrize("max_beta", [3.0, 3.5])
def test_sampler_reaches_both_ends_and_replays_from_a_saved_state(max_beta):
    from dc_vic_amd.train.trainer import sample_beta_grid
    rng = np.random.RandomState(11)
    saved = rng.get_state()
    first = torch.cat([sample_beta_grid(rng, max_beta, 100, 8) for _ in range(250)])
    assert first.numel() == 2000 and float(first.min()) == 0.0 and float(first.max()) == max_beta
    assert len(set(first.tolist())) == 101
    rng.set_state(saved)
    again = torch.cat([sample_beta_grid(rng, max_beta, 100, 8) for _ in range(250)])
    assert torch.equal(first, again)


def test_trainer_draws_rate_then_vq_from_its_own_generator():
    """The trainer's `sample_beta_pair` on the function sequence (constructing a trainer needs a GPU): beta_rate from max_beta_rate
    first, then beta_vq from max_beta_vq, both from `self.rng`; with selected pairs it is sample_selected_beta_pair as before."""
    from types import SimpleNamespace as NS
    from dc_vic_amd.train.trainer import DualBetaCondGanDistortionVqCodeTrainer as Tr
    model = NS(use_selected_beta_pairs=False, max_beta_rate=3.0, max_beta_vq=3.5, num_beta_levels=100)
    me = NS(model=model, rng=np.random.RandomState(5))
    ref = np.random.RandomState(5)
    for n in (8, 1, 8):
        rate, vq = Tr.sample_beta_pair(me, n)
        assert np.array_equal(rate.numpy(), numpy_grid(ref, 3.0, 100, n)) and np.array_equal(vq.numpy(), numpy_grid(ref, 3.5, 100, n))
    model.num_beta_levels = 4
    rate, vq = Tr.sample_beta_pair(me, 64)
    assert set(rate.tolist()) <= {0.0, 0.75, 1.5, 2.25, 3.0} and set(vq.tolist()) <= {0.0, 0.875, 1.75, 2.625, 3.5}
    numpy_grid(ref, 3.0, 4, 64), numpy_grid(ref, 3.5, 4, 64)
    sel = NS(use_selected_beta_pairs=True, selected_beta_rate=[2.29, 0.16], selected_beta_vq=[3.0, 1.0])
    me2 = NS(model=sel, rng=np.random.RandomState(9), sample_selected_beta_pair=lambda n: Tr.sample_selected_beta_pair(me2, n))
    rate, vq = Tr.sample_beta_pair(me2, 8)
    i = np.random.RandomState(9).randint(0, 2, 8)
    assert rate.tolist() == [np.float32([2.29, 0.16][k]).item() for k in i] and vq.tolist() == [[3.0, 1.0][k] for k in i]


# ---------------------------------------------------------------------------------------------------- the YAML's loss section
@pytest.fixture(scope="module")
def read():
    from dc_vic_amd.train.losses import read_loss_section
    return read_loss_section


@pytest.fixture(scope="module")
def sections():
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        return json.load(f)


GAN = "DualBetaCondGanDistortionVqCodeTrainer"


def _opt(trainer=GAN, **entries):
    return {"trainer": {"type": trainer}, "loss": entries}


def test_every_reference_yaml_is_accepted(read, sections):
    assert sorted(sections) == ["dc_vic_oasis.yaml", "dc_vic_patchgan.yaml", "exp1_stage1_1.yaml", "exp1_stage1_2.yaml", "exp1_stage1_3.yaml",
                                "exp1_stage3.yaml"]
    for name, opt in sections.items():
        r = read(opt)
        assert r["distortion_factor"] == 0.25, name
    # the GAN-stage files and the two inference files: today's losses, with the weights the YAML gives
    for name in ("exp1_stage1_3.yaml", "exp1_stage3.yaml"):
        r = read(sections[name])
        assert r["code_ce"] == dict(type="CrossEntropyLoss", gamma=0.0, reduction="mean") and r["code_distortion_reduction"] == "mean"
        assert r["weights"] == dict(distortion=50.0, perceptual=1.0, gan=0.01, code_distortion=1.0, code_ce=0.5) and not r["per_sample"]
    for name in ("dc_vic_oasis.yaml", "dc_vic_patchgan.yaml"):
        r = read(sections[name])
        assert r["code_ce"]["type"] is None and r["weights"] == {} and r["code_distortion_reduction"] == "mean"
    # stage 1-1 / 1-2 name rate-distortion trainers (scripts/train.py refuses those by trainer.type): focal gamma 2 is read, their
    # rate_loss and per-sample `reduction: none` are passed over as those trainers' business
    r = read(sections["exp1_stage1_1.yaml"])
    assert r["code_ce"] == dict(type="FocalCrossEntropyLoss", gamma=2.0, reduction="mean") and r["weights"]["code_ce"] == 0.05 and r["per_sample"]
    r = read(sections["exp1_stage1_2.yaml"])
    assert r["code_ce"] == dict(type="FocalCrossEntropyLoss", gamma=2.0, reduction="none") and r["per_sample"]


def test_synthetic_config_is_accepted_with_todays_losses(read):
    from dc_vic_amd import BaseConfig
    from dc_vic_amd.train.losses import build_code_ce_loss
    from dc_vic_amd.train.trainer import DEFAULT_LOSS
    r = read(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"is_train": True}))
    assert r["distortion_factor"] == 0.25 and r["code_ce"]["type"] is None and r["weights"] == {} and r["code_distortion_reduction"] == "mean"
    assert build_code_ce_loss(r["code_ce"], 0.5) is None                     # the trainer's own default: A.cross_entropy_loss
    assert DEFAULT_LOSS == dict(distortion=50.0, perceptual=1.0, gan=0.01, code_distortion=1.0, code_ce=0.5)
    assert "CrossEntropyLoss" in r["line"] and "Focal" not in r["line"] and "0.25" in r["line"]
    # no loss section at all, and entries that give a weight only
    assert read({})["code_ce"]["type"] is None and read({"loss": None})["distortion_factor"] == 0.25
    r = read(_opt(code_ce_loss=dict(loss_weight=0.25), distortion_loss=dict(loss_weight=10)))
    assert r["weights"] == dict(code_ce=0.25, distortion=10.0) and r["code_ce"]["type"] is None and r["distortion_factor"] == 0.25


def test_focal_choice_reaches_the_loss_object(read):
    from dc_vic_amd.registry import LOSS_REGISTRY
    from dc_vic_amd.train.losses import CrossEntropyLoss, FocalCrossEntropyLoss, build_code_ce_loss
    assert LOSS_REGISTRY.get("CrossEntropyLoss") is CrossEntropyLoss and LOSS_REGISTRY.get("FocalCrossEntropyLoss") is FocalCrossEntropyLoss
    r = read(_opt(code_ce_loss=dict(type="FocalCrossEntropyLoss", gamma=2.0, loss_weight=0.05)))
    obj = build_code_ce_loss(r["code_ce"], r["weights"]["code_ce"])
    assert isinstance(obj, FocalCrossEntropyLoss) and (obj.loss_weight, obj.gamma, obj.reduction) == (0.05, 2.0, "mean")
    assert "FocalCrossEntropyLoss(gamma=2, mean)" in r["line"]
    r = read(_opt(code_ce_loss=dict(type="FocalCrossEntropyLoss", gamma=0, reduction="sum", loss_weight=1)))
    obj = build_code_ce_loss(r["code_ce"], 1.0)
    assert (obj.gamma, obj.reduction) == (0.0, "sum")
    obj = build_code_ce_loss(read(_opt(code_ce_loss=dict(type="CrossEntropyLoss", loss_weight=0.5, ce_kwargs={})))["code_ce"], 0.5)
    assert isinstance(obj, CrossEntropyLoss) and obj.loss_weight == 0.5
    # the classes refuse, with the reason, what the section reader refuses
    for kw, word in ((dict(gamma=2.0, reduction="none"), "per-sample"), (dict(gamma=0.5), "gamma: 0.5"), (dict(gamma=-1), "gamma: -1"),
                     (dict(gamma=2.0, ignore_index=3), "ignore_index")):
        with pytest.raises(ValueError, match=word):
            FocalCrossEntropyLoss(0.05, **kw)
    with pytest.raises(ValueError, match="ce_kwargs"):
        CrossEntropyLoss(0.5, ce_kwargs=dict(label_smoothing=0.1))
    with pytest.raises(ValueError, match="reduction"):
        CrossEntropyLoss(0.5, reduction="sum")


@pytest.mark.parametrize("entries,words", [
    (dict(code_ce_loss=dict(type="FocalCrossEntropyLoss", gamma=2.0, reduction="none")), ("loss.code_ce_loss.reduction", "none")),
    (dict(code_ce_loss=dict(type="FocalCrossEntropyLoss", gamma=0.5)), ("loss.code_ce_loss.gamma", "0.5")),
    (dict(code_ce_loss=dict(type="FocalCrossEntropyLoss", gamma=-1)), ("loss.code_ce_loss.gamma", "-1")),
    (dict(code_ce_loss=dict(type="CrossEntropyLoss", ce_kwargs=dict(label_smoothing=0.1))), ("loss.code_ce_loss.ce_kwargs", "label_smoothing")),
    (dict(distortion_loss=dict(type="L1Loss", loss_weight=1.0)), ("loss.distortion_loss.type", "L1Loss")),
    (dict(distortion_loss=dict(type="MSSSIMLoss", loss_weight=1.0)), ("loss.distortion_loss.type", "MSSSIMLoss")),
    (dict(code_ce_loss=dict(type="NoSuchLoss")), ("loss.code_ce_loss.type", "NoSuchLoss")),
    (dict(code_distortion_loss=dict(type="NoSuchLoss")), ("loss.code_distortion_loss.type", "NoSuchLoss")),
    (dict(perceptual_loss=dict(type="LPIPSLoss", net="vgg")), ("loss.perceptual_loss.net", "vgg")),
    (dict(perceptual_loss=dict(type="LPIPSLoss")), ("loss.perceptual_loss.net", "vgg")),                 # the reference's default net
    (dict(perceptual_loss=dict(type="LPIPSLoss", net="alex", range_norm=True)), ("loss.perceptual_loss.range_norm", "True")),
    (dict(perceptual_loss=dict(type="DISTSLoss")), ("loss.perceptual_loss.type", "DISTSLoss")),
    (dict(distortion_loss=dict(type="MSELoss", mse_scale="0_100")), ("loss.distortion_loss.mse_scale", "0_100")),
    (dict(code_distortion_loss=dict(type="VanillaMSELoss", reduction="none")), ("loss.code_distortion_loss.reduction", "none")),
    (dict(code_ce_loss=dict(type="FocalCrossEntropyLoss", gamma=2.0, ignore_index=0)), ("loss.code_ce_loss.ignore_index", "0")),
    (dict(code_ce_loss=dict(type="FocalCrossEntropyLoss")), ("loss.code_ce_loss.gamma", "missing")),
    (dict(rate_loss=dict(type="RateLoss", loss_weight=0.5)), ("loss.rate_loss", "RateLoss")),
    (dict(style_loss=dict(type="StyleLoss")), ("loss.style_loss", "StyleLoss")),
])
def test_loss_section_refusals_name_the_key_and_the_value(read, entries, words):
    for trainer in (GAN, None):
        opt = _opt(trainer, **entries) if trainer else {"loss": entries}
        with pytest.raises(SystemExit) as e:
            read(opt)
        msg = str(e.value)
        for w in words:
            assert w in msg, msg


@pytest.mark.parametrize("normalize_img,mse_scale,factor", [
    (True, "0_1", 0.25), (False, "0_1", 0.25), (True, "0_255", (255.0 / 2.0) ** 2), (False, "0_255", 255.0 ** 2 / 4000.0)])
def test_mse_distortion_factors(read, normalize_img, mse_scale, factor):
    """distortion_loss.py:11-39 on [-1, 1] images, restated with torch: the factor multiplies mean((a - b)^2)."""
    r = read(_opt(distortion_loss=dict(type="MSELoss", loss_weight=50, normalize_img=normalize_img, mse_scale=mse_scale)))
    assert r["distortion_factor"] == factor
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand((2, 3, 8, 8), generator=g, dtype=torch.float64) * 2 - 1, torch.rand((2, 3, 8, 8), generator=g, dtype=torch.float64) * 2 - 1
    fn = {"0_255": lambda t: (t + 1.) / 2. * 255., "0_1": lambda t: (t + 1.) / 2.}[mse_scale]
    alpha = 1 if normalize_img else {"0_255": (255 ** 2) / 4000, "0_1": 1 / 4}[mse_scale]
    want = alpha * (F.mse_loss(fn(a), fn(b)) if normalize_img else F.mse_loss(a, b))
    assert abs(float(want) - factor * float(F.mse_loss(a, b))) <= 1e-12 * float(want)
    # MSELoss's own defaults: un-normalised 0_255
    assert read(_opt(distortion_loss=dict(type="MSELoss", loss_weight=1)))["distortion_factor"] == 255.0 ** 2 / 4000.0
    assert read(_opt(code_distortion_loss=dict(type="VanillaMSELoss", reduction="sum")))["code_distortion_reduction"] == "sum"


# ---------------------------------------------------------------------------------------------------- the fixture
def focal_fp64(logits, target, gamma, weight, reduction):
    """FocalCrossEntropyLoss.forward (cross_entropy_loss.py:42-53) in plain torch fp64."""
    lg = torch.as_tensor(logits).double() if not isinstance(logits, torch.Tensor) else logits
    tgt = torch.as_tensor(target).long()
    ce = F.cross_entropy(lg, tgt, reduction="none")
    pt = F.softmax(lg, dim=1).gather(1, tgt.unsqueeze(1)).squeeze(1)
    f = ((1 - pt) ** gamma) * ce
    return weight * (f.mean() if reduction == "mean" else f.sum())


def test_fixture_is_the_fp64_restatement():
    """Value within 2e-6 (relative), gradient within 2e-5 of its max: the fixture is the reference's fp32, which stays within 1.1e-7
    and 5.2e-7 of fp64 on such shapes."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "focal.npz"))
    w = float(G["loss_weight"])
    assert w == 0.05 and G["logits"].shape == (2, 256, 8, 8) and G["logits"].dtype == np.float32
    tgt = G["target"]
    assert tgt.shape == (2, 8, 8) and tgt.dtype == np.int64 and tgt.min() == 0 and tgt.max() == 255
    assert list(G["gammas"]) == [0.0, 1.0, 2.0] and list(G["reductions"]) == ["mean", "sum"]
    for gamma in (0.0, 1.0, 2.0):
        for red in ("mean", "sum"):
            lg = torch.from_numpy(G["logits"]).double().requires_grad_(True)
            val = focal_fp64(lg, tgt, gamma, w, red)
            val.backward()
            val = val.detach()
            got_v, got_g = float(G[f"loss_g{gamma:g}_{red}"]), torch.from_numpy(G[f"grad_g{gamma:g}_{red}"]).double()
            ev = abs(got_v - float(val)) / abs(float(val))
            eg = float((got_g - lg.grad).abs().max()) / float(lg.grad.abs().max())
            print(f"[focal fixture] gamma {gamma:g} {red}: value {got_v:.9e} rel err {ev:.2e}, gradient err / max {eg:.2e}")
            assert ev <= 2e-6 and eg <= 2e-5, (gamma, red, ev, eg)
    # gamma 0 is plain cross entropy
    assert abs(float(G["loss_g0_mean"]) - w * float(F.cross_entropy(torch.from_numpy(G["logits"]).double(), torch.from_numpy(tgt)))) <= 2e-6 * 0.4


# ---------------------------------------------------------------------------------------------------- the second header
def loss_header_prototypes(path):
    """test_cabi.declared_prototypes for a header given by path (same mapping to ctypes)."""
    scalars = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^(\w[\w \t]*?\**)\s*\b(dcvic_\w+)\s*\(([^()]*)\)\s*;", txt, flags=re.M):
        ret = " ".join(ret.split())
        restype = C.c_char_p if ret == "const char*" else C.c_void_p if "*" in ret else None if ret == "void" else scalars[ret]
        argtypes = []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            if "*" in prm:
                argtypes.append(C.c_void_p)
                continue
            words = prm.split()
            ty = " ".join(words)
            argtypes.append(scalars[ty] if ty in scalars else scalars[" ".join(words[:-1])])
        assert name not in protos, f"{name} declared twice"
        protos[name] = (restype, argtypes)
    return protos


def test_loss_header_matches_its_signature_table():
    main = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic.h"))
    assert main == test_cabi.declared_prototypes()                       # the copy of the parser reads dcvic.h as the original does
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_loss.h"))
    assert sorted(protos) == ["dcvic_focal_ce_f32", "dcvic_focal_ce_workspace_doubles"]
    assert protos["dcvic_focal_ce_workspace_doubles"] == (C.c_longlong, [C.c_int, C.c_int])
    assert protos["dcvic_focal_ce_f32"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_int, C.c_int, C.c_void_p])
    assert test_cabi.signature_mismatches(_lib.LOSS_SIGNATURES, protos) == []
    assert not set(protos) & set(main) and not set(_lib.LOSS_SIGNATURES) & set(_lib.SIGNATURES)
    assert not set(_lib.LOSS_SIGNATURES) & set(_lib.SYMBOLS)
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the comparison catches a double declared as float and a missing parameter
    for sig in ("i:ppfdpppiiip", "i:ppddpppiip", "q:ppddpppiiip"):
        bad = test_cabi.signature_mismatches(dict(_lib.LOSS_SIGNATURES, dcvic_focal_ce_f32=sig), protos)
        assert len(bad) == 1 and bad[0].startswith("dcvic_focal_ce_f32:"), (sig, bad)
    # the host-side size query: one double per 64-position workgroup, nothing for an empty tensor
    assert L.dcvic_focal_ce_workspace_doubles(8, 1024) == 8 * 16 and L.dcvic_focal_ce_workspace_doubles(3, 77) == 3 * 2
    assert L.dcvic_focal_ce_workspace_doubles(0, 64) == 0 and L.dcvic_focal_ce_workspace_doubles(2, 0) == 0


# focal_ce(logits, target, gamma, scale, loss, dlogits, workspace, N, C, HW, stream); baseline N = 2, C = 4, HW = 16.  Every case
# breaks one rule and keeps the others valid (see test_cabi._NO_GPU_PRELUDE: every GPU hidden, dummy non-null addresses).
_FOCAL_ARG_CHECKS = r"""
D = C.c_double
def fc(logits=P, target=P, gamma=2.0, scale=1.0, loss=P, dl=P, ws=P, N=2, Cc=4, HW=16):
    return L.dcvic_focal_ce_f32(logits, target, D(gamma), D(scale), loss, dl, ws, N, Cc, HW, None)
for kw in (dict(N=0), dict(Cc=0), dict(HW=0)):
    err(fc(**kw), "focal_ce", "empty")
err(fc(Cc=1), "focal_ce", "C=1")
err(fc(gamma=0.5), "focal_ce", "gamma=0.5")
err(fc(gamma=-1.0), "focal_ce", "gamma=-1")
err(fc(gamma=float("nan")), "focal_ce", "gamma")
for kw in (dict(logits=None), dict(loss=None), dict(ws=None), dict(target=None)):
    err(fc(**kw), "focal_ce", "null pointer")
for kw in (dict(logits=None, dl=None), dict(loss=None, dl=None), dict(ws=None, dl=None)):     # the value-only call checks the same
    err(fc(**kw), "focal_ce", "null pointer")
err(fc(Cc=1 << 20, HW=1 << 12), "focal_ce", "too large")
print("CHECKS_OK")
"""


def test_focal_argument_checks_without_gpu():
    """dcvic_focal_ce_f32 rejects zero sizes, C = 1, a gamma in (0, 1) or below 0 and null pointers with a message, before any launch."""
    test_cabi._run_without_gpu(_FOCAL_ARG_CHECKS)
