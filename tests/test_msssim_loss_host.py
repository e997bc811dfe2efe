"""MSSSIMLoss / L1Loss for the rate-distortion trainer, what holds without a GPU: the restatement tests/msssim_loss_ref.py itself
(its autograd gradient against central differences, the two closed-form cases), the window, the workspace formula, the header
include/dcvic_msssim_loss.h against _lib.MSSSIM_LOSS_SIGNATURES, the entry points' refusals (all of them come before any launch), and the
YAML rules: the two types are read under the rate-distortion trainer only."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

import msssim_loss_ref as R
import test_cabi
from dc_vic_amd import _lib
from test_focal_host import loss_header_prototypes
from test_ssim_host import scale_sizes, ssim_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD, GAN = "DualBetaCondRateDistortionVqCodeTrainer", "DualBetaCondGanDistortionVqCodeTrainer"


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_gradient_matches_central_differences():
    """fp64, 1 x 3 x 161 x 161 (every pool pads, the last valid map is 1 x 1): the directional derivative along 8 random directions."""
    shape = (1, 3, 161, 161)
    real, fake = R.pair(shape, "far")
    _, g = R.value_and_grad(R.ms_ssim_loss, real, fake, 50.0, torch.float64)
    gen = torch.Generator().manual_seed(7)
    h = 1e-6                                                 # unit-variance directions: the difference is ~1e-7 of a loss known to ~1e-16
    for _ in range(8):
        d = torch.randn(shape, generator=gen, dtype=torch.float64)
        up = R.ms_ssim_loss(real, fake.double() + h * d, 50.0)
        dn = R.ms_ssim_loss(real, fake.double() - h * d, 50.0)
        num, ana = float(up - dn) / (2 * h), float((g * d).sum())
        assert abs(num - ana) <= 1e-6 * abs(ana), (num, ana)


def test_identical_and_anticorrelated_images():
    shape = (1, 3, 161, 161)
    real, _ = R.pair(shape, "identical")
    for dt in (torch.float64, torch.float32):
        assert float(R.ms_ssim_loss(real, real, 50.0, dt)) == 0.0
    real, fake = R.pair(shape, "anticorrelated")
    v, g = R.value_and_grad(R.ms_ssim_loss, real, fake, 50.0, torch.float64)
    assert float(v) == 50.0 and float(g.abs().max()) == 0.0 and not torch.isnan(g).any()
    assert float(R.factors(real, fake).min()) < 0                    # a non-positive factor: relu selects, no NaN from 0^(w - 1)


def test_l1_restatement():
    a = torch.tensor([[0.5, -0.25, 0.0, 1.0]])
    b = torch.tensor([[0.25, -0.25, 0.5, 2.0]])
    v, g = R.value_and_grad(R.l1_loss, b, a, 8.0, torch.float64)         # d / d a
    assert float(v) == 8.0 * (0.25 + 0.0 + 0.5 + 1.0) / 4
    assert g.tolist() == [[2.0, 0.0, -2.0, -2.0]]


def test_window_of_the_loss_is_the_packages():
    src = open(os.path.join(ROOT, "dc_vic_amd", "csrc", "msssim_loss.hip")).read()
    body = re.search(r"kWindow\s*=\s*\{\{([^}]*)\}\}", src).group(1)
    lits = [float.fromhex(t.strip().rstrip("f")) for t in body.split(",")]
    assert lits == [float(v) for v in ssim_window()]


# ---------------------------------------------------------------------------------------------------- the C ABI
def workspace_bytes(N, Cc, H, W):
    """dcvic_msssim_loss_workspace_bytes restated: the validation metric's sections (squared-error partials, 2 fp64 per 64 x 16 stats tile
    and plane at each scale, the pooled pairs of scales 1-4), then 5 fp32 seeds and 1 fp64 value per plane and the fp32 gradient planes
    of scales 1-4, each section rounded up to 256 bytes."""
    al = lambda b: (b + 255) & ~255
    cdiv = lambda a, b: -(-a // b)
    planes, sz = N * Cc, scale_sizes(H, W)
    b = al(planes * cdiv(sz[1][1], 64) * cdiv(sz[1][0], 4) * 8)
    for h, w in sz:
        b = al(b + planes * cdiv(w - 10, 64) * cdiv(h - 10, 16) * 2 * 8)
    for h, w in sz[1:]:
        b = al(b + 2 * planes * h * w * 4)
    b = al(b + planes * 5 * 4)
    b = al(b + planes * 8)
    for h, w in sz[1:]:
        b = al(b + planes * h * w * 4)
    return b


def test_workspace_formula():
    L = _lib.lib()
    for shape in ((1, 3, 161, 161), (2, 3, 163, 201), (1, 3, 162, 331), (3, 3, 256, 256), (8, 3, 256, 256), (1, 1, 1000, 777)):
        assert L.dcvic_msssim_loss_workspace_bytes(*shape) == workspace_bytes(*shape), shape
    for shape in ((0, 3, 256, 256), (1, 0, 256, 256), (1, 3, 160, 256), (1, 3, 256, 160), (21846, 3, 161, 161)):
        assert L.dcvic_msssim_loss_workspace_bytes(*shape) == 0, shape
    assert L.dcvic_abs_err_workspace_bytes(3, 2048) == 3 * 8 and L.dcvic_abs_err_workspace_bytes(3, 2049) == 6 * 8
    assert L.dcvic_abs_err_workspace_bytes(2, 1 << 30) == 2 * 64 * 8 and L.dcvic_abs_err_workspace_bytes(0, 5) == 0


def test_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_msssim_loss.h"))
    I, Q, D_, P = C.c_int, C.c_longlong, C.c_double, C.c_void_p
    assert protos == {"dcvic_msssim_loss_workspace_bytes": (Q, [I, I, I, I]),
                      "dcvic_msssim_loss_f32": (I, [P, P, I, I, I, I, D_, P, P, P, P, Q, P]),
                      "dcvic_abs_err_workspace_bytes": (Q, [I, Q]),
                      "dcvic_abs_err_f32": (I, [P, P, Q, I, D_, P, P, P, Q, P])}
    assert test_cabi.signature_mismatches(_lib.MSSSIM_LOSS_SIGNATURES, protos) == []
    others, tables = set(), set()
    for h in ("dcvic.h", "dcvic_loss.h", "dcvic_rate.h", "dcvic_train.h", "dcvic_vq.h", "dcvic_sample_loss.h", "dcvic_gumbel.h"):
        others |= set(loss_header_prototypes(os.path.join(ROOT, "include", h)))
    for t in (_lib.SIGNATURES, _lib.LOSS_SIGNATURES, _lib.RATE_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.VQ_SIGNATURES, _lib.SAMPLE_LOSS_SIGNATURES,
              _lib.GUMBEL_SIGNATURES):
        tables |= set(t)
    assert not set(protos) & others and not set(_lib.MSSSIM_LOSS_SIGNATURES) & tables
    L = _lib.lib()
    for name in protos:                                      # lib() typed them
        assert getattr(L, name).argtypes == protos[name][1]


FAKE_PTR = 256                                               # non-null, never dereferenced: every refusal precedes the first launch


def msssim_call(real=FAKE_PTR, fake=FAKE_PTR, N=1, Cc=3, H=161, W=161, scale=1.0, loss=FAKE_PTR, ws=FAKE_PTR, ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = max(int(L.dcvic_msssim_loss_workspace_bytes(N, Cc, H, W)), 1)
    return L.dcvic_msssim_loss_f32(real, fake, N, Cc, H, W, scale, loss, None, None, ws, ws_bytes, None)


def abs_call(a=FAKE_PTR, b=FAKE_PTR, M=48, N=2, scale=1.0, loss=FAKE_PTR, ws=FAKE_PTR, ws_bytes=1 << 20):
    return _lib.lib().dcvic_abs_err_f32(a, b, M, N, scale, loss, None, ws, ws_bytes, None)


REFUSALS = [
    (lambda: msssim_call(real=None), "msssim_loss: null pointer"), (lambda: msssim_call(fake=None), "msssim_loss: null pointer"),
    (lambda: msssim_call(loss=None), "msssim_loss: null pointer"), (lambda: msssim_call(ws=None), "msssim_loss: null pointer"),
    (lambda: msssim_call(N=0), "msssim_loss: empty tensor"), (lambda: msssim_call(Cc=0), "msssim_loss: empty tensor"),
    (lambda: msssim_call(H=160), "msssim_loss: MS-SSIM needs min(H, W) > 160, got 160 x 161"),
    (lambda: msssim_call(W=64, H=64), "msssim_loss: MS-SSIM needs min(H, W) > 160, got 64 x 64"),
    (lambda: msssim_call(scale=float("inf")), "msssim_loss: scale inf is not finite"),
    (lambda: msssim_call(scale=float("nan")), "msssim_loss: scale"),
    (lambda: msssim_call(ws_bytes=workspace_bytes(1, 3, 161, 161) - 1), f"msssim_loss: workspace of {workspace_bytes(1, 3, 161, 161) - 1} bytes, need"),
    (lambda: msssim_call(N=21846), "msssim_loss: 65538 planes, at most 65535"),
    (lambda: abs_call(a=None), "abs_err: null pointer"), (lambda: abs_call(b=None), "abs_err: null pointer"),
    (lambda: abs_call(loss=None), "abs_err: null pointer"), (lambda: abs_call(ws=None), "abs_err: null pointer"),
    (lambda: abs_call(N=0), "abs_err: empty tensor"), (lambda: abs_call(M=0), "abs_err: empty tensor"),
    (lambda: abs_call(scale=float("-inf")), "abs_err: scale -inf is not finite"),
    (lambda: abs_call(ws_bytes=15), "abs_err: workspace of 15 bytes, need 16"),
]


def check_refusals():
    """Every refusal returns DCVIC_EINVAL with the entry point's name in front of the message (shared with the GPU test file)."""
    L = _lib.lib()
    for call, words in REFUSALS:
        assert call() == -1, words
        assert L.dcvic_last_error().decode().startswith(words), (L.dcvic_last_error(), words)


def test_argument_refusals_without_gpu():
    check_refusals()


# ---------------------------------------------------------------------------------------------------- the YAML rules
@pytest.fixture(scope="module")
def cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dcvic_train_cli_msssim", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def sections():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        return json.load(f)


def with_distortion(opt, entry, trainer_type=None):
    opt = copy.deepcopy(opt)
    opt["loss"]["distortion_loss"] = entry
    if trainer_type is not None:
        opt.setdefault("trainer", {})["type"] = trainer_type
    return opt


@pytest.mark.parametrize("dtype", ["L1Loss", "MSSSIMLoss"])
def test_stage_1_2_yaml_with_the_two_types_is_read(cli, sections, dtype):
    from dc_vic_amd.train.losses import read_distortion_loss, read_loss_section
    base = sections["exp1_stage1_2.yaml"]
    opt = with_distortion(base, dict(type=dtype, loss_weight=7.5))
    assert cli.choose_trainer(opt) == cli.choose_trainer(base) and cli.choose_trainer(opt)[0] == "rd"
    assert read_distortion_loss(opt) == dict(type=dtype, loss_weight=7.5)
    r, r0 = read_loss_section(opt), read_loss_section(base)
    assert r["distortion_type"] == dtype and r["weights"]["distortion"] == 7.5 and r["line"].startswith(f"distortion {dtype} on [-1, 1]")
    for k in ("code_ce", "code_distortion_reduction", "per_sample", "rate"):
        assert r[k] == r0[k], k
    # the shipped config is read as before
    assert r0["distortion_type"] == "MSELoss" and read_distortion_loss(base)["type"] == "MSELoss" and r0["line"].startswith("distortion MSELoss(")
    assert read_distortion_loss({}) == dict(type="MSELoss", loss_weight=None)


@pytest.mark.parametrize("dtype", ["L1Loss", "MSSSIMLoss"])
def test_extra_keyword_and_unknown_type_are_refused_with_key_and_value(sections, dtype):
    from dc_vic_amd.train.losses import read_distortion_loss, read_loss_section
    base = sections["exp1_stage1_2.yaml"]
    for fn in (read_loss_section, read_distortion_loss):
        with pytest.raises(SystemExit) as e:
            fn(with_distortion(base, dict(type=dtype, loss_weight=1.0, mse_scale="0_1")))
        assert "loss.distortion_loss.mse_scale" in str(e.value) and "0_1" in str(e.value) and dtype in str(e.value)
        with pytest.raises(SystemExit) as e:
            fn(with_distortion(base, dict(type=dtype, loss_weight=1.0, data_range=255)))
        assert "loss.distortion_loss.data_range" in str(e.value) and "255" in str(e.value)
    with pytest.raises(SystemExit) as e:
        read_distortion_loss(with_distortion(base, dict(type="CharbonnierLoss", loss_weight=1.0)))
    assert "loss.distortion_loss.type" in str(e.value) and "CharbonnierLoss" in str(e.value)
    with pytest.raises(SystemExit) as e:
        read_loss_section(with_distortion(base, dict(type=dtype, loss_weight="heavy")))
    assert "loss.distortion_loss.loss_weight" in str(e.value) and "heavy" in str(e.value)


@pytest.mark.parametrize("dtype", ["L1Loss", "MSSSIMLoss"])
@pytest.mark.parametrize("cfg,trainer_type", [("exp1_stage1_3.yaml", None), ("exp1_stage3.yaml", None), ("exp1_stage1_3.yaml", GAN), ("exp1_stage1_2.yaml", "")])
def test_gan_stage_and_untyped_configs_still_refuse_the_two_types(sections, dtype, cfg, trainer_type):
    """The boundary of this feature: under a GAN-stage trainer type, or with none, the message is the one from before."""
    from dc_vic_amd.train.losses import read_loss_section
    opt = with_distortion(sections[cfg], dict(type=dtype, loss_weight=1.0), trainer_type)
    if trainer_type == "":
        del opt["trainer"]["type"]
        opt["loss"].pop("rate_loss", None)                   # with no trainer type a rate_loss entry is refused first
        for k in ("code_distortion_loss", "code_ce_loss"):
            opt["loss"][k] = dict(opt["loss"][k], reduction="mean")
    with pytest.raises(SystemExit) as e:
        read_loss_section(opt)
    assert str(e.value) == f"loss.distortion_loss.type: {dtype} is not built, expected MSELoss"


def test_trainer_keyword():
    import inspect
    from dc_vic_amd.train import rd_trainer as T
    sig = inspect.signature(T.DualBetaCondRateDistortionVqCodeTrainer.__init__)
    assert sig.parameters["distortion_type"].default == "MSELoss"
    assert T.DISTORTION_TYPES == ("MSELoss", "L1Loss", "MSSSIMLoss")
    assert T.LOG_KEYS == ("rate", "distortion", "perceptual", "code_distortion", "code_ce", "total", "qbpp", "vq_acc", "lr", "aux")
    with pytest.raises(ValueError, match="distortion_type: SSIMLoss"):
        T.DualBetaCondRateDistortionVqCodeTrainer(None, distortion_type="SSIMLoss")
