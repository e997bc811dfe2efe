"""The normalised GAN discriminators, host side (no GPU): tests/golden/disc_norm.npz (the reference's own BatchNorm / ActNorm PatchGANs
and OASIS U-Net in train mode, tools/gen_disc_norm_golden.py) against the plain-torch restatement tests/disc_norm_ref.py, the product
classes' state-dict keys, the builder's reading of the `discriminator` section with every refusal, choose_gan_trainer with the U-Net,
the tenth public header include/dcvic_bn.h against _lib.BN_SIGNATURES with the entry points' argument refusals, the loop arithmetic
that says which shape reaches which kernel path, and the `norm_type: none` initialisation draws."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import disc_norm_ref as R
import test_cabi
from dc_vic_amd import _lib
from test_focal_host import loss_header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("patchgan_bn", "patchgan_an", "unet_bn")
PATCHGAN, UNET = "DualBetaCondTamingNLayerDiscriminator", "OasisDualBetaCondTamingNLayerDiscriminator"
FLOOR = 2e-5                    # the issue's floor on every fixture comparison of this file
BUFFER_LEAVES = ("running_mean", "running_var", "num_batches_tracked", "initialized")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "disc_norm.npz"))


def case_spec(case):
    """(type, kwargs, manifest, the synthetic state) of one fixture case."""
    from dc_vic_amd.synth import synth_norm_discriminator_state
    G, p = fixture(), case + "."
    man = {k: tuple(v) for k, v in json.loads(str(G[p + "manifest"])).items()}
    return str(G[p + "type"]), json.loads(str(G[p + "kwargs"])), man, synth_norm_discriminator_state(man, int(G[p + "seed"]))


def grad_keys(case):
    p = case + ".grad/"
    return [k[len(p):] for k in fixture().files if k.startswith(p)]


def _scaled_err(a, b):
    """max |a - b| over max |b| (1 for an all-zero b): the error of a gradient against its tensor's own maximum."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


@functools.lru_cache(maxsize=None)
def restatement(case, dtype):
    """The restatement's two train-mode calls and the gradients of <cot, logits1>, in `dtype` on the CPU: dict of fp64 tensors under the
    fixture's names (logits1, logits2, grad_x, grad/<key>, buf1/<key>, buf2/<key>).  Computed once per (case, dtype) and shared."""
    G, p = fixture(), case + "."
    d_type, kw, _, state = case_spec(case)
    D = R.build(d_type, kw, state, dtype)
    x = torch.from_numpy(G["x"]).to(dtype)
    b1, b2 = torch.from_numpy(G["beta_1"]), torch.from_numpy(G["beta_2"])
    xg = x.clone().requires_grad_(True)
    l1 = D(xg, b1, b2)
    (l1 * torch.from_numpy(G[p + "cot"]).to(dtype)).sum().backward()
    out = {"logits1": l1.detach().double(), "grad_x": xg.grad.double()}
    params = dict(D.named_parameters())
    for k in grad_keys(case):
        out["grad/" + k] = params[k].grad.double()
    out.update({"buf1/" + k: v.double() for k, v in R.norm_buffers(D).items()})
    with torch.no_grad():
        out["logits2"] = D(x, b1, b2).double()
    out.update({"buf2/" + k: v.double() for k, v in R.norm_buffers(D).items()})
    return out


def _is_gradient(name):
    return name.startswith("grad")


@functools.lru_cache(maxsize=None)
def fp32_spread(case):
    """{name: the restatement's fp32-against-fp64 difference}: absolute for logits and buffers, over the fp64 tensor's maximum for
    gradients.  The GPU tests widen a bound to 4 x this where it exceeds the bound's floor."""
    a, b = restatement(case, torch.float32), restatement(case, torch.float64)
    return {k: (_scaled_err(a[k], b[k]) if _is_gradient(k) else float((a[k] - b[k]).abs().max())) for k in b}


# ---------------------------------------------------------------------------------------------------- the fixture and the restatement
@pytest.mark.parametrize("case", CASES)
def test_fixture_is_the_restatement_in_fp32(case):
    """Every stored quantity against disc_norm_ref in fp32 on the same inputs, within max(2e-5, 4 x the restatement's own
    fp32-against-fp64 spread); integer buffers (num_batches_tracked, initialized) exactly.  Measured here: the fp32 restatement gives
    the fixture's bits (error 0); the spread is up to 7e-6 on the logits and, for patchgan_bn, 7e-3 of max on d/d input."""
    G, p = fixture(), case + "."
    got, spread = restatement(case, torch.float32), fp32_spread(case)
    assert set(got) == {k[len(p):] for k in G.files if k.startswith(p)} - {"kwargs", "type", "seed", "manifest", "cot"}
    for name, val in got.items():
        want = torch.from_numpy(np.asarray(G[p + name]))
        if name.rsplit(".", 1)[-1] in ("num_batches_tracked", "initialized"):
            assert torch.equal(val.long(), want.long()), name
            continue
        err = _scaled_err(val, want) if _is_gradient(name) else float((val - want.double()).abs().max())
        bound = max(FLOOR, 4 * spread[name])
        print(f"[disc_norm fixture] {case} {name}: err {err:.3g} bound {bound:.3g} (fp32 spread {spread[name]:.3g})")
        assert err <= bound, (case, name, err, bound)
    # the second call shows the first one's updates: the counter moved twice, ActNorm's flag is set after the first call
    for k in (k for k in got if k.startswith("buf2/") and k.endswith("num_batches_tracked")):
        assert int(got[k]) == 5 and int(got[k.replace("buf2/", "buf1/")]) == 4
    for k in (k for k in got if k.endswith("initialized")):
        assert int(got[k]) == 1


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_and_shapes_match_the_reference(case):
    import dc_vic_amd.train  # noqa: F401  (registers the classes)
    from dc_vic_amd.registry import DISCRIMINATOR_REGISTRY
    d_type, kw, man, state = case_spec(case)
    D = DISCRIMINATOR_REGISTRY.get(d_type)(**kw)
    sd = D.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == man
    assert list(sd) == list(R.CLASSES[d_type](**kw).state_dict())                       # the same order too
    for k, v in sd.items():
        leaf = k.rsplit(".", 1)[-1]
        assert v.dtype == (torch.int64 if leaf == "num_batches_tracked" else torch.uint8 if leaf == "initialized" else torch.float32), k
    D.load_state_dict(state, strict=True)
    for k, v in state.items():
        if k.endswith("running_var"):
            assert float(v.min()) > 0
    # the norm layers' weights are parameters: ParamGroup([D]) picks them up
    names = {n for n, _ in D.named_parameters()}
    assert set(R.norm_param_names(R.CLASSES[d_type](**kw))) <= names
    if case == "patchgan_bn":
        assert {"main.3.running_mean", "main.6.num_batches_tracked", "main.9.weight"} <= set(sd) and "main.2.bias" not in sd and "main.8.bias" not in sd
        assert "main.0.bias" in sd and "main.11.bias" in sd
    if case == "patchgan_an":
        assert {"main.3.loc", "main.3.scale", "main.3.initialized", "main.2.bias"} <= set(sd) and tuple(sd["main.3.loc"].shape) == (1, 128, 1, 1)
    if case == "unet_bn":
        assert {"body.1.1.running_var", "bottleneck.1.weight", "up_blocks.0.1.bias", "up_blocks.0.2.running_mean", "head.2.weight",
                "beta_emb.mlp.0.weight"} <= set(sd) and "bottleneck.0.bias" not in sd and "body.1.0.bias" not in sd


def test_weights_init_restated():
    """taming's weights_init: conv weights N(0, 0.02), BatchNorm weight N(1, 0.02) and bias 0; `weight_init: false` leaves the layers' own."""
    from dc_vic_amd.train import nets
    torch.manual_seed(3)
    D = nets.DualBetaCondTamingNLayerDiscriminator(norm_type="batchnorm", max_beta_1=3.0, max_beta_2=3.5)
    w = D.main[5].weight
    assert abs(float(w.std()) - 0.02) < 1e-3 and abs(float(w.mean())) < 1e-3
    g = D.main[6].weight
    assert abs(float(g.mean()) - 1.0) < 5e-3 and 0.01 < float(g.std()) < 0.03 and float(D.main[6].bias.abs().max()) == 0.0
    assert D.main[5].bias is None and D.main[0].bias is not None and D.main[11].bias is not None
    U = nets.OasisDualBetaCondTamingNLayerDiscriminator(input_nc=6, cond_ch=3, n_layers=3, norm_type="batchnorm", max_beta_1=3.0, max_beta_2=3.5)
    assert abs(float(U.head[0].weight.std()) - 0.02) < 2e-3 and abs(float(U.up_blocks[0][2].weight.mean()) - 1.0) < 1e-2
    assert U.up_blocks[0][1].bias is not None and U.bottleneck[0].bias is None and U.logit_stride == 4


def test_norm_none_initialisation_draws_are_unchanged():
    """`norm_type: none` consumes the random draws it consumed before the norm layers existed: the SHA-256 of the seeded state dict
    (keys and fp32 bytes in order), recorded on the commit before this one."""
    from dc_vic_amd.train import nets
    torch.manual_seed(1234)
    D = nets.DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, L=10, cond_ch=8)
    h = hashlib.sha256()
    for k, v in D.state_dict().items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    after = float(torch.rand(1))                        # and it leaves the generator where it left it
    assert (h.hexdigest(), after) == NORM_NONE_HASH


NORM_NONE_HASH = ("f5354a5dd6c5f6042d2ff160abe3c55f8b88c9691bda2351325b152b9ad2c615", 0.714116632938385)


# ---------------------------------------------------------------------------------------------------- the builder
@pytest.fixture(scope="module")
def sections():
    with open(os.path.join(ROOT, "tests", "golden", "reference_discriminator_sections.json")) as f:
        return json.load(f)


def test_read_discriminator_on_the_shipped_sections(sections):
    """Every reference YAML with a `discriminator` section, and a config without one: the type, the kwargs unchanged, norm none."""
    from dc_vic_amd.train.build import DEFAULT_DISCRIMINATOR, read_discriminator
    assert sorted(sections) == ["dc_vic_oasis.yaml", "dc_vic_patchgan.yaml", "exp1_stage1_3.yaml"]
    for name, sec in list(sections.items()) + [("no section", None)]:
        r = read_discriminator({"discriminator": sec} if sec is not None else {})
        want = dict(sec if sec is not None else DEFAULT_DISCRIMINATOR)
        assert r["type"] == want.pop("type") == PATCHGAN and r["kwargs"] == want, name
        assert r["norm_type"] == "none" and r["norm_type_given"] and r["norm_kwargs"] == {}
        assert r["line"] == f"discriminator: {PATCHGAN}, n_layers 3, norm none", name
    r = read_discriminator({"discriminator": dict(sections["exp1_stage1_3.yaml"], norm_type="batchnorm", norm_kwargs={"eps": 1e-3, "momentum": 0.2})})
    assert r["norm_type"] == "batchnorm" and r["line"].endswith("norm batchnorm (eps 0.001, momentum 0.2)")
    r = read_discriminator({"discriminator": dict(sections["exp1_stage1_3.yaml"], use_actnorm=True)})
    assert r["norm_type"] == "actnorm" and r["line"].endswith("norm actnorm")              # use_actnorm wins over norm_type: none
    sec = {k: v for k, v in sections["exp1_stage1_3.yaml"].items() if k not in ("norm_type", "use_actnorm")}
    r = read_discriminator({"discriminator": sec})
    assert r["norm_type"] == "none" and not r["norm_type_given"] and "reference's class default is batchnorm" in r["line"] and "none is in effect" in r["line"]
    r = read_discriminator({"discriminator": dict(type=UNET, input_nc=6, cond_ch=3, n_layers=4, num_upsample=1, out_nc=257, norm_type="batchnorm")})
    assert r["type"] == UNET and r["line"] == f"discriminator: {UNET}, n_layers 4, norm batchnorm (eps 1e-05, momentum 0.1), num_upsample 1"


_UNET_OK = dict(type=UNET, input_nc=6, cond_ch=3, n_layers=4, num_upsample=1, out_nc=257, norm_type="batchnorm")
REFUSALS = [
    (dict(type="TamingNLayerDiscriminator"), ("discriminator.type", "TamingNLayerDiscriminator", "unknown")),
    (dict(norm_type="instancenorm"), ("discriminator.norm_type", "instancenorm", "not built")),
    (dict(norm_type="groupnorm"), ("discriminator.norm_type", "groupnorm", "not built")),
    (dict(norm_type="layernorm"), ("discriminator.norm_type", "layernorm", "not built")),
    (dict(norm_type="spectral"), ("discriminator.norm_type", "spectral", "unknown")),
    (dict(y_hat_cond=True), ("discriminator.y_hat_cond", "true", "not built")),
    (dict(norm_type="batchnorm", norm_kwargs={"affine": False}), ("discriminator.norm_kwargs.affine", "False", "not built")),
    (dict(norm_type="batchnorm", norm_kwargs={"track_running_stats": False}), ("discriminator.norm_kwargs.track_running_stats", "False", "not built")),
    (dict(norm_type="batchnorm", norm_kwargs={"momentum": None}), ("discriminator.norm_kwargs.momentum", "None", "not built")),
    (dict(norm_type="batchnorm", norm_kwargs={"eps": "1e-5"}), ("discriminator.norm_kwargs.eps", "'1e-5'", "not built")),
    (dict(norm_type="batchnorm", norm_kwargs={"eps": 0.0}), ("discriminator.norm_kwargs.eps", "0.0", "positive")),
    (dict(norm_type="batchnorm", norm_kwargs={"momentum": 1.5}), ("discriminator.norm_kwargs.momentum", "1.5", "[0, 1]")),
    (dict(norm_type="actnorm", norm_kwargs={"logdet": True}), ("discriminator.norm_kwargs.logdet", "True", "not built")),
    (dict(norm_type="none", norm_kwargs={"eps": 1e-5}), ("discriminator.norm_kwargs.eps", "1e-05", "norm_type none")),
    (dict(n_layers=0), ("discriminator.n_layers", "0", "at least 1")),
    (dict(_UNET_OK, cond_ch=8, input_nc=11), ("discriminator.cond_ch", "8", "expand_as", "not built")),
    (dict(_UNET_OK, input_nc=3), ("discriminator.input_nc", "3", "3 + cond_ch")),
    (dict(_UNET_OK, num_upsample=4), ("discriminator.num_upsample", "4", "n_layers - 1")),
    (dict(_UNET_OK, num_upsample=0), ("discriminator.num_upsample", "0", "n_layers - 1")),
    (dict(_UNET_OK, y_hat_cond=True), ("discriminator.y_hat_cond", "not built")),
    (dict(_UNET_OK, norm_type="groupnorm"), ("discriminator.norm_type", "groupnorm", "not built")),
]


@pytest.mark.parametrize("over, words", REFUSALS, ids=[f"{i}-{w[0].split('.', 1)[1]}" for i, (_, w) in enumerate(REFUSALS)])
def test_read_discriminator_refusals(sections, over, words):
    """Each refusal ends the run (SystemExit) before any GPU work and names the key and the value; the constructors refuse the same."""
    from dc_vic_amd.registry import DISCRIMINATOR_REGISTRY
    from dc_vic_amd.train.build import read_discriminator
    sec = dict(sections["exp1_stage1_3.yaml"]) if over.get("type") != UNET else {}
    sec.update(over)
    with pytest.raises(SystemExit) as e:
        read_discriminator({"discriminator": sec})
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    if sec["type"] in DISCRIMINATOR_REGISTRY:
        kw = {k: v for k, v in sec.items() if k != "type"}
        with pytest.raises((NotImplementedError, ValueError)) as e2:
            DISCRIMINATOR_REGISTRY.get(sec["type"])(**kw)
        assert str(e2.value) in str(e.value)


def test_registry_holds_both_classes():
    import dc_vic_amd.train as T
    from dc_vic_amd.registry import DISCRIMINATOR_REGISTRY
    assert DISCRIMINATOR_REGISTRY.get(PATCHGAN) is T.DualBetaCondTamingNLayerDiscriminator
    assert DISCRIMINATOR_REGISTRY.get(UNET) is T.OasisDualBetaCondTamingNLayerDiscriminator
    assert sorted(DISCRIMINATOR_REGISTRY.keys()) == [PATCHGAN, UNET]


def test_choose_gan_trainer_with_the_unet():
    """The U-Net under OASIS needs out_nc = n_embed + 1 and 2^(n_layers - num_upsample) = 8; keep_shape does not apply to it."""
    from dc_vic_amd.train.build import OASIS_TRAINER, VANILLA_TRAINER, choose_gan_trainer
    vq = {"vq_model": {"n_embed": 256}}
    opt = lambda **d: {"subnet": vq, "discriminator": dict(_UNET_OK, **d)}
    assert choose_gan_trainer(opt())[:2] == ("oasis", OASIS_TRAINER)                    # no keep_shape key, chosen by out_nc
    assert choose_gan_trainer(opt(keep_shape=False), "oasis")[:2] == ("oasis", OASIS_TRAINER)
    assert choose_gan_trainer(opt(n_layers=5, num_upsample=2))[0] == "oasis"
    for bad in (dict(n_layers=3, num_upsample=1), dict(n_layers=4, num_upsample=2)):
        with pytest.raises(SystemExit) as e:
            choose_gan_trainer(opt(**bad))
        assert "U-Net" in str(e.value) and "n_layers" in str(e.value) and "num_upsample" in str(e.value) and "8" in str(e.value)
    with pytest.raises(SystemExit) as e:
        choose_gan_trainer(opt(out_nc=128), "oasis")
    assert "out_nc: 128" in str(e.value) and "257" in str(e.value)
    assert choose_gan_trainer(opt(out_nc=1))[:2] == ("vanilla", VANILLA_TRAINER)
    # the PatchGAN's answers are what they were
    pg = {"subnet": vq, "discriminator": {"type": PATCHGAN, "out_nc": 257, "keep_shape": False}}
    with pytest.raises(SystemExit) as e:
        choose_gan_trainer(pg)
    assert "keep_shape: false" in str(e.value)


# ---------------------------------------------------------------------------------------------------- the tenth header
def test_bn_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_bn.h"))
    P, I, Q, D = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    assert protos == {
        "dcvic_bn_workspace_bytes": (Q, [I, I, I]),
        "dcvic_bn_stats_f32": (I, [P, Q, P, P, P, Q, I, I, I, P]),
        "dcvic_bn_train_fwd_f32": (I, [P, Q, P, Q, P, P, P, P, D, D, P, P, I, P, Q, I, I, I, P]),
        "dcvic_bn_train_bwd_f32": (I, [P, Q, P, Q, P, Q, P, P, P, P, Q, P, P, I, I, P, Q, I, I, I, P]),
        "dcvic_actnorm_fwd_f32": (I, [P, Q, P, Q, P, P, I, I, I, I, P]),
        "dcvic_actnorm_bwd_f32": (I, [P, Q, P, Q, P, Q, P, P, P, Q, P, P, I, I, P, Q, I, I, I, P]),
    }
    assert test_cabi.signature_mismatches(_lib.BN_SIGNATURES, protos) == []
    others, tables = set(), set()
    for h in ("dcvic.h", "dcvic_loss.h", "dcvic_rate.h", "dcvic_train.h", "dcvic_vq.h", "dcvic_sample_loss.h", "dcvic_gumbel.h", "dcvic_msssim_loss.h",
              "dcvic_data.h"):
        others |= set(loss_header_prototypes(os.path.join(ROOT, "include", h)))
    for t in (_lib.SIGNATURES, _lib.LOSS_SIGNATURES, _lib.RATE_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.VQ_SIGNATURES, _lib.SAMPLE_LOSS_SIGNATURES,
              _lib.GUMBEL_SIGNATURES, _lib.MSSSIM_LOSS_SIGNATURES, _lib.DATA_SIGNATURES):
        tables |= set(t)
    assert not set(protos) & others and not set(_lib.BN_SIGNATURES) & tables
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the comparison catches a double declared as float, a missing parameter and a narrowed stride
    for name, sig in (("dcvic_bn_train_fwd_f32", "i:pqpqppppfdppipqiiip"), ("dcvic_bn_stats_f32", "i:pqpppqiip"), ("dcvic_actnorm_fwd_f32", "i:pipqppiiiip")):
        bad = test_cabi.signature_mismatches(dict(_lib.BN_SIGNATURES, **{name: sig}), protos)
        assert len(bad) == 1 and bad[0].startswith(name + ":"), (sig, bad)


# The loop arithmetic of csrc/bn_train.hip, restated: a plane of HW values is cut into chunks of 4096; a workgroup of 256 threads walks
# its chunk in steps of 1024 (4 values per thread); 16-byte accesses when HW and every batch stride are multiples of 4.
CHUNK, STEP = 4096, 1024


def kernel_path(N, C, H, W, bs_extra=0):
    HW = H * W
    S = -(-HW // CHUNK)
    return dict(chunks=S, steps_in_last=-(-(HW - (S - 1) * CHUNK) // STEP), vec=HW % 4 == 0 and bs_extra % 4 == 0, partials=N * S,
                final_rounds=-(-N * S // 64), ws=16 * C * N * S + (12 * C + 15) // 16 * 16)


# the shapes tests/test_gpu_bn_train.py runs, with the path each one is there for
GPU_SHAPES = {
    (2, 1, 1, 1): "M = 2, one value per plane",
    (1, 3, 1, 2): "one image, scalar path",
    (3, 5, 3, 7): "odd HW: scalar path with a tail inside a group of 4",
    (2, 64, 8, 8): "16-byte path, a quarter of a step",
    (2, 130, 31, 31): "HW = 961, C not a multiple of 64, scalar path over a whole step",
    (4, 8, 64, 64): "16-byte path, one full chunk of 4 steps",
    (1, 2, 65, 64): "HW = 4160: just above the chunk threshold, two chunks",
    (66, 2, 2, 2): "more than 64 partials per channel: the final pass's second round",
}


def test_loop_arithmetic_names_the_path_of_every_gpu_shape():
    L = _lib.lib()
    paths = {s: kernel_path(*s) for s in GPU_SHAPES}
    for s, p in paths.items():
        assert L.dcvic_bn_workspace_bytes(s[0], s[1], s[2] * s[3]) == p["ws"], s
    assert L.dcvic_bn_workspace_bytes(0, 4, 4) == 0 and L.dcvic_bn_workspace_bytes(2, 0, 4) == 0 and L.dcvic_bn_workspace_bytes(2, 4, 0) == 0
    assert [paths[s]["chunks"] for s in GPU_SHAPES] == [1, 1, 1, 1, 1, 1, 2, 1]
    assert [paths[s]["vec"] for s in GPU_SHAPES] == [False, False, False, True, False, True, True, True]
    assert paths[(4, 8, 64, 64)]["steps_in_last"] == 4 and paths[(1, 2, 65, 64)]["steps_in_last"] == 1 and paths[(2, 130, 31, 31)]["steps_in_last"] == 1
    assert kernel_path(1, 2, 64, 64)["chunks"] == 1                                        # the threshold itself stays one chunk
    assert paths[(66, 2, 2, 2)]["final_rounds"] == 2 and all(paths[s]["final_rounds"] == 1 for s in GPU_SHAPES if s != (66, 2, 2, 2))
    assert not kernel_path(2, 64, 8, 8, bs_extra=5)["vec"]                                  # a foreign batch stride: the scalar loads of the same values
    # the trainer's three tensors
    assert [kernel_path(8, c, h, h)["chunks"] for c, h in ((128, 64), (256, 32), (512, 31))] == [1, 1, 1]


# Every case breaks one rule and keeps the others valid (test_cabi._NO_GPU_PRELUDE: every GPU hidden, dummy non-null addresses).
# baseline N = 2, C = 4, HW = 16, dense strides 64, workspace of exactly dcvic_bn_workspace_bytes
_BN_ARG_CHECKS = r"""
D = C.c_double
WS = L.dcvic_bn_workspace_bytes(2, 4, 16)
assert WS == 16 * 4 * 2 + 48
def fwd(x=P, x_bs=64, y=P, y_bs=64, gamma=P, beta=P, rm=P, rv=P, mom=0.1, eps=1e-5, sm=P, sr=P, act=2, ws=P, wsb=WS, N=2, Cc=4, HW=16):
    return L.dcvic_bn_train_fwd_f32(x, LL(x_bs), y, LL(y_bs), gamma, beta, rm, rv, D(mom), D(eps), sm, sr, act, ws, LL(wsb), N, Cc, HW, None)
def bwd(x=P, x_bs=64, g=P, g_bs=64, y=P, y_bs=64, sm=P, sr=P, gamma=P, dx=P, dx_bs=64, dg=P, db=P, accum=1, act=2, ws=P, wsb=WS, N=2, Cc=4, HW=16):
    return L.dcvic_bn_train_bwd_f32(x, LL(x_bs), g, LL(g_bs), y, LL(y_bs), sm, sr, gamma, dx, LL(dx_bs), dg, db, accum, act, ws, LL(wsb), N, Cc, HW, None)
def stats(x=P, x_bs=64, mean=P, std=P, ws=P, wsb=WS, N=2, Cc=4, HW=16):
    return L.dcvic_bn_stats_f32(x, LL(x_bs), mean, std, ws, LL(wsb), N, Cc, HW, None)
def afwd(x=P, x_bs=64, y=P, y_bs=64, loc=P, scale=P, act=2, N=2, Cc=4, HW=16):
    return L.dcvic_actnorm_fwd_f32(x, LL(x_bs), y, LL(y_bs), loc, scale, act, N, Cc, HW, None)
def abwd(x=P, x_bs=64, g=P, g_bs=64, y=P, y_bs=64, loc=P, scale=P, dx=P, dx_bs=64, dl=P, ds=P, accum=1, act=2, ws=P, wsb=WS, N=2, Cc=4, HW=16):
    return L.dcvic_actnorm_bwd_f32(x, LL(x_bs), g, LL(g_bs), y, LL(y_bs), loc, scale, dx, LL(dx_bs), dl, ds, accum, act, ws, LL(wsb), N, Cc, HW, None)
for fn, name in ((fwd, "bn_train_fwd"), (bwd, "bn_train_bwd"), (stats, "bn_stats"), (afwd, "actnorm_fwd"), (abwd, "actnorm_bwd")):
    for kw in (dict(N=0), dict(Cc=0), dict(HW=0), dict(N=-1)):
        err(fn(**kw), name + ":", "empty")
    err(fn(N=65536), name + ":", "65535")
    err(fn(x=None), name + ":", "null pointer")
    err(fn(x_bs=63), name + ":", "batch stride", "x")
    if fn is not afwd:
        err(fn(N=1, HW=1), name + ":", "M = N * HW = 1", "at least 2")              # torch refuses it too
        err(fn(ws=None), name + ":", "null pointer", "workspace")
        err(fn(wsb=WS - 1), name + ":", "workspace", str(WS))
        err(fn(ws=C.c_void_p(68)), name + ":", "8-byte aligned")
    if fn is not stats:
        err(fn(act=1), name + ":", "act=1")
        err(fn(act=3), name + ":", "act=3")
for kw in (dict(y=None), dict(gamma=None), dict(beta=None), dict(sm=None), dict(sr=None), dict(rm=None), dict(rv=None)):
    err(fwd(**kw), "bn_train_fwd:", "null pointer")
for eps in (0.0, -1e-5, float("nan"), float("inf")):
    err(fwd(eps=eps), "bn_train_fwd:", "eps")
for mom in (-0.1, 1.5, float("nan")):
    err(fwd(mom=mom), "bn_train_fwd:", "momentum", "[0, 1]")
err(fwd(y_bs=10), "bn_train_fwd:", "batch stride", "y")
for kw in (dict(g=None), dict(sm=None), dict(sr=None), dict(gamma=None), dict(dx=None), dict(y=None), dict(dg=None), dict(db=None)):
    err(bwd(**kw), "bn_train_bwd:", "null pointer")
for kw in (dict(g_bs=1), dict(y_bs=1), dict(dx_bs=1)):
    err(bwd(**kw), "bn_train_bwd:", "batch stride")
for kw in (dict(mean=None), dict(std=None)):
    err(stats(**kw), "bn_stats:", "null pointer")
for kw in (dict(y=None), dict(loc=None), dict(scale=None)):
    err(afwd(**kw), "actnorm_fwd:", "null pointer")
for kw in (dict(g=None), dict(loc=None), dict(scale=None), dict(dx=None), dict(y=None), dict(dl=None), dict(ds=None)):
    err(abwd(**kw), "actnorm_bwd:", "null pointer")
err(fwd(Cc=1 << 20, HW=1 << 30, x_bs=1 << 50, y_bs=1 << 50, wsb=1 << 60), "bn_train_fwd:", "too large")
print("CHECKS_OK")
"""


def test_bn_argument_checks_without_gpu():
    """All five entry points refuse, before any launch and with their name in front: empty sizes, N > 65535, M < 2, every required null
    pointer (one of a both-or-neither pair too), short batch strides, a non-finite or non-positive eps, a momentum outside [0, 1],
    another activation, and a null, misaligned or short workspace."""
    test_cabi._run_without_gpu(_BN_ARG_CHECKS)
