"""The unconditioned stage 1-1 model (ElicVqCatScEncoder, ElicFeatFusionDecoder, HyperpriorCharmVicModel) on a real MI355X: the two
sub-networks against the reference's own classes (tests/golden/uncond.npz), run_model against the CPU oracle on the neutralised dual
state (tests/stage11_ref.py) with tests/test_gpu_model.py's bounds and parity_util's itemised near-ties, the same model against the
dual-conditioned one carrying the neutralised state on the device, and bit stability.

Inputs are the smallest legal ones: 2 x 3 x 64 x 64 and 1 x 3 x 64 x 128 (the model's stride is 64; the second shape is not square).
Set DCVIC_STAGE11_EQUIV=<file> to have the device equivalence (equal bits, and the largest differences) written there as JSON."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import stage11_ref as S11
from parity_util import Report, run_model_parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = {"2x64x64": ((2, 3, 64, 64), 411), "1x64x128": ((1, 3, 64, 128), 412)}
REFERENCE_KEYS = {"real_images", "fake_images", "y_hat", "z_hat", "out_vq_latent", "gt_vq_latent", "out_vq_logits", "gt_vq_indices", "vq_accuracy",
                  "quantized_code", "latent_code", "likelihoods", "q_likelihoods", "y_likelihood", "z_likelihood", "bpp", "y_q_likelihood",
                  "z_q_likelihood", "qbpp"}          # hyperprior_vic_model.py:128-135 over forward's dict and get_rate_summary_dict's


def img(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@functools.lru_cache(maxsize=None)
def neutral_state():
    from dc_vic_amd.synth import full_synth_state_dict
    sd = full_synth_state_dict(1234)
    return S11.neutral_dual_state({k: v for k, v in sd.items() if not S11.is_conditioning_key(k)}, sd)


@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic_stage1_1.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    m.codec_setup()
    return m


@pytest.fixture(scope="module")
def dual():
    """The dual-conditioned model carrying the neutralised state: the same function, through the beta-FT kernels."""
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    have = set(m.state_dict())
    m.load_state_dict({k: v for k, v in neutral_state().items() if k in have}, strict=False)
    m.codec_setup()
    return m


@pytest.fixture(scope="module")
def cpu_oracle():
    from oracle.dcvic_oracle import Oracle
    return Oracle(neutral_state())


def test_sub_networks_vs_the_reference_classes(model):
    """Encoder and get_feats against the fixture, at the bounds tests/test_gpu_model.py applies to the same two stages of the dual
    model (test_stage_elic_encoder 2e-5, test_stage_elic_decoder_feats 4e-4, absolute)."""
    G = np.load(os.path.join(ROOT, "tests", "golden", "uncond.npz"))
    x = (torch.from_numpy(G["x_u8"]).float() / 127.5 - 1.0).to(DEV)
    idx = torch.from_numpy(G["vq_indices"].astype(np.int64)).to(DEV)
    lat, idx2, feat = model.vq_encode(x, idx, want_feat=True)
    assert torch.equal(idx2, idx)
    y = model.comp_encode(x, lat, idx, feat=feat)
    err = {"y": float((y.cpu() - torch.from_numpy(G["y"])).abs().max())}
    f1, fd = model.decoder.get_feats(torch.from_numpy(G["y_hat"]).to(DEV))
    assert sorted(fd) == ["block_1_2", "block_1_4", "block_1_8"]
    for k, t in (("feat_1", f1), ("block_1_8", fd["block_1_8"]), ("block_1_4", fd["block_1_4"]), ("block_1_2", fd["block_1_2"])):
        err[k] = float((t.cpu() - torch.from_numpy(G["feat_1" if k == "block_1_8" else k])).abs().max())
    print("[stage 1-1 sub-networks] max |diff| " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err.pop("y") <= 2e-5
    assert all(v <= 4e-4 for v in err.values()), err
    # the free-running VQ search finds the fixture's indices, or itemised near-ties: the encoder input above does not depend on it
    _, own = model.vq_encode(x, None)
    assert int((own != idx).sum()) <= 1


class AsDual:
    """The unconditioned model behind the dual model's call signatures, for parity_util.run_model_parity: the betas are dropped."""

    def __init__(self, m):
        self.m = m

    def __getattr__(self, k):
        return getattr(self.m, k)

    def run_model(self, x, is_train=False, beta_rate=None, beta_vq=None, **kw):
        return self.m.run_model(x, is_train=is_train, **kw)

    def comp_encode(self, x, lat, idx, enc_kwargs=None, feat=None):
        return self.m.comp_encode(x, lat, idx, feat=feat)


@pytest.mark.parametrize("case", list(SHAPES))
def test_run_model_vs_oracle_on_the_neutralised_state(model, cpu_oracle, case):
    shape, seed = SHAPES[case]
    x = img(shape, seed)
    ro = cpu_oracle.run_model(x, S11.BETA, S11.BETA)
    rep = Report(f"stage11_run_model_{case}")
    try:
        rg = run_model_parity(AsDual(model), ro, x, S11.BETA, S11.BETA, rep)
    finally:
        rep.dump()
    assert REFERENCE_KEYS <= set(rg), sorted(REFERENCE_KEYS - set(rg))
    assert not [k for k in rg if "beta" in k]
    assert torch.equal(rg["real_images"].cpu(), ro["real_images"]) and tuple(rg["fake_images"].shape) == shape
    assert rg["quantized_code"]["y"] is rg["y_hat"] and rg["likelihoods"]["z"] is rg["z_likelihood"] and rg["qbpp"] == rg["bpp"]
    assert tuple(rg["out_vq_latent"].shape) == (shape[0], 4, shape[2] // 8, shape[3] // 8)
    with pytest.raises(TypeError):
        model.run_model(x, is_train=False, beta_rate=1.0, beta_vq=1.0)


def test_validation_rows_carry_the_four_keys(model):
    rows = model.validation([img((1, 3, 64, 128), 413), img((1, 3, 64, 64), 414)], max_sample_size=100)
    assert [sorted(r) for r in rows] == [["bpp", "idx", "ms_ssim", "psnr", "vq_acc"]] * 2 and [r["idx"] for r in rows] == [1, 2]
    assert all(np.isfinite(v) for r in rows for v in r.values()) and all(r["bpp"] > 0 and 0 <= r["vq_acc"] <= 1 for r in rows)
    one = model.run_model(img((1, 3, 64, 128), 413), is_train=False)
    assert rows[0]["bpp"] == one["bpp"] and rows[0]["vq_acc"] == one["vq_accuracy"]
    assert len(model.validation([img((1, 3, 64, 64), 414)] * 3, max_sample_size=2)) == 2


@pytest.mark.parametrize("case", list(SHAPES))
def test_equivalence_with_the_neutralised_dual_model_on_the_device(model, dual, case):
    """y, the decoder features, the logits and the image of the unconditioned model against the dual model's with the neutralised
    state at beta (0, 0).  The affine epilogue with (scale 0, shift 0) is an identity and the accumulation order does not depend on
    the epilogue: the bits are equal on the MI355X (profiles/stage11_equivalence.json), and equal bits are what is asserted."""
    shape, seed = SHAPES[case]
    x = img(shape, seed).to(DEV)
    out = {}
    for tag, m, b in (("uncond", model, None), ("dual", dual, S11.BETA)):
        lat, idx, feat = m.vq_encode(x, None, want_feat=True)
        y = m.comp_encode(x, lat, idx, enc_kwargs={} if b is None else dict(beta_1=b, beta_2=b), feat=feat)
        e = m._entropy_encode_side(y, want_symbols=False)
        f1, fd = m.decoder.get_feats(e["y_hat"], beta_1=b, beta_2=b)
        fake, out_idx, logits, embed = m._decode(e["y_hat"], 1.0, b, b, want_logits=True, want_embed=True)
        out[tag] = dict(idx=idx, y=y, y_hat=e["y_hat"], feat_1=f1, **{k: v.clone() for k, v in fd.items()}, logits=logits, embed=embed, out_idx=out_idx, image=fake)
    a, d = out["uncond"], out["dual"]
    assert torch.equal(a["idx"], d["idx"]) and torch.equal(a["out_idx"], d["out_idx"])
    res = {}
    for k in ("y", "y_hat", "feat_1", "block_1_8", "block_1_4", "block_1_2", "logits", "embed", "image"):
        res[k] = dict(equal_bits=bool(torch.equal(a[k], d[k])), rel=float((a[k] - d[k]).abs().max()) / float(d[k].abs().max()))
    print(f"[stage 1-1 equivalence {case}] " + ", ".join(f"{k} {'equal bits' if v['equal_bits'] else format(v['rel'], '.3e')}" for k, v in res.items()))
    path = os.environ.get("DCVIC_STAGE11_EQUIV")
    if path:
        prev = json.load(open(path)) if os.path.exists(path) else {}
        prev[case] = res
        with open(path, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)
    for k, v in res.items():
        assert v["equal_bits"], (k, v)


def test_bit_stability(model):
    """Two calls give equal bits; image 0 of a batch of 1 and of a batch of 3 gives equal bits."""
    x3 = img((3, 3, 64, 64), 415)
    keys = ("y_hat", "z_hat", "out_vq_logits", "fake_images", "out_vq_latent", "gt_vq_indices", "bits_per_image")
    a, b = model.run_model(x3, is_train=False), model.run_model(x3, is_train=False)
    assert all(torch.equal(a[k], b[k]) for k in keys) and a["bpp"] == b["bpp"]
    one = model.run_model(x3[:1], is_train=False)
    for k in keys:
        assert torch.equal(one[k][0], a[k][0]), k
