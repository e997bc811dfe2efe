"""What the GAN-stage trainers and the rate-distortion trainer share, on a real MI355X: a step skipped for its loss (base_trainer.py:
235-245) leaves every parameter, moment, step count and scheduler where it was and the next step trains; nets.synthesis_forward is the
synthesis half of generator_forward, with and without a Gumbel sample.  The synthetic model, 2 x 64x64 and 1 x 64x128 (not square, so
that an H / W swap shows)."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


def disc():
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator
    torch.manual_seed(5)
    return DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5).to(DEV)


def build(kind, model):
    """-> (trainer, [(group, optimizer)], [scheduler])"""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondRateDistortionVqCodeTrainer
    if kind == "gan":
        tr = DualBetaCondGanDistortionVqCodeTrainer(model, disc(), seed=3, loss_weights={"distortion": 1e9})
        return tr, [(tr.g_group, tr.g_opt), (tr.d_group, tr.d_opt)], [tr.g_sched, tr.d_sched]
    tr = DualBetaCondRateDistortionVqCodeTrainer(model, seed=3, loss_weights={"distortion": 1e9})
    return tr, [(tr.group, tr.opt), (tr.aux_group, tr.aux_opt)], [tr.sched]


@pytest.mark.parametrize("kind", ["gan", "rd"])
def test_a_skipped_step_changes_nothing_and_the_next_one_trains(model, kind):
    """distortion x 1e9 puts the total far above 1e4 and keeps it finite (shown by the second step's own distortion value, on the same
    image and the untouched weights): optimize_parameters returns None and flat / m / v of every group, every Adam step count and every
    scheduler epoch are what they were -- the discriminator's too.  One trained step first, so that the moments are not all zero."""
    tr, groups, scheds = build(kind, model)
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(31)) * 2 - 1
    tr.w["distortion"] = 50.0
    assert tr.optimize_parameters(1, {"real_images": x}) is not None
    tr.w["distortion"] = 1e9
    before = [(g.flat.clone(), g.m.clone(), g.v.clone()) for g, _ in groups]
    counts = [o.t for _, o in groups] + [s.last_epoch for s in scheds]
    assert counts == [1] * len(counts) and all(float(m_.abs().max()) > 0 for _, m_, _ in before)
    assert tr.optimize_parameters(2, {"real_images": x}) is None
    for (g, _), (flat, m_, v_) in zip(groups, before):
        assert torch.equal(g.flat, flat) and torch.equal(g.m, m_) and torch.equal(g.v, v_)
    assert [o.t for _, o in groups] + [s.last_epoch for s in scheds] == counts
    tr.w["distortion"] = 50.0
    log = tr.optimize_parameters(3, {"real_images": x})
    assert log is not None and all(math.isfinite(v) for v in log.values()), log
    skipped_total = log["distortion"] * (1e9 / 50.0)
    print(f"[skip {kind}] the skipped step's distortion term alone: {skipped_total:.4g}")
    assert 1e4 < skipped_total < float("inf")
    assert not torch.equal(groups[0][0].flat, before[0][0])
    assert [o.t for _, o in groups] + [s.last_epoch for s in scheds] == [2] * len(counts)


def test_synthesis_forward_is_generator_forwards_synthesis_half(model):
    """On generator_forward's own y_hat (a tensor) it returns that forward's fake, logits and argmax bit for bit; with a constant noise
    tensor the sample is the argmax, so the Gumbel path's fake is the argmax path's."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import nets
    x = torch.rand((1, 3, 64, 128), generator=torch.Generator().manual_seed(32)) * 2 - 1
    b1, b2 = torch.tensor([1.51]), torch.tensor([2.25])
    tr = DualBetaCondGanDistortionVqCodeTrainer(model, disc(), seed=3, gumbel_sampling=False)
    o = tr.generator_forward(A.Ctx([tr.g_group]), x, None, b1, b2)
    assert isinstance(o["y_hat"], torch.Tensor) and tuple(o["fake"].shape) == (1, 3, 64, 128) and tuple(o["logits"].shape)[2:] == (8, 16)
    s = nets.synthesis_forward(A.Ctx([tr.g_group]), model, o["y_hat"], b1, b2)
    assert sorted(s) == ["fake", "logits", "out_vq_indices", "pred_embed"]
    for k in ("fake", "logits", "pred_embed"):
        assert torch.equal(s[k].data, o[k].data), k
    assert torch.equal(s["out_vq_indices"], o["out_vq_indices"])
    g = nets.synthesis_forward(A.Ctx([tr.g_group]), model, o["y_hat"], b1, b2, gumbel=(torch.ones_like(o["logits"].data), 1.0))
    assert torch.equal(g["fake"].data, o["fake"].data) and torch.equal(g["out_vq_indices"], o["out_vq_indices"])
