"""tests/rd_step_ref.py's stage 1-2 step with the image distortion replaced by MSSSIMLoss or L1Loss of tests/msssim_loss_ref.py (no test
in here; used by test_gpu_msssim_trainer.py).

rd_step_ref.step writes the distortion as  loss_weight * mse_factor(entry) * F.mse_loss(x, fake)  -- the one F.mse_loss call of the step
with the default reduction.  While `distortion(kind)` is active that call returns the restated distortion (without its weight) and
mse_factor is 1, so the rest of the step -- the analysis side in fp64, the synthesis side, the forced decisions, the other four
terms -- is rd_step_ref's, unchanged; the calls with an explicit `reduction` (the code distortion) pass through.

`step_image` gives the test its image.  The synthetic decoder's output barely depends on its input, so half of the reconstruction of a
smooth image, clamped to [-1, 1], is an image whose own reconstruction has every MS-SSIM factor far from 0 (asserted by the test from
the restatement: the sign of a factor is a decision of the relu, and a plane with a non-positive factor has no gradient at all)."""
import contextlib

import torch
import torch.nn.functional as F

import analysis_train_ref as AR
import msssim_loss_ref as MR
import rd_step_ref as RS
from oracle import dcvic_oracle as orc


@contextlib.contextmanager
def distortion(kind):
    real_mse, real_factor = F.mse_loss, RS.mse_factor

    def mse_loss(a, b, *args, **kw):
        if args or kw:
            return real_mse(a, b, *args, **kw)
        if kind == "MSSSIMLoss":                             # rd_step_ref passes (x, fake): real first, as MSSSIMLoss.forward takes them
            return 1 - MR.ms_ssim_planes(a, b, b.dtype).mean()
        return F.l1_loss(a, b)
    F.mse_loss, RS.mse_factor = mse_loss, (lambda e: 1.0)
    try:
        yield
    finally:
        F.mse_loss, RS.mse_factor = real_mse, real_factor


def step(kind, *args, **kw):
    """rd_step_ref.step(*args) with distortion_loss.type `kind` (MSSSIMLoss or L1Loss)."""
    assert kind in ("MSSSIMLoss", "L1Loss"), kind
    with distortion(kind):
        return RS.step(*args, **kw)


def inputs_for(sd, x, seed):
    """analysis_train_ref.analysis_inputs for a given image (its noises are seeded, its VQ side is the image's)."""
    I = AR.analysis_inputs(sd, tuple(x.shape), seed)
    with torch.no_grad():
        zq, idx = orc.vq_encode(sd, x)
        feat = orc.onehot_feat(sd, zq, idx)
    return dict(I, x=x, idx=idx, feat=feat)


def step_image(sd, shape, b1, b2, opt, seed):
    """clamp(0.5 * reconstruction of a smooth image): see the head of the file."""
    x0 = MR.smooth(shape, seed)
    _, vals, _, _ = RS.step(sd, inputs_for(sd, x0, seed), b1, b2, opt, None, dict(y=None, z=None))
    return (0.5 * vals["fake"].float()).clamp(-1, 1).contiguous()
