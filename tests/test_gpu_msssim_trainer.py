"""The stage 1-2 rate-distortion trainer with `distortion_type` MSSSIMLoss and L1Loss on a real MI355X: one whole step at 1 x 3 x 192 x 192
(the smallest multiple of the model stride 64 above MS-SSIM's 160) against torch autograd over the CPU restatement -- tests/rd_step_ref.py
composed with tests/msssim_loss_ref.py by tests/msssim_step_ref.py -- with the bounds and the decision caps of test_gpu_rd_trainer.py:
2e-4 for values and loss terms, 3e-3 of the tensor's max for each of the 741 parameter gradients, analysis_train_ref.tie_report's caps for
the rounded symbols, the estimator's argmax and the ReLU signs.  The image is msssim_step_ref.step_image's: every MS-SSIM factor of
its reconstruction is asserted (from the restatement) to be at least 1e-3 away from 0.  Then: `distortion_type="MSELoss"` gives the bits
of a trainer built without the keyword, and a 64 x 64 batch under MSSSIMLoss raises, naming the size.

Set DCVIC_RD_ERRLOG=<file> to have the worst errors appended there."""
import functools

import pytest
import torch

import analysis_train_ref as AR
import msssim_loss_ref as MR
import msssim_step_ref as MS
import rd_step_ref as RS
from test_gpu_rd_trainer import (BETA_RATE, BETA_VQ, GRAD_TOL, VAL_TOL, _log, build_model, build_trainer, cpu_state, data_dict, forward_backward, inputs,
                                 relerr, section)

pytestmark = pytest.mark.gpu
SHAPE, SEED = (1, 3, 192, 192), 73


@functools.lru_cache(maxsize=None)
def model():
    return build_model()


@functools.lru_cache(maxsize=None)
def step_inputs():
    b1, b2 = torch.tensor(BETA_RATE)[:1], torch.tensor(BETA_VQ)[:1]
    x = MS.step_image(cpu_state(), SHAPE, b1, b2, section(), SEED)
    return MS.inputs_for(cpu_state(), x, SEED)


@pytest.mark.parametrize("kind", ["MSSSIMLoss", "L1Loss"])
def test_step_vs_cpu_restatement(kind):
    m = model()
    tr = build_trainer(m, distortion_type=kind)
    I = step_inputs()
    dd = data_dict(I)
    relu_outputs = []
    L, o = forward_backward(tr, dd, relu_outputs)
    relu = RS.ReluDecisions(relu_outputs)
    force = dict(y=o["symbols"]["y"].cpu(), z=o["symbols"]["z"].cpu(), out_idx=o["out_vq_indices"].cpu(), relu=relu)
    lsd = {k: v.detach().cpu().clone() for k, v in tr.lpips.state_dict().items()}
    R, vals, grads, dec = MS.step(kind, cpu_state(), I, torch.tensor(BETA_RATE)[:1], torch.tensor(BETA_VQ)[:1], section(), lsd, force)
    factors = MR.factors(I["x"], vals["fake"].float())
    assert float(factors.min()) >= 1e-3, factors
    assert max(vals["clamped"]) < 1e-3, vals["clamped"]
    assert not relu.unmatched and len(relu.own) >= 140, (relu.unmatched, len(relu.own))
    n_relu, worst_relu, cap_relu = AR.tie_report(*relu.report())
    assert n_relu <= cap_relu and worst_relu < 1e-4, (n_relu, cap_relu, worst_relu)
    for k in "yz":
        n, worst, cap = AR.tie_report(dec[k][0], force[k], dec[k][1])
        assert n <= cap and worst < 1e-4, f"{k}: {n} differing symbols (cap {cap}), largest distance from a tie {worst:.3e}"
    differ = int((dec["out_idx"] != force["out_idx"]).sum())
    assert differ <= max(1, int(1e-5 * force["out_idx"].numel())), f"{differ} argmax decisions differ"
    worst = {}
    assert sorted(L) == sorted(R) == ["code_ce", "code_distortion", "distortion", "perceptual", "rate"]
    for k in R:
        worst[f"loss {k}"] = relerr(L[k].reshape(()), R[k])
    worst["y_hat"] = relerr(o["quantized_code"]["y"].data, vals["y_hat"])
    worst["fake"] = relerr(o["fake"].data, vals["fake"])
    for k, v in worst.items():
        assert v <= VAL_TOL, (k, v)
    own = dict(m.named_parameters())
    checked, w_grad, w_name = 0, 0.0, ""
    for k, g in grads.items():
        if g is None or k.endswith(".quantiles"):
            continue
        e = relerr(tr.group.grad_of(own[k]), g)
        assert e <= GRAD_TOL, f"grad {k}: {e:.3e}"
        checked += 1
        if e > w_grad:
            w_grad, w_name = e, k
    assert checked == 741, checked
    _log(f"[rd step {kind} 1x192x192] " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"; distortion {float(R['distortion']):.4f} of total "
         f"{float(vals['total']):.4f}; smallest MS-SSIM factor {float(factors.min()):.3f}; {checked} parameter gradients, worst {w_grad:.3e} ({w_name}); "
         f"{n_relu} ReLU signs differ (cap {cap_relu})")


def test_mse_keyword_keeps_the_bits_and_small_images_are_refused():
    m = model()
    dd = data_dict(inputs("2x64x64"))
    out = []
    for kw in ({}, dict(distortion_type="MSELoss")):
        tr = build_trainer(m, **kw)
        L, o = forward_backward(tr, dd)
        out.append(({k: v.clone() for k, v in L.items()}, tr.group.grad.clone()))
    assert all(torch.equal(out[0][0][k], out[1][0][k]) for k in out[0][0]) and torch.equal(out[0][1], out[1][1])
    tr = build_trainer(m, distortion_type="MSSSIMLoss")
    with pytest.raises(ValueError, match="64 x 64"):
        forward_backward(tr, dd)
    with pytest.raises(ValueError, match="distortion_type"):
        build_trainer(m, distortion_type="SSIMLoss")
