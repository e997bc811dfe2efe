"""The unconditioned stage 1-1 networks and training step through the unchanged dual-conditioned oracle (no test in here; used by
test_stage11_host.py, test_gpu_uncond_model.py and test_gpu_stage11_trainer.py).

The unconditioned model is the dual-conditioned one with its conditioning neutralised: with every `beta_ft_list.*.scale/shift` weight
and bias 0, `decoder.init_fuse.scale.bias` -1 and the rest of `init_fuse.scale/shift` 0, each beta-FT is v * (1 + 0) + 0 = v and the
initial fuse x * (1 - 1) + 0 + x = x, exactly, in any precision and for any `mlp.*` / `shared.*`.  So oracle.dcvic_oracle's
elic_encoder / elic_decoder_feats on neutral_dual_state(...) compute ElicVqCatScEncoder / ElicFeatFusionDecoder, and
rd_step_ref.step at beta (0, 0) with `beta_policy: linear`, `beta_offset: 1` and every reduction `none` computes the stage 1-1 step:
the per-image weights are all 1, and the mean of per-image means over images of equal size is the mean."""
import copy

import torch

import rd_step_ref as RS

BETA = 0.0          # any pair inside [0, max_beta] gives the same values; (0, 0) also makes the linear policy's weights 0 + offset = 1


def is_conditioning_key(k):
    return k.split(".")[0] in ("encoder", "decoder") and k.split(".")[1] in ("beta_ft_list", "mlp", "init_fuse")


def neutral_dual_state(uncond_sd, dual_sd):
    """`dual_sd` (any dual-conditioned state dict: it supplies the conditioning keys, their shapes and the arbitrary `mlp` / `shared`
    values) with every shared tensor taken from `uncond_sd` and the conditioning neutralised."""
    out = {}
    for k, v in dual_sd.items():
        if not is_conditioning_key(k):
            if k in uncond_sd:
                out[k] = uncond_sd[k].clone()
            continue
        parts = k.split(".")
        if parts[-2] in ("scale", "shift"):
            out[k] = torch.full_like(v, -1.0) if k == "decoder.init_fuse.scale.bias" else torch.zeros_like(v)
        else:
            out[k] = v.clone()                       # mlp.*, shared.*: arbitrary
    for k, v in uncond_sd.items():
        if k not in out:
            out[k] = v.clone()
    return out


def dual_section(opt11):
    """The stage 1-1 `loss` section (mean reductions, no beta) as the dual step's: unit beta weights and every reduction none."""
    loss = copy.deepcopy({k: dict(v) for k, v in opt11["loss"].items()})
    for name in ("rate_loss", "code_distortion_loss", "code_ce_loss"):
        assert loss[name].get("reduction", "mean") == "mean", (name, loss[name])
        loss[name]["reduction"] = "none"
    return dict(trainer=dict(beta_policy="linear", beta_offset=1.0, sample_beta_batch=True), loss=loss)


def step(neutral_sd, I, opt11, lsd, force, synth_dtype=torch.float32):
    """rd_step_ref.step for the stage 1-1 step on `neutral_sd` (neutral_dual_state's): same return, the gradients restricted to the
    tensors the unconditioned model has."""
    N = I["x"].shape[0]
    b = torch.full((N,), BETA)
    R, vals, grads, dec = RS.step(neutral_sd, I, b, b, dual_section(opt11), lsd, force, synth_dtype)
    return R, vals, {k: g for k, g in grads.items() if not is_conditioning_key(k)}, dec
