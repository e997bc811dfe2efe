"""The analysis side in training mode, restated in plain torch on the CPU (no test in here; shared by test_analysis_train_host.py and
test_gpu_analysis_tape.py).

It composes the differentiable functions of oracle/dcvic_oracle.py (elic_encoder, hyper_encoder, hyper_decoder, slice_transform) with
the training-mode restatements of tests/rate_train_fp64.py (noise-quantised likelihoods, LowerBound as an autograd.Function) into the
reference's estimate_entropy(is_train=True) (hyperprior_charm_dc_vic_model.py:24-56) and its CHARM loop
(minnen20_charm_context_model.py:70-119), in the dtype it is given: fp64 is the yardstick, the same code in fp32 is the reference's own
arithmetic and gives the error the bounds start from.  torch autograd supplies every gradient.

`force_symbols` (as oracle.charm_forward's): integer symbols used INSTEAD of round(y - mu) / round(z - median), so a comparison can
continue past a rounding near-tie; the helper's own rounding and its distance from a half-integer are returned beside them."""
import contextlib
import math

import torch

import rate_train_fp64 as R
from oracle import dcvic_oracle as orc
from oracle import entropy_oracle as eo

MODULES = ("encoder", "hyperencoder", "hyperdecoder", "context_model", "entropy_model_z")


def shifted_state(sd, scale_shift=1.5):
    """The synthetic weights as the training tests use them: every scale transform's last bias raised by `scale_shift`.  The synthetic
    CHARM puts 80 % of its sigmas below the 0.11 scale bound, where LowerBound's gradient rule (not the function's slope) decides;
    trained weights do not, and the tests cap the clamped share at 0.1 %."""
    out = dict(sd)
    for i in range(orc.NUM_SLICES):
        k = f"context_model.scale_slice_transforms.{i}.model.4.bias"
        out[k] = sd[k] + scale_shift
    return out


def clamped_share(e_or_c):
    """(share of sigmas below the scale bound, share of raw likelihoods below the likelihood bound) of a charm() / estimate_entropy() result."""
    pr = e_or_c["p_raw"]
    pr = torch.cat([pr["y"].flatten(), pr["z"].flatten()]) if isinstance(pr, dict) else pr.flatten()
    return float((e_or_c["sigma"] < R.SCALE_BOUND).double().mean()), float((pr < R.LIK_BOUND).double().mean())


def trainable_names(sd):
    """The float tensors of the five analysis-side modules, in sorted order (integer CDF buffers and the bottleneck's `target` excluded)."""
    return sorted(k for k, v in sd.items() if k.split(".")[0] in MODULES and v.is_floating_point() and not k.endswith(".target")
                  and not k.endswith(".scale_table"))


def leaf_state(sd, dtype, names=None):
    """sd with the named tensors (default: trainable_names) replaced by `dtype` leaves that require a gradient."""
    names = trainable_names(sd) if names is None else names
    out = dict(sd)
    for k in names:
        out[k] = sd[k].detach().to(dtype).clone().requires_grad_(True)
    return out


@contextlib.contextmanager
def _embed_as(dtype):
    """oracle.beta_cond feeds the fp32 host-side Fourier features (constants, as in the product) to F.linear: hand them over in the
    weights' dtype while the encoder runs."""
    real = orc.fourier_embed
    orc.fourier_embed = lambda *a, **k: real(*a, **k).to(dtype)
    try:
        yield
    finally:
        orc.fourier_embed = real


def ste(v, s):
    """ste_round(v) with the symbols s: value s, gradient 1."""
    return v + (s - v).detach()


def half_margin(v):
    """| |frac(v)| - 0.5 |: the distance of v from the nearest rounding tie."""
    return ((v - torch.floor(v)) - 0.5).abs()


def charm(sd, y, hyper_out, noise, is_train, force_symbols=None, p="context_model"):
    """Minnen20CharmContextModel.forward(is_train, calc_q_likelihood=True).  -> dict(y_hat, lik [noisy when training], q_lik, symbols
    [used], own_symbols [round(y - mu) of this run], margin [distance of y - mu from a tie], p_raw, sigma)."""
    hm, hs = torch.chunk(hyper_out, 2, dim=1)
    sc = y.shape[1] // orc.NUM_SLICES
    hat, lik, qlik, syms, own, margin, praw, sigs = [], [], [], [], [], [], [], []
    for i in range(orc.NUM_SLICES):
        y_i = y[:, i * sc:(i + 1) * sc]
        support = hat[:orc.MAX_SUPPORT]
        mean_support = torch.cat([hm] + support, dim=1)
        mu = orc.slice_transform(sd, f"{p}.mean_slice_transforms.{i}", mean_support)
        sigma = orc.slice_transform(sd, f"{p}.scale_slice_transforms.{i}", torch.cat([hs] + support, dim=1))
        v = y_i - mu
        s_own = torch.round(v).detach()
        s = s_own if force_symbols is None else force_symbols[:, i * sc:(i + 1) * sc].to(y.dtype)
        with torch.no_grad():
            q = eo.gc_likelihood(s + mu, sigma, mu)
        if is_train:
            l, pr = R.gaussian_likelihood(y_i, mu, sigma, noise[:, i * sc:(i + 1) * sc])
            yq = ste(v, s) + mu                           # ste_round(y - mean) + mean: gradient 1 to y, 0 to the mean
        else:
            l, pr = q, q
            yq = s + mu
        lrp = 0.5 * torch.tanh(orc.slice_transform(sd, f"{p}.lrp_slice_transforms.{i}", torch.cat([mean_support, yq], dim=1)))
        hat.append(yq + lrp)
        lik.append(l); qlik.append(q); syms.append(s.detach()); own.append(s_own); margin.append(half_margin(v.detach())); praw.append(pr.detach())
        sigs.append(sigma.detach())
    cat = lambda l: torch.cat(l, dim=1)
    return dict(y_hat=cat(hat), lik=cat(lik), q_lik=cat(qlik), symbols=cat(syms), own_symbols=cat(own), margin=cat(margin), p_raw=cat(praw),
                sigma=cat(sigs))


def eb_params_of(sd, prefix="entropy_model_z"):
    return {k: sd[f"{prefix}.{k}"] for k in R.EB_NAMES + ("quantiles",)}


def estimate_entropy(sd, y, noise_y, noise_z, is_train=True, force_symbols=None):
    """estimate_entropy(is_train) of the CHARM model on a state dict whose tensors carry the dtype (and the leaves).
    force_symbols: None or dict(y=..., z=...) (either may be None)."""
    fs = force_symbols or {}
    P = eb_params_of(sd)
    z = orc.hyper_encoder(sd, y)
    med = P["quantiles"][:, 0, 1].detach().view(1, -1, 1, 1)
    vz = z - med
    sz_own = torch.round(vz).detach()
    sz = sz_own if fs.get("z") is None else fs["z"].to(z.dtype)
    with torch.no_grad():
        zq_lik, _ = R.eb_likelihood(sz + med, torch.zeros_like(z), P)
    if is_train:
        z_lik, z_praw = R.eb_likelihood(z, noise_z, P)
        z_hat = ste(vz, sz) + med
    else:
        z_lik, z_praw = zq_lik, zq_lik
        z_hat = sz + med
    hyper_out = orc.hyper_decoder(sd, z_hat)
    c = charm(sd, y, hyper_out, noise_y, is_train, fs.get("y"))
    return dict(y=y, z=z, y_hat=c["y_hat"], z_hat=z_hat, hyper_out=hyper_out, lik_y=c["lik"], lik_z=z_lik, q_lik_y=c["q_lik"], q_lik_z=zq_lik,
                bits_y=R.image_bits(c["lik"]), bits_z=R.image_bits(z_lik), q_bits_y=R.image_bits(c["q_lik"]), q_bits_z=R.image_bits(zq_lik),
                symbols=dict(y=c["symbols"], z=sz.detach()), own_symbols=dict(y=c["own_symbols"], z=sz_own),
                margin=dict(y=c["margin"], z=half_margin(vz.detach())), p_raw=dict(y=c["p_raw"], z=z_praw.detach()), sigma=c["sigma"])


def rate_loss(e, w, scale):
    """sum_n scale * w[n] * (bits_y[n] + bits_z[n])  (w None for 1)."""
    bits = e["bits_y"] + e["bits_z"]
    return (scale * (bits if w is None else w.to(bits.dtype) * bits)).sum()


def eb_aux(sd, dtype):
    P = eb_params_of(sd)
    t = math.log(2 / 1e-9 - 1)
    target = torch.tensor([-t, 0.0, t], dtype=torch.float32).to(dtype)       # the module's fp32 buffer
    return torch.abs(R.eb_logits(P["quantiles"], P, detach=True) - target).sum()


def analysis(sd, x, feat, b1, b2, noise_y, noise_z, w, scale, G=None, aux=False, dtype=torch.float64, force_symbols=None):
    """Encoder + estimate_entropy(is_train=True) + backward of loss = rate (+ <G, y_hat>) (+ the bottleneck's aux loss).
    -> (values dict, {parameter name: gradient}, the leaves' state dict)."""
    L = leaf_state({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.split(".")[0] in MODULES}, dtype)
    to = lambda t: None if t is None else t.detach().to(dtype)
    with _embed_as(dtype):
        y = orc.elic_encoder(L, to(x), to(feat), b1, b2)
    e = estimate_entropy(L, y, to(noise_y), to(noise_z), True, force_symbols)
    loss_rate = rate_loss(e, w, scale)
    total = loss_rate
    if G is not None:
        total = total + (to(G) * e["y_hat"]).sum()
    if aux:
        e["aux"] = eb_aux(L, dtype)
        total = total + e["aux"]
    total.backward()
    e["loss"] = loss_rate.detach()
    names = trainable_names(sd)
    grads = {k: (L[k].grad if L[k].grad is not None else torch.zeros_like(L[k])) for k in names}
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in e.items()}, grads, L


def charm_only(sd, y, hyper_out, noise, w, scale, G=None, dtype=torch.float64, force_symbols=None):
    """The CHARM loop alone: loss = sum_n scale * w[n] * bits[n] + <G, y_hat>.  -> (values, dict(dy, dhyper, params {name: grad}))."""
    names = [k for k in trainable_names(sd) if k.startswith("context_model.")]
    L = leaf_state({k: v.to(dtype) for k, v in sd.items() if k.startswith("context_model.")}, dtype, names)
    y = y.detach().to(dtype).clone().requires_grad_(True)
    h = hyper_out.detach().to(dtype).clone().requires_grad_(True)
    c = charm(L, y, h, noise.to(dtype), True, force_symbols)
    bits, q_bits = R.image_bits(c["lik"]), R.image_bits(c["q_lik"])
    loss = (scale * (bits if w is None else w.to(dtype) * bits)).sum()
    total = loss if G is None else loss + (G.to(dtype) * c["y_hat"]).sum()
    total.backward()
    vals = {k: v.detach() for k, v in c.items()}
    vals.update(bits=bits.detach(), q_bits=q_bits.detach(), loss=loss.detach())
    return vals, dict(dy=y.grad, dhyper=h.grad, params={k: (L[k].grad if L[k].grad is not None else torch.zeros_like(L[k])) for k in names})


def tie_report(own, used, margin, limit=1e-4):
    """(positions where the forced symbols differ from this run's rounding, the largest distance from a tie among them, cap):
    a legitimate difference sits within `limit` of a half-integer; cap = max(1, 1e-5 * decisions) (parity_util CAP_RATE)."""
    diff = own != used.to(own.dtype)
    n = int(diff.sum())
    worst = float(margin[diff].max()) if n else 0.0
    return n, worst, max(1, int(1e-5 * own.numel()))


def analysis_inputs(sd, shape, seed):
    """Seeded inputs of one whole-analysis case: image in [-1, 1], the oracle's VQ indices and feature (latent | one-hot), the two
    noises and the upstream gradient G on y_hat (y is 1/16 of the image, z 1/64)."""
    N, _, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 2 - 1
    with torch.no_grad():
        zq, idx = orc.vq_encode(sd, x)
        feat = orc.onehot_feat(sd, zq, idx)
    noise_y = torch.rand((N, 192, H // 16, W // 16), generator=g) - 0.5
    noise_z = torch.rand((N, 192, H // 64, W // 64), generator=g) - 0.5
    G = torch.randn((N, 192, H // 16, W // 16), generator=g) * 0.05
    return dict(x=x, idx=idx, feat=feat, noise_y=noise_y, noise_z=noise_z, G=G)
