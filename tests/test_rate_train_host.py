"""The differentiable rate term, host side (no GPU): the fp64 restatement the GPU tests pin the kernels to (tests/rate_train_fp64.py)
against central differences and on the planted bound cases, RateLoss.sample_weights against both rate-distortion trainers'
expressions, the third public header include/dcvic_rate.h against _lib.RATE_SIGNATURES, and the entry points' argument checks."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

import rate_train_fp64 as R
import test_cabi
from dc_vic_amd import _lib
from test_focal_host import loss_header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.entropy_oracle import synth_entropy_bottleneck  # noqa: E402


# ---------------------------------------------------------------------------------------------------- the restatement
def _gaussian_terms(y, mu, sigma, u, w, scale):
    """per-element loss terms -scale * w[n] * log2 p (the loss is their sum, and each depends on its own element only)"""
    lik, _ = R.gaussian_likelihood(y, mu, sigma, u)
    return -scale * w.view(-1, 1, 1, 1) * torch.log(lik) / R.LN2


def test_gaussian_restatement_agrees_with_central_differences():
    y, mu, sigma, u, w = (t.double() for t in R.gaussian_inputs((2, 5, 6, 7), 1, plant=False))
    w = torch.tensor([0.7, 1.3], dtype=torch.float64)
    ref = R.gaussian_rate(y, mu, sigma, u, w, 0.37)
    assert abs(float(ref["loss"]) - float(_gaussian_terms(y, mu, sigma, u, w, 0.37).sum())) <= 1e-12 * abs(float(ref["loss"]))
    # interior: away from both bounds and from the kink of |yt - mu|
    inside = (ref["p_raw"] > 1e-6) & (sigma > 0.12) & ((y + u - mu).abs() > 1e-3)
    assert inside.float().mean() > 0.8
    h = 1e-6
    for name, k in (("dy", 0), ("dmu", 1), ("dsigma", 2)):
        args = [y, mu, sigma]
        up, dn = list(args), list(args)
        up[k], dn[k] = args[k] + h, args[k] - h
        fd = (_gaussian_terms(*up, u, w, 0.37) - _gaussian_terms(*dn, u, w, 0.37)) / (2 * h)
        err = ((fd - ref[name]).abs() / ref[name].abs().clamp_min(1e-3))[inside].max()
        print(f"[rate restatement] gaussian {name}: central differences rel err {float(err):.2e}")
        assert err <= 1e-6, (name, float(err))
    assert torch.equal(ref["dmu"], -ref["dy"])


def test_gaussian_bound_rules_on_planted_elements():
    y, mu, sigma, u, w = R.gaussian_inputs((2, 4, 4, 4), 2)
    for dtype in (torch.float64, torch.float32):
        r = R.gaussian_rate(y, mu, sigma, u, None, 1.0, dtype)
        f = lambda k: r[k][0].reshape(-1)
        # sigma = 0.05, yt == mu: a wider scale lowers p, the gradient w.r.t. s is positive and stops at the bound
        assert f("dsigma")[0] == 0 and f("dy")[0] == 0 and f("dmu")[0] == 0 and f("lik")[0] > 0.9
        # sigma = 0.05, v = 0.625: in the tail a wider scale raises p, the gradient is negative and passes
        s, v = R.SCALE_BOUND, 0.625
        a, b = (0.5 - v) / s, (-0.5 - v) / s
        phi = lambda x: math.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        p = 0.5 * math.erfc(-a / math.sqrt(2)) - 0.5 * math.erfc(-b / math.sqrt(2))
        want = -1 / (p * R.LN2) * (-(a * phi(a) - b * phi(b)) / s)
        assert want < 0 and abs(float(f("dsigma")[1]) - want) <= 1e-5 * abs(want)
        assert abs(float(f("dy")[1]) - (-1 / (p * R.LN2)) * (-(phi(a) - phi(b)) / s)) <= 1e-5 * abs(float(f("dy")[1]))
        # |yt - mu| = 12 at sigma = 0.11: p_raw < 1e-9, the value is the bound; the (negative) gradient passes, and is 0 as phi is
        assert f("p_raw")[2] < R.LIK_BOUND and float(f("lik")[2]) == float(torch.tensor(R.LIK_BOUND, dtype=dtype))
        assert f("dy")[2] == 0 and f("dsigma")[2] == 0
        # yt == mu: sign(0) = 0
        assert f("dy")[3] == 0 and f("dmu")[3] == 0 and f("dsigma")[3] > 0
        assert all(bool(torch.isfinite(r[k]).all()) for k in ("dy", "dmu", "dsigma", "bits"))


def test_lower_bound_backward_is_the_stated_rule():
    x = torch.tensor([0.05, 0.05, 0.2, 0.2, 0.11], dtype=torch.float64, requires_grad=True)
    g = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0], dtype=torch.float64)
    out = R.LowerBound.apply(x, 0.11)
    out.backward(g)
    assert out.tolist() == [0.11, 0.11, 0.2, 0.2, 0.11] and x.grad.tolist() == [0.0, -1.0, 1.0, -1.0, 1.0]


def test_eb_restatement_agrees_with_central_differences():
    sd = {k: v.double() for k, v in synth_entropy_bottleneck(5, seed=7, prefix="eb").items()}
    z, u, _ = (t.double() for t in R.eb_inputs((2, 5, 3, 3), 3))
    w = torch.tensor([0.7, 1.3], dtype=torch.float64)
    ref = R.eb_rate(z, u, sd, "eb", w, 0.37)

    def loss_of(zz, sdd):
        P = {k: sdd[f"eb.{k}"] for k in R.EB_NAMES}
        lik, _ = R.eb_likelihood(zz, u, P)
        return -0.37 * w.view(-1, 1, 1, 1) * torch.log(lik) / R.LN2

    h = 1e-6
    inside = ref["p_raw"] > 1e-6
    fd = (loss_of(z + h, sd) - loss_of(z - h, sd)) / (2 * h)
    err = ((fd - ref["dz"]).abs() / ref["dz"].abs().clamp_min(1e-3))[inside].max()
    print(f"[rate restatement] eb dz: central differences rel err {float(err):.2e}")
    assert inside.all() and err <= 1e-6
    worst = 0.0
    for name in R.EB_NAMES:                                              # one entry of every raw parameter tensor
        idx = (3, min(1, sd[f"eb.{name}"].shape[1] - 1), 0)
        up, dn = dict(sd), dict(sd)
        up[f"eb.{name}"], dn[f"eb.{name}"] = sd[f"eb.{name}"].clone(), sd[f"eb.{name}"].clone()
        up[f"eb.{name}"][idx] += h
        dn[f"eb.{name}"][idx] -= h
        fd = float((loss_of(z, up).sum() - loss_of(z, dn).sum()) / (2 * h))
        got = float(ref["grads"][name][idx])
        worst = max(worst, abs(fd - got) / max(abs(got), 1e-3))
    print(f"[rate restatement] eb raw parameters: central differences rel err {worst:.2e}")
    assert worst <= 1e-6
    # the auxiliary loss: the gradient reaches quantiles only and matches central differences
    aux, dq = R.eb_aux(sd, "eb")
    for idx in ((0, 0, 0), (2, 0, 1), (4, 0, 2)):
        up, dn = dict(sd), dict(sd)
        up["eb.quantiles"], dn["eb.quantiles"] = sd["eb.quantiles"].clone(), sd["eb.quantiles"].clone()
        up["eb.quantiles"][idx] += h
        dn["eb.quantiles"][idx] -= h
        fd = float((R.eb_aux(up, "eb")[0] - R.eb_aux(dn, "eb")[0]) / (2 * h))
        assert abs(fd - float(dq[idx])) <= 1e-6 * abs(fd)
    assert float(aux) > 0


# ---------------------------------------------------------------------------------------------------- RateLoss.sample_weights
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_sample_weights_reproduce_both_trainer_expressions(reduction):
    from dc_vic_amd.registry import LOSS_REGISTRY
    from dc_vic_amd.train.losses import RateLoss
    assert LOSS_REGISTRY.get("RateLoss") is RateLoss
    loss = RateLoss(loss_weight=0.6, target_rate=0.0, reduction=reduction)
    g = torch.Generator().manual_seed(5)
    N, num_pixel = 4, 256 * 256
    bits = 2000.0 * torch.rand(N, generator=g, dtype=torch.float64) + 100.0

    def rate_loss(bpp):                                                  # rate_loss.py:19-24
        bpp = bpp.mean() if reduction == "mean" else bpp.sum() if reduction == "sum" else bpp
        return 0.6 * bpp

    # RateDistortionVqCodeTrainer: rate_loss(outputs.bpp), bpp = sum(bits) / (N * num_pixel), a scalar
    want = rate_loss(bits.sum() / (N * num_pixel))
    w = loss.sample_weights(N, num_pixel)
    assert w.dtype == torch.float32 and tuple(w.shape) == (N,) and w.is_contiguous()
    assert abs(float((w.double() * bits).sum()) - float(want)) <= 1e-7 * float(want)
    # DualBetaCondRateDistortionVqCodeTrainer with sample_beta_batch: _calc_batch_bpp, rate_loss, apply_loss_weight
    beta_rate = torch.tensor([0.0, 2.29, 0.16, 3.0])
    for beta_weight in (torch.exp(beta_rate), beta_rate + 1.0):         # beta_policy exp / linear with beta_offset 1
        rate = rate_loss(bits / num_pixel)
        want = (rate * beta_weight.double()).mean()                      # apply_loss_weight (a scalar rate broadcasts)
        w = loss.sample_weights(N, num_pixel, beta_weight)
        assert w.dtype == torch.float32 and tuple(w.shape) == (N,) and w.is_contiguous()
        assert abs(float((w.double() * bits).sum()) - float(want)) <= 1e-6 * float(want), (reduction, float(want))
    with pytest.raises(ValueError, match="beta_weight"):
        loss.sample_weights(N, num_pixel, torch.ones(N + 1))


def test_rate_loss_keywords():
    from dc_vic_amd.train.losses import RateLoss
    assert (RateLoss(0.5).reduction, RateLoss(0.5).target_rate) == ("mean", 0.0)
    with pytest.raises(ValueError, match="reduction"):
        RateLoss(0.5, reduction="batchmean")
    with pytest.raises(ValueError, match="unknown"):
        RateLoss(0.5, gamma=2.0)


# ---------------------------------------------------------------------------------------------------- the third header
def test_rate_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_rate.h"))
    assert sorted(protos) == ["dcvic_eb_aux_loss_f32", "dcvic_eb_rate_train_f32", "dcvic_eb_rate_train_workspace_doubles",
                              "dcvic_gaussian_rate_train_f32"]
    assert protos["dcvic_eb_rate_train_workspace_doubles"] == (C.c_longlong, [C.c_int, C.c_int, C.c_int])
    p, q, i, d = C.c_void_p, C.c_longlong, C.c_int, C.c_double
    assert protos["dcvic_gaussian_rate_train_f32"] == (i, [p, q, p, p, q, p, q, p, d, p, q, p, q, p, p, p, q, p, p, q, p, i, i, i, p])
    assert protos["dcvic_eb_rate_train_f32"] == (i, [p, p, p, p, i, p, d, p, p, p, p, p, p, p, i, i, i, p])
    assert protos["dcvic_eb_aux_loss_f32"] == (i, [p, p, p, p, p, i, i, p])
    assert test_cabi.signature_mismatches(_lib.RATE_SIGNATURES, protos) == []
    others = dict(loss_header_prototypes(os.path.join(ROOT, "include", "dcvic.h")), **loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_loss.h")))
    assert not set(protos) & set(others)
    assert not set(_lib.RATE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES))
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the comparison catches a double declared as float and a missing parameter
    for sig in ("i:ppppipfpppppppiiip", "i:ppppipdppppppiiip"):
        bad = test_cabi.signature_mismatches(dict(_lib.RATE_SIGNATURES, dcvic_eb_rate_train_f32=sig), protos)
        assert len(bad) == 1 and bad[0].startswith("dcvic_eb_rate_train_f32:"), (sig, bad)
    # the host-side size query: ln p per element and one partial per image and 2048-element span; nothing for an empty tensor
    ws = L.dcvic_eb_rate_train_workspace_doubles
    assert ws(8, 192, 16) == 8 * 192 * 16 + 8 * 2 and ws(3, 5, 9) == 3 * 45 + 3 and ws(0, 5, 9) == 0 and ws(2, 0, 9) == 0 and ws(2, 5, 0) == 0


# Every case breaks one rule and keeps the others valid (see test_cabi._NO_GPU_PRELUDE: every GPU hidden, dummy non-null addresses).
_RATE_ARG_CHECKS = r"""
D = C.c_double
# gaussian_rate_train(y, y_bs, mu, sigma, ms_bs, noise, noise_bs, w, scale, y_hat, yh_bs, lik, lik_bs, bits, loss, dy, dy_bs, dmu, dsigma,
#                     dms_bs, ws, N, C, HW, stream); baseline N = 2, C = 3, HW = 4 (C*HW = 12)
def gr(y=P, y_bs=12, mu=P, sigma=P, ms_bs=12, noise=P, noise_bs=12, w=None, y_hat=P, yh_bs=12, lik=P, lik_bs=12, bits=P, loss=P, dy=P, dy_bs=12,
       dmu=P, dsigma=P, dms_bs=12, ws=P, N=2, Cc=3, HW=4):
    return L.dcvic_gaussian_rate_train_f32(y, LL(y_bs), mu, sigma, LL(ms_bs), noise, LL(noise_bs), w, D(1.0), y_hat, LL(yh_bs), lik, LL(lik_bs),
                                           bits, loss, dy, LL(dy_bs), dmu, dsigma, LL(dms_bs), ws, N, Cc, HW, None)
name = "dcvic_gaussian_rate_train_f32"
def starts(rc, *words):
    err(rc, *words)
    assert L.dcvic_last_error().decode().startswith(name), L.dcvic_last_error().decode()
for kw in (dict(N=0), dict(Cc=0), dict(HW=0), dict(N=-1)):
    starts(gr(**kw), "empty")
for kw in (dict(y=None), dict(mu=None), dict(sigma=None), dict(noise=None)):
    starts(gr(**kw), "null pointer")
for kw in (dict(y_bs=11), dict(ms_bs=11), dict(noise_bs=11), dict(yh_bs=11), dict(lik_bs=11), dict(dy_bs=11), dict(dms_bs=11)):
    starts(gr(**kw), "batch stride")
starts(gr(dy=None, dmu=None, dms_bs=0), "batch stride")                       # dsigma alone still needs its stride
starts(gr(N=1025), "1024")
starts(gr(N=1025, bits=None), "1024")                                         # loss alone needs the finishing pass too
starts(gr(ws=None), "workspace")
starts(gr(ws=None, bits=None), "workspace")
starts(gr(y_hat=None, lik=None, bits=None, loss=None, dy=None, dmu=None, dsigma=None), "no output")

# eb_rate_train(z, noise, params, medians, med_stride, w, scale, z_hat, lik, bits, loss, dz, grads, ws, N, C, HW, stream)
full = (C.c_void_p * 14)(*[64] * 14)
def holed(i):
    a = (C.c_void_p * 14)(*[64] * 14)
    a[i] = None
    return a
A = C.addressof
def eb(z=P, noise=P, params=A(full), med=P, stride=3, z_hat=P, lik=P, bits=P, loss=P, dz=P, grads=A(full), ws=P, N=2, Cc=3, HW=4):
    return L.dcvic_eb_rate_train_f32(z, noise, params, med, stride, None, D(1.0), z_hat, lik, bits, loss, dz, grads, ws, N, Cc, HW, None)
name = "dcvic_eb_rate_train_f32"
for kw in (dict(N=0), dict(Cc=0), dict(HW=0)):
    starts(eb(**kw), "empty")
for kw in (dict(z=None), dict(noise=None), dict(params=None), dict(med=None)):
    starts(eb(**kw), "null pointer")
for i in (0, 4, 5, 9, 13):
    h = holed(i)
    starts(eb(params=A(h)), "null pointer")
    starts(eb(grads=A(h)), "null pointer in grads")
starts(eb(stride=0), "med_stride")
starts(eb(N=1025), "1024")
starts(eb(ws=None), "workspace")
starts(eb(ws=None, bits=None), "workspace")
starts(eb(z_hat=None, lik=None, bits=None, loss=None, dz=None, grads=None), "no output")

# eb_aux_loss(params, quantiles, target, aux, dquantiles, accumulate, C, stream)
def ax(params=A(full), q=P, t=P, aux=P, dq=P, Cc=3):
    return L.dcvic_eb_aux_loss_f32(params, q, t, aux, dq, 0, Cc, None)
name = "dcvic_eb_aux_loss_f32"
starts(ax(Cc=0), "C=0")
h7 = holed(7)
for kw in (dict(params=None), dict(q=None), dict(t=None), dict(params=A(h7))):
    starts(ax(**kw), "null pointer")
starts(ax(aux=None, dq=None), "no output")
print("CHECKS_OK")
"""


def test_rate_argument_checks_without_gpu():
    """The three entry points reject null required pointers, zero sizes, batch strides below C*HW, N > 1024 with bits or loss, a
    missing workspace and a call without outputs, with a message that starts with the entry point's name, before any launch."""
    test_cabi._run_without_gpu(_RATE_ARG_CHECKS)
