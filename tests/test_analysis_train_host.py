"""The analysis-side tape, host side (no GPU): the torch restatement the GPU tests pin the tape to (tests/analysis_train_ref.py) against
the oracle's eval CHARM and against central differences, the fourth public header include/dcvic_train.h against _lib.TRAIN_SIGNATURES,
and the per-source weight gradient's argument checks."""
import ctypes as C
import os
import sys

import torch

import analysis_train_ref as AR
import test_cabi
from dc_vic_amd import _lib
from test_focal_host import loss_header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import dcvic_oracle as orc  # noqa: E402


def test_helper_eval_mode_is_the_oracles_charm(charm_golden, synth_sd):
    """is_train=False: the helper's loop is oracle.charm_forward (same symbols, y_hat and quantised likelihood, bit for bit in fp32)."""
    G = charm_golden
    y, ho = torch.from_numpy(G["c1_y"]), torch.from_numpy(G["c1_hyper_out"])
    want = orc.charm_forward(synth_sd, y, ho)
    got = AR.charm(synth_sd, y, ho, None, is_train=False)
    assert torch.equal(got["symbols"].int(), want["symbols"])
    assert torch.equal(got["y_hat"], want["y_hat"]) and torch.equal(got["lik"], want["y_likelihood"]) and torch.equal(got["q_lik"], want["y_likelihood"])
    # teacher forcing: the oracle's symbols handed back reproduce it; in training mode the STE output has the same VALUE
    forced = AR.charm(synth_sd, y, ho, None, is_train=False, force_symbols=want["symbols"])
    assert torch.equal(forced["y_hat"], want["y_hat"])
    noise = torch.rand(y.shape, generator=torch.Generator().manual_seed(3)) - 0.5
    tr = AR.charm(synth_sd, y, ho, noise, is_train=True)
    assert torch.equal(tr["symbols"].int(), want["symbols"]) and torch.equal(tr["q_lik"], want["y_likelihood"])
    assert float((tr["y_hat"] - want["y_hat"]).abs().max()) <= 1e-5          # (y - mu) + (s - (y - mu)) + mu rounds differently from s + mu
    assert not torch.equal(tr["lik"], tr["q_lik"])


def test_ste_passes_the_gradient_to_y_only():
    y = torch.tensor([0.3, 1.7, -2.2], dtype=torch.float64, requires_grad=True)
    mu = torch.tensor([0.1, 0.4, 0.25], dtype=torch.float64, requires_grad=True)
    v = y - mu
    out = AR.ste(v, torch.round(v).detach()) + mu
    assert torch.equal(out.detach(), torch.round(v).detach() + mu.detach())
    out.sum().backward()
    assert torch.equal(y.grad, torch.ones(3, dtype=torch.float64)) and torch.equal(mu.grad, torch.zeros(3, dtype=torch.float64))
    assert abs(float(AR.half_margin(torch.tensor([2.5000001], dtype=torch.float64))) - 1e-7) < 1e-12


def test_helper_gradients_match_central_differences(synth_sd):
    """fp64, y (1, 192, 2, 2), symbols held at the base run's: directional central differences of loss = rate + <G, y_hat> along
    parameters whose effect does not pass a straight-through rounding (where autograd and the function's slope differ by design):
    the last slice's scale transform (rate only) and its LRP (y_hat only), and the first slice's scale transform, whose sigma also
    moves nothing but the rate."""
    synth_sd = AR.shifted_state(synth_sd)           # no sigma at the scale bound: there LowerBound's rule replaces the slope
    g = torch.Generator().manual_seed(5)
    y, ho = 2 * torch.randn((1, 192, 2, 2), generator=g), torch.randn((1, 256, 2, 2), generator=g)
    noise, G = torch.rand(y.shape, generator=g) - 0.5, torch.randn(y.shape, generator=g)
    w = torch.tensor([1.3])
    base, grads = AR.charm_only(synth_sd, y, ho, noise, w, 0.01, G)
    sym = base["own_symbols"]
    assert AR.clamped_share(base) == (0.0, 0.0)

    def total(sd):
        v, _ = AR.charm_only(sd, y, ho, noise, w, 0.01, G, force_symbols=sym)
        return float(v["loss"] + (G.double() * v["y_hat"]).sum())
    for name in ("context_model.scale_slice_transforms.5.model.4.weight", "context_model.lrp_slice_transforms.5.model.0.weight",
                 "context_model.scale_slice_transforms.0.model.2.bias"):
        d = torch.randn(synth_sd[name].shape, generator=g, dtype=torch.float64)
        d = d / d.norm()
        eps = 1e-5
        hi, lo = dict(synth_sd), dict(synth_sd)
        hi[name], lo[name] = synth_sd[name].double() + eps * d, synth_sd[name].double() - eps * d
        for k in synth_sd:
            if k.startswith("context_model.") and k != name:
                hi[k] = lo[k] = synth_sd[k].double()
        fd = (total(hi) - total(lo)) / (2 * eps)
        an = float((grads["params"][name] * d).sum())
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (name, fd, an)
        assert abs(an) > 1e-8, name


def test_train_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_train.h"))
    assert sorted(protos) == ["dcvic_conv_wgrad_src_f32"]
    p, q, i = C.c_void_p, C.c_longlong, C.c_int
    assert protos["dcvic_conv_wgrad_src_f32"] == (i, [p, q, i, i, i, p, q, i, i, i, i, i, i, i, i, i, p, i, i, i, p, p])
    assert test_cabi.signature_mismatches(_lib.TRAIN_SIGNATURES, protos) == []
    others = set()
    for h in ("dcvic.h", "dcvic_loss.h", "dcvic_rate.h"):
        others |= set(loss_header_prototypes(os.path.join(ROOT, "include", h)))
    assert not set(protos) & others
    assert not set(_lib.TRAIN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.RATE_SIGNATURES))
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the comparison catches a long long declared as int and a missing parameter
    for sig in ("i:piiiipqiiiiiiiiipiiipp", "i:pqiiipqiiiiiiiiipiipp"):
        bad = test_cabi.signature_mismatches(dict(_lib.TRAIN_SIGNATURES, dcvic_conv_wgrad_src_f32=sig), protos)
        assert len(bad) == 1 and bad[0].startswith("dcvic_conv_wgrad_src_f32:"), (sig, bad)


# Every case breaks one rule and keeps the others valid (see test_cabi._NO_GPU_PRELUDE: every GPU hidden, dummy non-null addresses).
_WGRAD_SRC_ARG_CHECKS = r"""
# conv_wgrad_src(G, g_bs, M, Hg, Wg, X, x_bs, Cs, Hx, Wx, N, KH, KW, stride, pt, pl, dW, Cx_total, c_off, accumulate, workspace, stream)
# baseline: N = 2, M = 8, 4x4 maps, Cs = 5 at c_off = 3 of Cx_total = 16, k3 s1 p1
def ws(G=P, g_bs=8 * 16, M=8, Hg=4, Wg=4, X=P, x_bs=5 * 16, Cs=5, Hx=4, Wx=4, N=2, KH=3, KW=3, stride=1, dW=P, Ct=16, c_off=3, wk=P):
    return L.dcvic_conv_wgrad_src_f32(G, LL(g_bs), M, Hg, Wg, X, LL(x_bs), Cs, Hx, Wx, N, KH, KW, stride, 1, 1, dW, Ct, c_off, 0, wk, None)
name = "dcvic_conv_wgrad_src_f32"
def starts(rc, *words):
    err(rc, *words)
    assert L.dcvic_last_error().decode().startswith(name), L.dcvic_last_error().decode()
for kw in (dict(c_off=-1), dict(c_off=12), dict(Cs=0), dict(Cs=-2), dict(Ct=0), dict(Ct=7), dict(Cs=17), dict(c_off=2 ** 31 - 1)):
    starts(ws(**kw), "Cx_total")
for kw in (dict(g_bs=8 * 16 - 1), dict(x_bs=5 * 16 - 1), dict(x_bs=0)):
    starts(ws(**kw), "batch stride")
for kw in (dict(G=None), dict(X=None), dict(dW=None), dict(wk=None)):
    starts(ws(**kw), "null pointer")
for kw in (dict(N=0), dict(M=0), dict(Hg=0), dict(Wx=0)):
    starts(ws(**kw), "empty map")
for kw in (dict(KH=6), dict(KW=0), dict(stride=5)):
    starts(ws(**kw), "unsupported")
# the existing entry point keeps its messages
rc = L.dcvic_conv_wgrad_f32(P, LL(128), 8, 4, 4, P, LL(80), 0, 4, 4, 2, 3, 3, 1, 1, 1, P, 0, P, None)
err(rc, "conv_wgrad", "empty map")
assert L.dcvic_last_error().decode().startswith("conv_wgrad:")
print("CHECKS_OK")
"""


def test_wgrad_src_argument_checks_without_gpu():
    """dcvic_conv_wgrad_src_f32 rejects a channel range outside [0, Cx_total), batch strides below their maps, null pointers and what
    dcvic_conv_wgrad_f32 rejects, with a message that starts with the entry point's name, before any launch."""
    test_cabi._run_without_gpu(_WGRAD_SRC_ARG_CHECKS)


def test_inference_classes_still_refuse_training_mode(synth_sd):
    """The tape lives in train/nets.py: the inference modules keep raising for is_train=True."""
    import pytest
    from dc_vic_amd.charm import Minnen20CharmContextModel
    cm = Minnen20CharmContextModel(6, 192, 256, 4)
    with pytest.raises(NotImplementedError):
        cm.forward(None, None, None, is_train=True)
