"""The differentiable rate term on the GPU (csrc/rate_train.hip, include/dcvic_rate.h): the training forward of the two entropy
models and the rate loss's gradients against the fp64 restatement of tests/rate_train_fp64.py (PARITY UNPINNED: CompressAI is not
importable), the bit-exact properties of the contract, the tape ops, the modules and the stage 1-2 trainer expression end to end.

Bounds.  The reference's arithmetic is fp32, so every error is measured against fp64 and bounded by 4 x the error of the same
restatement run in fp32 on the CPU on the same inputs (the device's erfcf / expf / tanhf differ from the host's by a few ulp), or by
the project's loss floors, whichever is larger: 1e-6 relative for values, 1e-5 of the tensor's max for gradients, 1e-5 absolute for
likelihoods.  Each test prints the kernel's error, the fp32 restatement's and the bound before it asserts (`pytest -s`;
profiles/rate_train_errors_vs_fp64.log is that output)."""
import functools
import json
import math
import os
import sys

import pytest
import torch

import rate_train_fp64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.entropy_oracle import synth_entropy_bottleneck  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
SCALE = 0.37


def _dev(t):
    return t.to("cuda").contiguous() if t is not None else None


def _report(what, got, fp32, bound):
    print(f"[rate_train] {what}: kernel err {got:.2e}, fp32 restatement err {fp32:.2e}, bound {bound:.2e}")
    assert got <= bound, (what, got, fp32, bound)


# ---------------------------------------------------------------------------------------------------- Gaussian conditional
GAUSS_CASES = {"dense": (2, 32, 16, 16), "slice_view": (3, 32, 16, 16), "scalar_path": (1, 5, 3, 7), "hw1": (2, 3, 1, 1), "five_blocks": (2, 40, 16, 16)}


@functools.lru_cache(maxsize=None)
def gauss_case(name, weighted=True):
    """(CPU inputs, fp64 restatement, fp32 restatement), computed once and shared"""
    y, mu, sigma, u, w = R.gaussian_inputs(GAUSS_CASES[name], 100 + list(GAUSS_CASES).index(name))
    w = w if weighted else None
    return (y, mu, sigma, u, w), R.gaussian_rate(y, mu, sigma, u, w, SCALE), R.gaussian_rate(y, mu, sigma, u, w, SCALE, torch.float32)


def gauss_device_inputs(name, weighted=True):
    """The case's inputs on the device; `slice_view` places y, noise (and dy) at channels 32:64 of 192-channel tensors and mu, sigma
    in the two halves of one parameter tensor, as the CHARM slices are."""
    (y, mu, sigma, u, w), _, _ = gauss_case(name, weighted)
    if name != "slice_view":
        return dict(y=_dev(y), mu=_dev(mu), sigma=_dev(sigma), u=_dev(u), w=_dev(w), dy=None)
    N, C, H, W = y.shape
    Y, U, DY = (torch.full((N, 192, H, W), NAN, device="cuda") for _ in range(3))
    Pm = torch.full((N, 2 * C, H, W), NAN, device="cuda")
    Y[:, 32:64], U[:, 32:64], Pm[:, :C], Pm[:, C:] = _dev(y), _dev(u), _dev(mu), _dev(sigma)
    m, s = Pm.chunk(2, 1)
    return dict(y=Y[:, 32:64], mu=m, sigma=s, u=U[:, 32:64], w=_dev(w), dy=DY[:, 32:64])


def run_gaussian(d, scale=SCALE, grads=True, values=True, fill=None, out=None):
    """One call of the kernel on device inputs `d`; returns the outputs (bits and loss start from zero unless `out` carries them)."""
    from dc_vic_amd.train import kernels as K
    y = d["y"]
    N = y.shape[0]
    new = lambda: torch.full(tuple(y.shape), NAN if fill is None else fill, device="cuda")
    o = out or dict(bits=torch.zeros(N, device="cuda"), loss=torch.zeros(1, device="cuda"))
    if values:
        o.update(y_hat=new(), lik=new())
    if grads:
        o.update(dy=d["dy"] if d.get("dy") is not None else new(), dmu=new(), dsigma=new())
    K.gaussian_rate_train(y, d["mu"], d["sigma"], d["u"], d["w"], scale, y_hat=o.get("y_hat"), lik=o.get("lik"), bits=o["bits"], loss=o["loss"],
                          dy=o.get("dy"), dmu=o.get("dmu"), dsigma=o.get("dsigma"))
    return o


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "null_weights"])
@pytest.mark.parametrize("name", list(GAUSS_CASES))
def test_gaussian_rate_against_fp64(name, weighted):
    _, r64, r32 = gauss_case(name, weighted)
    if name in ("dense", "five_blocks"):
        clamped = float((r64["p_raw"] < R.LIK_BOUND).double().mean())
        print(f"[rate_train] gaussian {name}: {100 * clamped:.4f} % of the restatement's likelihoods are clamped to 1e-9")
        assert 0 < clamped < 1e-3                     # clamping cannot hide an error: under 0.1 %, planted elements included
    o = run_gaussian(gauss_device_inputs(name, weighted))
    torch.cuda.synchronize()
    tag = f"gaussian {name} {'w' if weighted else 'w=NULL'}"
    _report(f"{tag} bits", R.value_err(o["bits"].cpu(), r64["bits"]), R.value_err(r32["bits"], r64["bits"]),
            R.bound(R.value_err(r32["bits"], r64["bits"]), R.VALUE_FLOOR))
    _report(f"{tag} loss", R.value_err(o["loss"].cpu(), r64["loss"]), R.value_err(r32["loss"], r64["loss"]),
            R.bound(R.value_err(r32["loss"], r64["loss"]), R.VALUE_FLOOR))
    _report(f"{tag} lik", R.lik_err(o["lik"].cpu(), r64["lik"]), R.lik_err(r32["lik"], r64["lik"]), R.bound(R.lik_err(r32["lik"], r64["lik"]), R.LIK_FLOOR))
    for k in ("dy", "dmu", "dsigma"):
        assert bool(torch.isfinite(o[k]).all())
        _report(f"{tag} {k}", R.grad_err(o[k].cpu(), r64[k]), R.grad_err(r32[k], r64[k]), R.bound(R.grad_err(r32[k], r64[k]), R.GRAD_FLOOR))
    assert torch.equal(o["dmu"], -o["dy"])
    # the planted elements: blocked scale gradient, passing scale gradient, p_raw < 1e-9, yt == mu
    f = lambda k: o[k][0].reshape(-1).cpu()
    n_planted = min(len(R.PLANTED), f("dy").numel())
    assert f("dsigma")[0] == 0 and f("dy")[0] == 0
    if n_planted > 1:
        assert f("dsigma")[1] < 0
    if n_planted > 2:
        assert float(f("lik")[2]) == float(torch.tensor(R.LIK_BOUND, dtype=torch.float32)) and f("dy")[2] == 0 and f("dsigma")[2] == 0
    if n_planted > 3:
        assert f("dy")[3] == 0 and f("dmu")[3] == 0 and f("dsigma")[3] > 0


def test_gaussian_properties_are_bit_exact():
    from dc_vic_amd import ops
    from dc_vic_amd.entropy import get_scale_table
    from dc_vic_amd.train import kernels as K
    for name in ("dense", "scalar_path", "five_blocks", "slice_view"):
        d = gauss_device_inputs(name)
        a = run_gaussian(d, fill=0.0)
        snap = {k: v.clone() for k, v in a.items()}
        # two runs are equal; outputs do not depend on what outputs and workspace held (NaN-filled here)
        K._workspace(1, d["y"].device, "rate_train", torch.float64).fill_(NAN)
        b = run_gaussian(d)
        for k in snap:
            assert torch.equal(snap[k], b[k]), (name, k)
        # the accumulating outputs double on a second call
        c = run_gaussian(d, out=dict(bits=b["bits"], loss=b["loss"]))
        assert torch.equal(c["bits"], 2 * snap["bits"]) and torch.equal(c["loss"], 2 * snap["loss"])
        # bits, loss and lik do not depend on the gradient outputs
        v = run_gaussian(d, grads=False)
        assert torch.equal(v["bits"], snap["bits"]) and torch.equal(v["loss"], snap["loss"]) and torch.equal(v["lik"], snap["lik"])
        g = run_gaussian(d, values=False)
        assert torch.equal(g["bits"], snap["bits"]) and torch.equal(g["dy"], snap["dy"]) and torch.equal(g["dsigma"], snap["dsigma"])
        # image k of the batch equals the image alone
        for k in range(d["y"].shape[0]):
            one = {key: (t[k:k + 1] if t is not None else None) for key, t in d.items()}
            s = run_gaussian(one)
            assert torch.equal(s["bits"], snap["bits"][k:k + 1]), (name, k)
            for key in ("dy", "dmu", "dsigma", "lik", "y_hat"):
                assert torch.equal(s[key], snap[key][k:k + 1]), (name, k, key)
        # y_hat has the bits of the eval kernel's
        yh = torch.empty(tuple(d["y"].shape), device="cuda")
        ops.gaussian_rate(d["y"], None, d["mu"], d["sigma"], get_scale_table().cuda(), yh, None, None, None, None)
        assert torch.equal(yh, snap["y_hat"])


def test_six_slice_calls_fill_one_gradient_like_one_call():
    from dc_vic_amd.train import kernels as K
    y, mu, sigma, u, w = (_dev(t) for t in R.gaussian_inputs((2, 192, 16, 16), 7))
    whole, parts = torch.full_like(y, NAN), torch.full_like(y, NAN)
    bits_a, bits_b = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    K.gaussian_rate_train(y, mu, sigma, u, w, SCALE, dy=whole, bits=bits_a)
    for k in range(6):
        sl = slice(32 * k, 32 * k + 32)
        K.gaussian_rate_train(y[:, sl], mu[:, sl], sigma[:, sl], u[:, sl], w, SCALE, dy=parts[:, sl], bits=bits_b)
    assert torch.equal(whole, parts) and bool(torch.isfinite(parts).all())
    assert R.value_err(bits_b.cpu(), bits_a.cpu()) <= 1e-6                 # the slices' bits add up (another order of the same sum)


# ---------------------------------------------------------------------------------------------------- entropy bottleneck
EB_CASES = {"trainer_width": (2, 192, 4, 4), "odd": (3, 5, 3, 3), "hw1": (1, 192, 1, 1), "batch8": (8, 7, 4, 4)}


@functools.lru_cache(maxsize=None)
def eb_case(name):
    shape = EB_CASES[name]
    sd = synth_entropy_bottleneck(shape[1], seed=1234 + list(EB_CASES).index(name), prefix="eb")
    z, u, w = R.eb_inputs(shape, 200 + list(EB_CASES).index(name))
    r64, r32 = R.eb_rate(z, u, sd, "eb", w, SCALE), R.eb_rate(z, u, sd, "eb", w, SCALE, torch.float32)
    return (z, u, w, sd), r64, r32, R.eb_aux(sd, "eb"), R.eb_aux(sd, "eb", dtype=torch.float32)


def eb_device_inputs(name):
    z, u, w, sd = eb_case(name)[0]
    return dict(z=_dev(z), u=_dev(u), w=_dev(w), params=[_dev(sd[f"eb.{k}"]) for k in R.EB_NAMES], q=_dev(sd["eb.quantiles"]))


def run_eb(d, scale=SCALE, grads=True, values=True, fill=None, out=None):
    from dc_vic_amd.train import kernels as K
    z = d["z"]
    new = lambda: torch.full(tuple(z.shape), NAN if fill is None else fill, device="cuda")
    o = out or dict(bits=torch.zeros(z.shape[0], device="cuda"), loss=torch.zeros(1, device="cuda"), grads=[torch.zeros_like(p) for p in d["params"]])
    if values:
        o.update(z_hat=new(), lik=new())
    if grads:
        o.update(dz=new())
    K.eb_rate_train(z, d["u"], d["params"], d["q"][:, 0, 1], d["w"], scale, z_hat=o.get("z_hat"), lik=o.get("lik"), bits=o["bits"], loss=o["loss"],
                    dz=o.get("dz"), grads=o["grads"] if grads else None)
    return o


@pytest.mark.parametrize("name", list(EB_CASES))
def test_eb_rate_against_fp64(name):
    from dc_vic_amd.train import kernels as K
    _, r64, r32, (aux64, dq64), (aux32, dq32) = eb_case(name)
    d = eb_device_inputs(name)
    o = run_eb(d)
    tag = f"eb {name}"
    for k in ("bits", "loss"):
        e32 = R.value_err(r32[k], r64[k])
        _report(f"{tag} {k}", R.value_err(o[k].cpu(), r64[k]), e32, R.bound(e32, R.VALUE_FLOOR))
    _report(f"{tag} lik", R.lik_err(o["lik"].cpu(), r64["lik"]), R.lik_err(r32["lik"], r64["lik"]), R.bound(R.lik_err(r32["lik"], r64["lik"]), R.LIK_FLOOR))
    _report(f"{tag} dz", R.grad_err(o["dz"].cpu(), r64["dz"]), R.grad_err(r32["dz"], r64["dz"]), R.bound(R.grad_err(r32["dz"], r64["dz"]), R.GRAD_FLOOR))
    for k, g in zip(R.EB_NAMES, o["grads"]):
        e32 = R.grad_err(r32["grads"][k], r64["grads"][k])
        _report(f"{tag} d{k}", R.grad_err(g.cpu(), r64["grads"][k]), e32, R.bound(e32, R.GRAD_FLOOR))
    # the auxiliary loss and its gradient w.r.t. the quantiles
    t = math.log(2 / 1e-9 - 1)
    target = torch.tensor([-t, 0.0, t], device="cuda")
    dq = torch.full_like(d["q"], NAN)
    aux = K.eb_aux_loss(d["params"], d["q"], target, dq)
    _report(f"{tag} aux", R.value_err(aux.cpu(), aux64), R.value_err(aux32, aux64), R.bound(R.value_err(aux32, aux64), R.VALUE_FLOOR))
    _report(f"{tag} dquantiles", R.grad_err(dq.cpu(), dq64), R.grad_err(dq32, dq64), R.bound(R.grad_err(dq32, dq64), R.GRAD_FLOOR))
    again = dq.clone()
    K.eb_aux_loss(d["params"], d["q"], target, again, accumulate=True, want_value=False)
    assert torch.equal(again, 2 * dq)


def test_eb_properties_are_bit_exact():
    from dc_vic_amd import ops
    from dc_vic_amd.entropy import pack_entropy_bottleneck
    from dc_vic_amd.train import kernels as K
    for name in ("trainer_width", "odd", "batch8"):
        d = eb_device_inputs(name)
        a = run_eb(d, fill=0.0)
        snap = {k: ([g.clone() for g in v] if k == "grads" else v.clone()) for k, v in a.items()}
        N, C, H, W = d["z"].shape
        K._workspace(int(K.lib().dcvic_eb_rate_train_workspace_doubles(N, C, H * W)), d["z"].device, "eb_rate_train", torch.float64).fill_(NAN)
        b = run_eb(d)
        for k in ("bits", "loss", "z_hat", "lik", "dz"):
            assert torch.equal(snap[k], b[k]), (name, k)
        assert all(torch.equal(x, y) for x, y in zip(snap["grads"], b["grads"]))
        c = run_eb(d, out=dict(bits=b["bits"], loss=b["loss"], grads=b["grads"]))
        assert torch.equal(c["bits"], 2 * snap["bits"]) and torch.equal(c["loss"], 2 * snap["loss"])
        assert all(torch.equal(x, 2 * y) for x, y in zip(c["grads"], snap["grads"]))
        v = run_eb(d, grads=False)
        assert torch.equal(v["bits"], snap["bits"]) and torch.equal(v["loss"], snap["loss"]) and torch.equal(v["lik"], snap["lik"])
        for k in range(N):
            one = dict(d, z=d["z"][k:k + 1], u=d["u"][k:k + 1], w=d["w"][k:k + 1])
            s = run_eb(one)
            assert torch.equal(s["bits"], snap["bits"][k:k + 1]), (name, k)
            for key in ("dz", "lik", "z_hat"):
                assert torch.equal(s[key], snap[key][k:k + 1]), (name, k, key)
        # z_hat has the bits of the eval kernel's
        sd = eb_case(name)[0][3]
        packs = tuple(_dev(t) for t in pack_entropy_bottleneck(sd, "eb"))
        zh = torch.empty_like(d["z"])
        ops.eb_rate(d["z"], packs, zh, None, None, None)
        assert torch.equal(zh, snap["z_hat"])


# ---------------------------------------------------------------------------------------------------- tape and modules
def _bottleneck(name):
    from dc_vic_amd.entropy import SteEntropyBottleneck
    sd = eb_case(name)[0][3]
    eb = SteEntropyBottleneck(EB_CASES[name][1])
    eb.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items()}, strict=False)
    return eb.cuda()


def test_tape_ops_seed_and_route_the_gradients():
    from dc_vic_amd.train import autograd as A
    # Gaussian: the seeds add to gradients the Vars already hold; a gradient on y_hat reaches y and not mu
    d = gauss_device_inputs("dense")
    want = run_gaussian(d)
    ctx = A.Ctx()
    y, mu, sigma = A.Var(d["y"]), A.Var(d["mu"]), A.Var(d["sigma"])
    held = {k: torch.full_like(d["y"], v) for k, v in (("y", 0.5), ("mu", -0.25), ("sigma", 2.0))}
    y.grad, mu.grad, sigma.grad = held["y"], held["mu"], held["sigma"]
    bits, loss = torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda")
    y_hat = A.gaussian_rate(ctx, y, mu, sigma, d["u"], d["w"], SCALE, bits, loss)
    assert torch.equal(y_hat.data, want["y_hat"]) and torch.equal(bits, want["bits"]) and torch.equal(loss, want["loss"])
    assert torch.equal(y.grad, want["dy"] + 0.5) and torch.equal(mu.grad, want["dmu"] - 0.25) and torch.equal(sigma.grad, want["dsigma"] + 2.0)
    y_hat.grad = torch.full_like(d["y"], 3.0)
    mu_before = mu.grad.clone()
    ctx.backward()
    assert torch.equal(y.grad, (want["dy"] + 0.5) + 3.0) and torch.equal(mu.grad, mu_before)
    # dy_out: the gradient goes to the caller's view, y is not seeded
    ctx, y2 = A.Ctx(), A.Var(d["y"])
    big = torch.full((2, 192, 16, 16), NAN, device="cuda")
    A.gaussian_rate(ctx, y2, A.const(d["mu"]), A.const(d["sigma"]), d["u"], d["w"], SCALE, None, torch.zeros(1, device="cuda"), dy_out=big[:, 32:64])
    assert y2.grad is None and torch.equal(big[:, 32:64], want["dy"]) and bool(torch.isnan(big[:, :32]).all())

    # entropy bottleneck: parameter gradients land in the ParamGroup's flat buffer at the parameters' views
    eb = _bottleneck("odd")
    group = A.ParamGroup([eb], "cuda")
    dd = eb_device_inputs("odd")
    ref = run_eb(dd)
    ctx = A.Ctx([group])
    z = A.Var(dd["z"])
    z.grad = torch.full_like(dd["z"], 0.5)
    group.grad.fill_(1.0)
    bits, loss = torch.zeros(3, device="cuda"), torch.zeros(1, device="cuda")
    z_hat = A.eb_rate(ctx, z, eb, dd["u"], dd["w"], SCALE, bits, loss)
    assert torch.equal(z_hat.data, ref["z_hat"]) and torch.equal(bits, ref["bits"]) and torch.equal(loss, ref["loss"])
    assert torch.equal(z.grad, ref["dz"] + 0.5)
    off = 0
    for p in group.params:
        name = next(k for k, v in eb.named_parameters() if v is p)
        got = group.grad[off:off + p.numel()].view(p.shape)
        off += p.numel()
        if name == "quantiles":
            assert torch.equal(got, torch.ones_like(got))
        else:
            assert torch.equal(got, ref["grads"][R.EB_NAMES.index(name)] + 1.0), name
    z_hat.grad = torch.full_like(dd["z"], 3.0)
    ctx.backward()
    assert torch.equal(z.grad, (ref["dz"] + 0.5) + 3.0)
    # the auxiliary loss reaches quantiles only
    group.zero_grad()
    aux = A.eb_aux_loss(A.Ctx([group]), eb)
    aux64, dq64 = eb_case("odd")[3]
    assert R.value_err(aux.cpu(), aux64) <= R.bound(R.value_err(eb_case("odd")[4][0], aux64), R.VALUE_FLOOR)
    qv = group.grad_of(eb.quantiles)
    assert int((qv != 0).sum()) == qv.numel() and int((group.grad != 0).sum()) == qv.numel()
    assert R.grad_err(qv.cpu(), dq64) <= R.bound(R.grad_err(eb_case("odd")[4][1], dq64), R.GRAD_FLOOR)
    # without a group the parameters get nothing and the value is the same
    assert torch.equal(A.eb_aux_loss(A.Ctx(), eb), aux)


def test_modules_train_forward_is_reproducible_and_equals_the_noise_form():
    from dc_vic_amd.entropy import SteGaussianMeanScaleConditional
    eb = _bottleneck("odd")
    dd = eb_device_inputs("odd")
    gen = torch.Generator(device="cuda").manual_seed(11)
    a_hat, a_lik = eb(dd["z"], is_train=True, generator=gen)
    gen.manual_seed(11)
    b_hat, b_lik = eb(dd["z"], is_train=True, generator=gen)
    gen.manual_seed(11)
    noise = torch.rand(dd["z"].shape, device="cuda", generator=gen) - 0.5
    c_hat, c_lik = eb(dd["z"], is_train=True, noise=noise)
    assert torch.equal(a_lik, b_lik) and torch.equal(a_lik, c_lik) and torch.equal(a_hat, b_hat) and torch.equal(a_hat, c_hat)
    ref = run_eb(dict(dd, u=noise))
    assert torch.equal(a_lik, ref["lik"]) and torch.equal(a_hat, ref["z_hat"])
    e_hat, e_lik = eb(dd["z"])                                            # is_train=False keeps its bits: the rounded input's likelihood
    assert torch.equal(e_hat, a_hat) and not torch.equal(e_lik, a_lik)
    aux64 = eb_case("odd")[3][0]
    assert R.value_err(eb.loss().cpu(), aux64) <= R.bound(R.value_err(eb_case("odd")[4][0], aux64), R.VALUE_FLOOR)

    gc = SteGaussianMeanScaleConditional().cuda()
    d = gauss_device_inputs("dense")
    params = torch.cat([d["mu"], d["sigma"]], 1)
    gen.manual_seed(12)
    a_hat, a_lik = gc(d["y"], params, is_train=True, generator=gen)
    gen.manual_seed(12)
    b_hat, b_lik = gc(d["y"], params, is_train=True, generator=gen)
    gen.manual_seed(12)
    noise = torch.rand(d["y"].shape, device="cuda", generator=gen) - 0.5
    bits = torch.zeros(2, device="cuda")
    c_hat, c_lik = gc(d["y"], params, is_train=True, noise=noise, bits_out=bits)
    assert torch.equal(a_lik, b_lik) and torch.equal(a_lik, c_lik) and torch.equal(a_hat, c_hat) and torch.equal(a_hat, b_hat)
    ref = run_gaussian(dict(d, u=noise, w=None), scale=1.0)
    assert torch.equal(c_lik, ref["lik"]) and torch.equal(bits, ref["bits"]) and torch.equal(c_hat, ref["y_hat"])
    e_hat, e_lik = gc(d["y"], params)
    assert torch.equal(e_hat, a_hat) and not torch.equal(e_lik, a_lik)


# ---------------------------------------------------------------------------------------------------- the trainer's expression
def test_stage_1_2_rate_expression_end_to_end():
    """DualBetaCondRateDistortionVqCodeTrainer with sample_beta_batch and beta_policy exp (config/exp1_stage1_2.yaml): rate =
    mean_n(loss_weight * (bits_y[n] + bits_z[n]) / num_pixel * exp(beta_rate[n])) on y (4, 192, 16, 16) -- six CHARM slices filling
    one gradient -- and z (4, 192, 4, 4), through RateLoss.sample_weights and the tape, against the fp64 restatement."""
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train.losses import RateLoss
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        entry = dict(json.load(f)["exp1_stage1_2.yaml"]["loss"]["rate_loss"])
    assert entry.pop("type") == "RateLoss" and entry == dict(loss_weight=0.5, reduction="none")
    rate_loss = RateLoss(**entry)
    N, num_pixel = 4, 256 * 256
    beta_w = torch.exp(torch.tensor([0.0, 2.29, 0.16, 3.0]))
    w = rate_loss.sample_weights(N, num_pixel, beta_w.cuda())
    assert w.is_cuda and w.dtype == torch.float32

    y, mu, sigma, uy, _ = R.gaussian_inputs((N, 192, 16, 16), 31)
    sd = synth_entropy_bottleneck(192, seed=77, prefix="eb")
    z, uz, _ = R.eb_inputs((N, 192, 4, 4), 32)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        wd = (0.5 * beta_w.to(dtype) / (N * num_pixel))
        gy, gz = R.gaussian_rate(y, mu, sigma, uy, wd, 1.0, dtype), R.eb_rate(z, uz, sd, "eb", wd, 1.0, dtype)
        # the trainer's own words: _calc_batch_bpp, RateLoss(reduction none), apply_loss_weight
        bpp = (gy["bits"] + gz["bits"]) / num_pixel
        value = ((0.5 * bpp) * beta_w.to(dtype)).mean()
        assert abs(float(value) - float(gy["loss"] + gz["loss"])) <= (1e-12 if dtype == torch.float64 else 1e-5) * float(value)
        ref[dtype] = dict(value=value, dy=gy["dy"], dmu=gy["dmu"], dsigma=gy["dsigma"], dz=gz["dz"], grads=gz["grads"])

    eb = _bottleneck("trainer_width")
    eb.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items()}, strict=False)
    group = A.ParamGroup([eb], "cuda")
    ctx = A.Ctx([group])
    Y, MU, SG, UY = _dev(y), _dev(mu), _dev(sigma), _dev(uy)
    dy = torch.full_like(Y, NAN)
    bits, loss = torch.zeros(N, device="cuda"), torch.zeros(1, device="cuda")
    mus, sgs = [], []
    for k in range(6):
        sl = slice(32 * k, 32 * k + 32)
        mus.append(A.Var(MU[:, sl]))
        sgs.append(A.Var(SG[:, sl]))
        A.gaussian_rate(ctx, A.Var(Y[:, sl]), mus[-1], sgs[-1], UY[:, sl], w, 1.0, bits, loss, dy_out=dy[:, sl])
    zv = A.Var(_dev(z))
    A.eb_rate(ctx, zv, eb, _dev(uz), w, 1.0, bits, loss)
    ctx.backward()
    torch.cuda.synchronize()
    r64, r32 = ref[torch.float64], ref[torch.float32]
    e32 = R.value_err(r32["value"], r64["value"])
    _report("stage 1-2 rate value", R.value_err(loss.cpu(), r64["value"]), e32, R.bound(e32, R.VALUE_FLOOR))
    got = dict(dy=dy, dmu=torch.cat([v.grad for v in mus], 1), dsigma=torch.cat([v.grad for v in sgs], 1), dz=zv.grad)
    for k, g in got.items():
        e32 = R.grad_err(r32[k], r64[k])
        _report(f"stage 1-2 rate {k}", R.grad_err(g.cpu(), r64[k]), e32, R.bound(e32, R.GRAD_FLOOR))
    for k in R.EB_NAMES:
        e32 = R.grad_err(r32["grads"][k], r64["grads"][k])
        _report(f"stage 1-2 rate d{k}", R.grad_err(group.grad_of(getattr(eb, k)).cpu(), r64["grads"][k]), e32, R.bound(e32, R.GRAD_FLOOR))
