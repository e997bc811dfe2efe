"""The analysis side on the tape (train/autograd.py, train/nets.py) on a real MI355X, against torch autograd over the CPU restatement
of tests/analysis_train_ref.py in fp64: the new convolution adjoints, the CHARM loop alone, the whole analysis side (encoder,
hyper-encoder, entropy bottleneck, hyper-decoder, CHARM), batch invariance, determinism, live weights and poisoned memory.

Bounds: values 2e-4 and gradients 3e-3 relative to the tensor's max (test_generator_and_discriminator_step_vs_oracle's), or 4 x the
error of the helper itself run in fp32 on the same inputs with the same symbols, whichever is larger, computed here
(tests/test_gpu_rate_train.py's rule).  The convolution adjoints use test_conv_wgrad_and_dgrad's 1e-5 / 2e-5.
rint(y - mu) is a decision: the GPU's symbols are fed to the helper (force_symbols); where they differ from the helper's own rounding,
the helper's fp64 y - mu must be within 1e-4 of a half-integer, and at most max(1, 1e-5 x decisions) positions may differ.
The synthetic weights get every scale transform's last bias raised by 1.5 (analysis_train_ref.shifted_state): under 0.1 % of the
sigmas and raw likelihoods may sit at their lower bounds in the helper.

Set DCVIC_ANALYSIS_ERRLOG=<file> to have the worst errors (kernel / fp32 helper) and the near-tie counts appended there."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import analysis_train_ref as AR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
VAL_TOL, GRAD_TOL = 2e-4, 3e-3
LOG = []


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("DCVIC_ANALYSIS_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(LOG) + "\n")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def relclose(a, b, tol, what):
    err = relerr(a, b)
    assert err <= tol, f"{what}: max |diff| / max |ref| = {err:.3e} > {tol:.3e}"
    return err


class Worst:
    """Compares tensors against fp64 with bound = max(project bound, 4 x the fp32 helper's error) and keeps the worst of each kind."""

    def __init__(self, tag):
        self.tag, self.rows = tag, {}

    def check(self, kind, name, got, ref64, ref32, tol):
        if float(ref64.abs().max()) == 0.0:
            assert float(got.detach().abs().max()) == 0.0, f"{name}: the reference gradient is zero, the tape's is not"
            return
        e32 = relerr(ref32, ref64)
        err = relerr(got, ref64)
        bound = max(tol, 4.0 * e32)
        print(f"{self.tag} {kind} {name}: kernel {err:.3e} fp32 helper {e32:.3e} bound {bound:.3e}")
        row = self.rows.setdefault(kind, [0.0, 0.0, ""])
        if err >= row[0]:
            row[0], row[2] = err, name
        row[1] = max(row[1], e32)
        assert err <= bound, f"{self.tag} {name}: max |diff| / max |ref| = {err:.3e} > {bound:.3e} (fp32 helper {e32:.3e})"

    def log(self, extra=""):
        for kind, (err, e32, name) in sorted(self.rows.items()):
            LOG.append(f"{self.tag:28s} {kind:10s} kernel {err:.3e}  fp32 helper {e32:.3e}  worst at {name}")
        if extra:
            LOG.append(f"{self.tag:28s} {extra}")


# ------------------------------------------------------------------------------------------------ model
def build_model(state=None):
    """The synthetic model with the scale transforms' last biases raised (AR.shifted_state), or loaded with `state`; its analysis-side
    ParamGroup; the CPU state dict the helper reads."""
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import full_synth_state_dict, load_synth_weights
    from dc_vic_amd.train import autograd as A
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    sd = AR.shifted_state(full_synth_state_dict(1234))
    if state is not None:
        sd = dict(sd, **state)
    have = set(m.state_dict())
    m.load_state_dict({k: v for k, v in sd.items() if k in have}, strict=False)
    mods = [m.encoder, m.hyperencoder, m.hyperdecoder, m.context_model, m.entropy_model_z]
    return m, A.ParamGroup(mods, DEV), sd


@functools.lru_cache(maxsize=None)
def bundle():
    return build_model()


def analysis_names(m):
    pre = ("encoder.", "hyperencoder.", "hyperdecoder.", "context_model.", "entropy_model_z.")
    return {k: p for k, p in m.named_parameters() if k.startswith(pre)}


# ------------------------------------------------------------------------------------------------ 2. new adjoints
def _conv_case(mod, x, ref_fn, act=0):
    from dc_vic_amd.train import autograd as A
    w, b = rnd(*mod.weight.shape, seed=2, scale=0.1), rnd(*mod.bias.shape, seed=3, scale=0.1)
    mod.weight.data.copy_(w); mod.bias.data.copy_(b)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    y = ref_fn(xr, wr, br)
    g = rnd(*y.shape, seed=4)
    y.backward(g.double())
    grp = A.ParamGroup([mod], DEV)
    ctx = A.Ctx([grp])
    xv = A.Var(x.to(DEV))
    out = A.conv(ctx, xv, mod, act=act)
    relclose(out.data, y, 1e-5, "forward")
    out.grad = g.to(DEV)
    ctx.backward()
    relclose(grp.grad_of(mod.weight), wr.grad, 2e-5, "dW")
    relclose(grp.grad_of(mod.bias), br.grad, 2e-5, "db")
    relclose(xv.grad, xr.grad, 2e-5, "dX")


@pytest.mark.parametrize("Ci,Co,H,W", [(3, 8, 16, 24), (192, 192, 8, 8)])
def test_conv_k5_s2_p2_adjoints(Ci, Co, H, W):
    """Conv2d(k5, s2, p2): the ELIC encoder's conv1..conv4 and the hyper-encoder's conv2 / conv3; its data gradient is the transposed
    convolution ("convT" plan) on the same tensor."""
    from dc_vic_amd.layers import Conv2d
    _conv_case(Conv2d(Ci, Co, 5, 2, 2).to(DEV), rnd(2, Ci, H, W, seed=1), lambda x, w, b: F.conv2d(x, w, b, stride=2, padding=2))


def test_conv_k5_s2_needs_even_sides():
    from dc_vic_amd.layers import Conv2d
    from dc_vic_amd.train import autograd as A
    with pytest.raises(ValueError, match="even"):
        A.conv(A.Ctx(), A.Var(rnd(1, 3, 7, 8).to(DEV)), Conv2d(3, 8, 5, 2, 2).to(DEV))


def test_conv_transpose_k3_s1_p1_adjoints():
    """ConvTranspose2d(k3, s1, p1), 256 -> 320 on 4x8: each hyper-decoder branch's conv3."""
    from dc_vic_amd.layers import ConvTranspose2d
    _conv_case(ConvTranspose2d(256, 320, 3, 1, 1).to(DEV), rnd(2, 256, 4, 8, seed=1), lambda x, w, b: F.conv_transpose2d(x, w, b, stride=1, padding=1))


def test_half_tanh_in_a_differentiable_conv():
    from dc_vic_amd import ops
    from dc_vic_amd.layers import Conv2d
    _conv_case(Conv2d(40, 32, 3, 1, 1).to(DEV), rnd(2, 40, 4, 8, seed=1), lambda x, w, b: 0.5 * torch.tanh(F.conv2d(x, w, b, padding=1)),
               act=ops.ACT_HALF_TANH)


@pytest.mark.parametrize("case", ["res_const", "half_tanh3", "init_relu"])
def test_conv_multi_adjoints(case):
    """conv_multi against torch autograd of the convolution of the concatenation: with a constant source and the residual (the encoder's
    projection([feat, x], res=x)), and with three sources and 0.5 tanh (an LRP's first conv read as [hyper | support | yq]); the sources
    are channel-slice views of one buffer; the per-source weight gradient and the cat + one launch form give the same bits."""
    from dc_vic_amd import ops
    from dc_vic_amd.layers import Conv2d
    from dc_vic_amd.train import autograd as A
    if case == "res_const":
        chans, Co, k, p, act, needs, H, W = (5, 37), 37, 3, 1, ops.ACT_NONE, (False, True), 8, 8
    elif case == "half_tanh3":
        chans, Co, k, p, act, needs, H, W = (32, 40, 32), 32, 5, 2, ops.ACT_HALF_TANH, (True, True, True), 4, 8
    else:           # `init`: accumulators to start from (a partial convolution over leading channels), ReLU on top
        chans, Co, k, p, act, needs, H, W = (37, 5), 33, 5, 2, ops.ACT_RELU, (True, True), 4, 8
    N, Ct = 2, sum(chans)
    xs = [rnd(N, c, H, W, seed=10 + i) for i, c in enumerate(chans)]
    w, b = rnd(Co, Ct, k, k, seed=2, scale=0.1), rnd(Co, seed=3, scale=0.1)
    xr = [t.double().requires_grad_(n) for t, n in zip(xs, needs)]
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv2d(torch.cat(xr, 1), wr, br, padding=p)
    i0 = rnd(N, Co, H, W, seed=5) if case == "init_relu" else None
    ir = i0.double().requires_grad_(True) if i0 is not None else None
    y = 0.5 * torch.tanh(y) if case == "half_tanh3" else y + xr[1] if case == "res_const" else F.relu(y + ir)
    g = rnd(*y.shape, seed=4)
    y.backward(g.double())
    mod = Conv2d(Ct, Co, k, 1, p).to(DEV)
    mod.weight.data.copy_(w); mod.bias.data.copy_(b)
    grp = A.ParamGroup([mod], DEV)
    flats, default = [], A.WGRAD_PER_SOURCE
    for per_source in (True, False):
        A.WGRAD_PER_SOURCE = per_source
        try:
            grp.zero_grad()
            big = torch.full((N, Ct + 4 * len(chans), H, W), float("nan"), device=DEV)
            vs, off = [], 4
            for t, c, n in zip(xs, chans, needs):
                big[:, off:off + c] = t.to(DEV)
                vs.append(A.Var(big[:, off:off + c], needs_grad=n))
                off += c + 4
            ctx = A.Ctx([grp])
            iv = A.Var(i0.to(DEV)) if i0 is not None else None
            out = A.conv_multi(ctx, vs, mod, act=act, res=vs[1] if case == "res_const" else None, init=iv)
            relclose(out.data, y, 1e-5, "forward")
            out.grad = g.to(DEV)
            ctx.backward()
        finally:
            A.WGRAD_PER_SOURCE = default
        relclose(grp.grad_of(mod.weight), wr.grad, 2e-5, "dW")
        relclose(grp.grad_of(mod.bias), br.grad, 2e-5, "db")
        for v, r, n in zip(vs, xr, needs):
            if n:
                relclose(v.grad, r.grad, 2e-5, "dX")
            else:
                assert v.grad is None
        if iv is not None:
            relclose(iv.grad, ir.grad, 2e-5, "dinit")
        flats.append(grp.grad.clone())
    assert torch.equal(flats[0], flats[1])


# ------------------------------------------------------------------------------------------------ 3. CHARM alone
def _ties(tag, vals_own, vals_used, margin):
    n, worst, cap = AR.tie_report(vals_own, vals_used, margin)
    print(f"{tag}: {n} symbol(s) differ from the helper's rounding (cap {cap}), largest distance from a tie {worst:.3e}")
    assert n <= cap and worst < 1e-4, f"{tag}: {n} differing symbols (cap {cap}), largest distance from a tie {worst:.3e}"
    return f"symbols differing from the fp64 helper's rounding {n} (cap {cap}, largest distance from a tie {worst:.1e})"


@pytest.mark.parametrize("shape", [(2, 192, 4, 8), (1, 192, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_charm_forward_train_vs_helper(shape):
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import nets
    m, grp, sd = bundle()
    N, _, H, W = shape
    y, h = rnd(*shape, seed=21), rnd(N, 256, H, W, seed=22, scale=0.5)        # (symbols up to +-4; at twice these scales 1 % of the helper's likelihoods sit at the bound)
    noise = torch.rand(shape, generator=torch.Generator().manual_seed(23)) - 0.5
    G = rnd(*shape, seed=24, scale=0.05)
    w, scale = torch.tensor([0.7, 1.9][:N]), 0.01
    grp.zero_grad()
    ctx = A.Ctx([grp])
    yv, hv = A.Var(y.to(DEV)), A.Var(h.to(DEV))
    bits, q_bits, loss = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), torch.zeros(1, device=DEV)
    r = nets.charm_forward_train(ctx, m.context_model, yv, hv, m.entropy_model_y, noise.to(DEV), w.to(DEV), scale, bits, loss, q_bits=q_bits)
    r["y_hat"].grad = G.to(DEV)
    ctx.backward()
    sym = r["symbols"].cpu()
    v64, g64 = AR.charm_only(sd, y, h, noise, w, scale, G, force_symbols=sym)
    v32, g32 = AR.charm_only(sd, y, h, noise, w, scale, G, dtype=torch.float32, force_symbols=sym)
    tag = "charm " + "x".join(map(str, shape))
    tie_line = _ties(tag, v64["own_symbols"], sym, v64["margin"])
    share = AR.clamped_share(v64)
    assert max(share) < 1e-3, share
    W_ = Worst(tag)
    for name, got in (("y_hat", r["y_hat"].data), ("lik", r["likelihood"]), ("q_lik", r["q_likelihood"]), ("bits", bits), ("q_bits", q_bits),
                      ("loss", loss)):
        W_.check("value", name, got.reshape(v64[name].shape), v64[name], v32[name], VAL_TOL)
    W_.check("grad", "dy", yv.grad, g64["dy"], g32["dy"], GRAD_TOL)
    W_.check("grad", "dhyper_out", hv.grad, g64["dhyper"], g32["dhyper"], GRAD_TOL)
    params = analysis_names(m)
    n = 0
    for name, ref in g64["params"].items():
        W_.check("grad", name, grp.grad_of(params[name]), ref, g32["params"][name], GRAD_TOL)
        n += 1
    assert n == 18 * 6
    W_.log(tie_line)


# ------------------------------------------------------------------------------------------------ 4. - 7. the whole analysis side
CASES = {"2x64x64": ((2, 3, 64, 64), 11), "1x64x128": ((1, 3, 64, 128), 12)}
BETA_RATE, BETA_VQ, WEIGHTS = [2.29, 0.62], [3.0, 1.5], [0.7, 1.9]


@functools.lru_cache(maxsize=None)
def inputs(case):
    shape, seed = CASES[case]
    return AR.analysis_inputs(bundle()[2], shape, seed)


def run_tape(m, grp, I, N, keep=slice(None), aux=True):
    """Forward + backward of the analysis side on images `keep` of the inputs I: loss = rate + <G, y_hat> (+ aux).  -> CPU results."""
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import nets
    H, W = I["x"].shape[2:]
    d = lambda t: t[keep].contiguous().to(DEV)
    grp.zero_grad()
    ctx = A.Ctx([grp])
    out = nets.analysis_forward(ctx, m, d(I["x"]), torch.tensor(BETA_RATE)[keep][:N], torch.tensor(BETA_VQ)[keep][:N], vq_indices=d(I["idx"]),
                                noise_y=d(I["noise_y"]), noise_z=d(I["noise_z"]), weights=torch.tensor(WEIGHTS)[keep][:N].to(DEV),
                                scale=1.0 / (H * W))
    aux_v = A.eb_aux_loss(ctx, m.entropy_model_z) if aux else None
    out["quantized_code"]["y"].grad = d(I["G"])
    ctx.backward()
    c = lambda t: t.detach().cpu().clone()
    return dict(y=c(out["latent_code"]["y"].data), z=c(out["latent_code"]["z"].data), y_hat=c(out["quantized_code"]["y"].data),
                z_hat=c(out["quantized_code"]["z"].data), lik_y=c(out["likelihoods"]["y"]), lik_z=c(out["likelihoods"]["z"]),
                q_lik_y=c(out["q_likelihoods"]["y"]), q_lik_z=c(out["q_likelihoods"]["z"]), bits_y=c(out["bits_y"]), bits_z=c(out["bits_z"]),
                q_bits_y=c(out["q_bits_y"]), q_bits_z=c(out["q_bits_z"]), loss=c(out["loss"]), aux=c(aux_v) if aux else None,
                sym_y=c(out["symbols"]["y"]), sym_z=c(out["symbols"]["z"]), dy=c(out["latent_code"]["y"].grad), flat_grad=c(grp.grad))


def compare_with_helper(case, res, tag):
    m, grp, sd = bundle()
    I = inputs(case)
    N, _, H, W = I["x"].shape
    b1, b2, w = torch.tensor(BETA_RATE)[:N], torch.tensor(BETA_VQ)[:N], torch.tensor(WEIGHTS)[:N]
    fs = dict(y=res["sym_y"], z=res["sym_z"])
    ref = {}
    for dtype in (torch.float64, torch.float32):
        ref[dtype] = AR.analysis(sd, I["x"], I["feat"], b1, b2, I["noise_y"], I["noise_z"], w, 1.0 / (H * W), G=I["G"], aux=True, dtype=dtype,
                                 force_symbols=fs)
    (v64, g64, _), (v32, g32, _) = ref[torch.float64], ref[torch.float32]
    ties = [_ties(f"{tag} {k}", v64["own_symbols"][k], fs[k], v64["margin"][k]) for k in "yz"]
    share = AR.clamped_share(v64)
    assert max(share) < 1e-3, share
    W_ = Worst(tag)
    for name in ("y", "z", "y_hat", "z_hat", "lik_y", "lik_z", "q_lik_y", "q_lik_z", "bits_y", "bits_z", "q_bits_y", "q_bits_z", "loss", "aux"):
        W_.check("value", name, res[name].reshape(v64[name].shape), v64[name], v32[name], VAL_TOL)
    params = analysis_names(m)
    names = AR.trainable_names(sd)
    assert sorted(params) == names and len(names) == len(grp.params) == 339
    off = {}
    o = 0
    for p in grp.params:
        off[id(p)] = (o, p.numel())
        o += p.numel()
    for name in names:
        a, n = off[id(params[name])]
        W_.check("grad", name, res["flat_grad"][a:a + n].view(params[name].shape), g64[name], g32[name], GRAD_TOL)
    assert float(g64["entropy_model_z.quantiles"].abs().max()) > 0        # the aux loss reaches the quantiles
    W_.log("; ".join(f"{k}: {t}" for k, t in zip("yz", ties)))


@functools.lru_cache(maxsize=None)
def whole(case):
    m, grp, _ = bundle()
    I = inputs(case)
    return run_tape(m, grp, I, I["x"].shape[0])


@pytest.mark.parametrize("case", list(CASES))
def test_analysis_forward_vs_helper(case):
    """Every value and every parameter gradient of the five modules (339 tensors) against autograd over the helper; the bottleneck's
    aux loss is part of the loss, so `quantiles` has a gradient too."""
    compare_with_helper(case, whole(case), "analysis " + case)


def test_batch_invariance_and_determinism():
    """Image 0 alone and image 0 inside a batch of 3 (images 0, 1, 0 of the 2x64x64 case): y_hat, bits, q_bits and dy of image 0 are
    bit-identical; a second run of the batch repeats every bit, parameter gradients included."""
    m, grp, _ = bundle()
    I = inputs("2x64x64")
    one = run_tape(m, grp, I, 1, keep=torch.tensor([0]))
    three = run_tape(m, grp, I, 3, keep=torch.tensor([0, 1, 0]))
    for k in ("y", "y_hat", "z_hat", "lik_y", "q_lik_y", "bits_y", "bits_z", "q_bits_y", "q_bits_z", "dy", "sym_y"):
        assert torch.equal(one[k][0], three[k][0]), k
        assert torch.equal(three[k][2], three[k][0]), k
    again = run_tape(m, grp, I, 3, keep=torch.tensor([0, 1, 0]))
    for k, v in three.items():
        assert torch.equal(v, again[k]), k
    assert torch.isfinite(three["flat_grad"]).all() and bool(three["flat_grad"].abs().max() > 0)


def test_live_weights_after_an_in_place_update():
    """Forward + backward, every parameter changed in place by about 1 % (the way the fused Adam kernel writes: torch sees no version
    change), refresh_plans, run again: the bits of a freshly built model loaded with the changed weights."""
    m, grp, _ = build_model()
    I = inputs("1x64x128")
    before = run_tape(m, grp, I, 1)
    g = torch.Generator().manual_seed(31)
    grp.flat.data.mul_((1.0 + 0.01 * torch.randn(grp.flat.numel(), generator=g)).to(DEV))
    grp.refresh_plans()
    after = run_tape(m, grp, I, 1)
    assert not torch.equal(before["y_hat"], after["y_hat"]) and not torch.equal(before["bits_z"], after["bits_z"])
    state = {k: p.detach().cpu().clone() for k, p in analysis_names(m).items()}
    m2, grp2, _ = build_model(state)
    for k, p in analysis_names(m2).items():
        assert torch.equal(p.detach().cpu(), state[k]), k
    fresh = run_tape(m2, grp2, I, 1)
    for k, v in after.items():
        assert torch.equal(v, fresh[k]), k


def test_analysis_forward_with_poisoned_memory(monkeypatch):
    """The 2x64x64 case once more with every float tensor torch.empty / empty_like hands out on the GPU filled with NaN (as
    conftest's DCVIC_POISON_EMPTY does): no result depends on what a buffer held -- the same bits, and nothing non-finite."""
    want = whole("2x64x64")
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poisoned(t):
        if t.is_cuda and t.is_floating_point() and t.numel():
            t.fill_(float("nan"))
        return t
    monkeypatch.setattr(torch, "empty", lambda *a, **k: poisoned(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: poisoned(real_empty_like(*a, **k)))
    m, grp, _ = bundle()
    I = inputs("2x64x64")
    from dc_vic_amd.train import kernels
    for t in kernels._WS.values():
        if t.is_floating_point():
            t.fill_(float("nan"))                     # the grow-only workspaces too
    got = run_tape(m, grp, I, 2)
    monkeypatch.undo()
    for k, v in want.items():
        if v.is_floating_point():
            assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], v), k
    compare_with_helper("2x64x64", got, "analysis 2x64x64 poisoned")
