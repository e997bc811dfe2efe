"""Training step on a real MI355X: every backward kernel against torch-CPU autograd of the same op, the
differentiable sub-network forwards against torch autograd over the CPU oracle (per-parameter gradients), and one full
G + D optimisation step (losses, clipped Adam update) against the oracle's torch restatement.
Tolerances: fp32 MFMA fmaf chains vs MKL summation order; gradients are compared relative to the tensor's max magnitude."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def relclose(a, b, tol=2e-4, what=""):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.as_tensor(a).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    den = float(b.abs().max()) + 1e-12
    err = float((a - b).abs().max()) / den
    assert err <= tol, f"{what}: max |diff| / max |ref| = {err:.3e} > {tol}"
    return err


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("case", [
    dict(N=2, Ci=40, Co=72, H=20, W=33, k=3, s=1, p=1), dict(N=3, Ci=192, Co=96, H=16, W=16, k=1, s=1, p=0),
    dict(N=2, Ci=11, Co=64, H=32, W=48, k=4, s=2, p=1), dict(N=2, Ci=64, Co=130, H=17, W=17, k=4, s=1, p=1),
    dict(N=1, Ci=448, Co=256, H=32, W=32, k=3, s=1, p=1)])
def test_conv_wgrad_and_dgrad(case):
    """dW (fp32 MFMA, slab-split, fixed-order reduce) and dX (forward kernel on transposed / flipped weights or the four
    sub-pixel phases for k4/s2) of Conv2d vs torch autograd."""
    from dc_vic_amd import ops
    from dc_vic_amd.layers import Conv2d
    from dc_vic_amd.train import autograd as A
    c = case
    x, w = rnd(c["N"], c["Ci"], c["H"], c["W"], seed=1), rnd(c["Co"], c["Ci"], c["k"], c["k"], seed=2, scale=0.1)
    b = rnd(c["Co"], seed=3, scale=0.1)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br, stride=c["s"], padding=c["p"])
    g = rnd(*y.shape, seed=4)
    y.backward(g)
    mod = Conv2d(c["Ci"], c["Co"], c["k"], c["s"], c["p"]).to(DEV)
    mod.weight.data.copy_(w); mod.bias.data.copy_(b)
    grp = A.ParamGroup([mod], DEV)
    ctx = A.Ctx([grp])
    xv = A.Var(x.to(DEV))
    out = A.conv(ctx, xv, mod)
    relclose(out.data, y, 1e-5, "conv forward")
    out.grad = g.to(DEV)
    ctx.backward()
    relclose(grp.grad_of(mod.weight), wr.grad, 2e-5, "dW")
    relclose(grp.grad_of(mod.bias), br.grad, 2e-5, "db")
    relclose(xv.grad, xr.grad, 2e-5, "dX")
    # accumulation: a second backward adds into the flat gradient buffer
    ctx = A.Ctx([grp]); xv = A.Var(x.to(DEV)); out = A.conv(ctx, xv, mod); out.grad = g.to(DEV); ctx.backward()
    relclose(grp.grad_of(mod.weight), 2 * wr.grad, 2e-5, "dW accumulated")


def test_conv_transpose_and_upsample_grads():
    from dc_vic_amd.layers import Conv2d, ConvTranspose2d, Linear
    from dc_vic_amd.train import autograd as A
    # ConvTranspose2d(k5, s2, p2, op1) -- elic up_conv
    x, w, b = rnd(2, 48, 9, 12, seed=5), rnd(48, 40, 5, 5, seed=6, scale=0.1), rnd(40, seed=7, scale=0.1)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, br, stride=2, padding=2, output_padding=1)
    g = rnd(*y.shape, seed=8); y.backward(g)
    mod = ConvTranspose2d(48, 40, 5, 2, 2, 1).to(DEV)
    mod.weight.data.copy_(w); mod.bias.data.copy_(b)
    grp = A.ParamGroup([mod], DEV); ctx = A.Ctx([grp]); xv = A.Var(x.to(DEV))
    out = A.conv(ctx, xv, mod); relclose(out.data, y, 1e-5, "convT forward")
    out.grad = g.to(DEV); ctx.backward()
    relclose(grp.grad_of(mod.weight), wr.grad, 2e-5, "convT dW"); relclose(grp.grad_of(mod.bias), br.grad, 2e-5, "convT db")
    relclose(xv.grad, xr.grad, 2e-5, "convT dX")
    # frozen nearest-x2 + conv3x3 (ldm Upsample): data gradient only
    x, w, b = rnd(2, 32, 8, 10, seed=9), rnd(32, 32, 3, 3, seed=10, scale=0.1), rnd(32, seed=11, scale=0.1)
    xr = x.clone().requires_grad_(True)
    y = F.conv2d(F.interpolate(xr, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    g = rnd(*y.shape, seed=12); y.backward(g)
    mod = Conv2d(32, 32, 3, 1, 1, upsample=True).to(DEV)
    mod.weight.data.copy_(w); mod.bias.data.copy_(b)
    ctx = A.Ctx([]); xv = A.Var(x.to(DEV)); out = A.conv(ctx, xv, mod)
    relclose(out.data, y, 1e-5, "upsample conv forward"); out.grad = g.to(DEV); ctx.backward()
    relclose(xv.grad, xr.grad, 2e-5, "upsample conv dX")
    # Linear on a [B, C, 1, 1] vector map with fused ReLU (the beta-conditioning MLPs)
    x, w, b = rnd(5, 42, 1, 1, seed=13), rnd(128, 42, seed=14, scale=0.2), rnd(128, seed=15, scale=0.1)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.relu(F.linear(xr.flatten(1), wr, br)); g = rnd(*y.shape, seed=16); y.backward(g)
    mod = Linear(42, 128).to(DEV); mod.weight.data.copy_(w); mod.bias.data.copy_(b)
    grp = A.ParamGroup([mod], DEV); ctx = A.Ctx([grp]); xv = A.Var(x.to(DEV))
    from dc_vic_amd import ops
    out = A.conv(ctx, xv, mod, act=ops.ACT_RELU); out.grad = g.view(5, 128, 1, 1).to(DEV); ctx.backward()
    relclose(grp.grad_of(mod.weight), wr.grad, 2e-5, "linear dW"); relclose(xv.grad.flatten(1), xr.grad.flatten(1), 2e-5, "linear dX")


def test_norm_and_activation_backward():
    from dc_vic_amd import ops
    from dc_vic_amd.layers import GroupNorm, LayerNormC
    from dc_vic_amd.train import autograd as A
    for C, H, W, act in ((64, 9, 7, ops.ACT_SWISH), (704, 8, 8, ops.ACT_SWISH), (128, 16, 16, ops.ACT_NONE)):
        x, ga, be = rnd(2, C, H, W, seed=20, scale=1.5) + 0.3, 1 + 0.1 * rnd(C, seed=21), 0.1 * rnd(C, seed=22)
        xr, gr, br = x.clone().requires_grad_(True), ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
        y = F.group_norm(xr, 32, gr, br, eps=1e-6)
        y = y * torch.sigmoid(y) if act == ops.ACT_SWISH else y
        g = rnd(*y.shape, seed=23); y.backward(g)
        mod = GroupNorm(C).to(DEV); mod.weight.data.copy_(ga); mod.bias.data.copy_(be)
        grp = A.ParamGroup([mod], DEV); ctx = A.Ctx([grp]); xv = A.Var(x.to(DEV))
        out = A.group_norm(ctx, xv, mod, act=act); out.grad = g.to(DEV); ctx.backward()
        relclose(xv.grad, xr.grad, 5e-5, f"GN dx C={C}"); relclose(grp.grad_of(mod.weight), gr.grad, 5e-5, "GN dgamma")
        relclose(grp.grad_of(mod.bias), br.grad, 5e-5, "GN dbeta")
    x, ga, be = rnd(2, 128, 8, 24, seed=24), 1 + 0.1 * rnd(128, seed=25), 0.1 * rnd(128, seed=26)
    xr, gr, br = x.clone().requires_grad_(True), ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
    y = F.layer_norm(xr.permute(0, 2, 3, 1), (128,), gr, br, eps=1e-5).permute(0, 3, 1, 2)
    g = rnd(*y.shape, seed=27); y.backward(g)
    mod = LayerNormC(128).to(DEV); mod.weight.data.copy_(ga); mod.bias.data.copy_(be)
    grp = A.ParamGroup([mod], DEV); ctx = A.Ctx([grp]); xv = A.Var(x.to(DEV))
    out = A.layer_norm_c(ctx, xv, mod); out.grad = g.to(DEV).contiguous(); ctx.backward()
    relclose(xv.grad, xr.grad, 5e-5, "LN dx"); relclose(grp.grad_of(mod.weight), gr.grad, 5e-5, "LN dgamma"); relclose(grp.grad_of(mod.bias), br.grad, 5e-5, "LN dbeta")
    acts = {ops.ACT_RELU: F.relu, ops.ACT_LRELU02: lambda t: F.leaky_relu(t, 0.2), ops.ACT_SIGMOID: torch.sigmoid, ops.ACT_SWISH: F.silu,
            ops.ACT_GELU: F.gelu, ops.ACT_HALF_TANH: lambda t: 0.5 * torch.tanh(t)}
    for a, fn in acts.items():
        x = rnd(2, 8, 6, 5, seed=28 + a); xr = x.clone().requires_grad_(True)
        y = fn(xr); g = rnd(*y.shape, seed=40); y.backward(g)
        ctx = A.Ctx([]); xv = A.Var(x.to(DEV)); out = A.activation(ctx, xv, a); out.grad = g.to(DEV); ctx.backward()
        relclose(out.data, y, 1e-5, f"act {a} fwd"); relclose(xv.grad, xr.grad, 2e-5, f"act {a} bwd")


def test_gates_and_affine_backward():
    from dc_vic_amd.train import autograd as A
    x, t, a = rnd(2, 16, 5, 7, seed=50), rnd(2, 16, 5, 7, seed=51), rnd(2, 16, 5, 7, seed=52)
    rs = [v.clone().requires_grad_(True) for v in (x, t, a)]
    y = rs[0] + rs[1] * torch.sigmoid(rs[2]); g = rnd(*y.shape, seed=53); y.backward(g)
    ctx = A.Ctx([]); vs = [A.Var(v.to(DEV)) for v in (x, t, a)]
    out = A.nlam_gate(ctx, *vs); out.grad = g.to(DEV); ctx.backward()
    for v, r, nm in zip(vs, rs, "xta"):
        relclose(v.grad, r.grad, 2e-5, f"nlam d{nm}")
    rs = [v.clone().requires_grad_(True) for v in (x, t, a)]
    y = rs[0] + 0.7 * (rs[0] * rs[1] + rs[2]); y.backward(g)
    ctx = A.Ctx([]); vs = [A.Var(v.to(DEV)) for v in (x, t, a)]
    out = A.sft(ctx, *vs, w=0.7); out.grad = g.to(DEV); ctx.backward()
    for v, r, nm in zip(vs, rs, ("dec", "scale", "shift")):
        relclose(v.grad, r.grad, 2e-5, f"sft d{nm}")
    for B in (1, 2):      # shared and per-sample beta vectors; with and without the "+ x" of init_fuse
        for add_x in (False, True):
            s, sh = rnd(B, 16, 1, 1, seed=54), rnd(B, 16, 1, 1, seed=55)
            xr, sr, tr = x.clone().requires_grad_(True), s.clone().requires_grad_(True), sh.clone().requires_grad_(True)
            y = xr * (1 + sr) + tr + (xr if add_x else 0); y.backward(g)
            ctx = A.Ctx([]); xv, sv, tv = A.Var(x.to(DEV)), A.Var(s.to(DEV)), A.Var(sh.to(DEV))
            out = A.chan_affine(ctx, xv, sv, tv, add_x=add_x); out.grad = g.to(DEV); ctx.backward()
            relclose(out.data, y, 1e-5, "chan_affine fwd"); relclose(xv.grad, xr.grad, 2e-5, "chan_affine dx")
            relclose(sv.grad, sr.grad, 2e-5, "chan_affine ds"); relclose(tv.grad, tr.grad, 2e-5, "chan_affine dt")
    # fan-out accumulation + channel concat
    xr = x.clone().requires_grad_(True); tr = t.clone().requires_grad_(True)
    y = torch.cat([xr, tr, xr], 1) * 1.0; y2 = y + F.interpolate(xr, scale_factor=2.0)[:, :, ::2, ::2].repeat(1, 3, 1, 1)
    g3 = rnd(*y.shape, seed=56); y2.backward(g3)
    ctx = A.Ctx([]); xv, tv = A.Var(x.to(DEV)), A.Var(t.to(DEV))
    out = A.cat_channels(ctx, [xv, tv, xv]); out.grad = g3.to(DEV); ctx.backward()
    relclose(xv.grad, g3[:, :16] + g3[:, 32:], 2e-5, "cat fan-out"); relclose(tv.grad, g3[:, 16:32], 2e-5, "cat middle")


# ------------------------------------------------------------------------------------------------ the tape's frame and its channel views
# These move data (or add once in fp32, which the CPU does to the same bits): torch.equal against torch slicing, cat and + on the CPU.
# The 3 x 5 plane keeps copy_planes off any float4 path.
def _nan_buffer(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.mark.parametrize("seeded", ["both", "second", "neither"])
@pytest.mark.parametrize("parent", ["dense", "view"])
def test_split_channels(parent, seeded):
    """The parent's gradient is the cat of the views' gradients (zeros for a view that received none, None if none did), added to what
    the parent held before; the parent dense, or a channel-slice view with its own batch stride."""
    from dc_vic_amd.train import autograd as A
    x, g0, g1, pre = rnd(2, 7, 3, 5, seed=70), rnd(2, 3, 3, 5, seed=71), rnd(2, 4, 3, 5, seed=72), rnd(2, 7, 3, 5, seed=73)
    if parent == "dense":
        xd = x.to(DEV)
    else:
        big = _nan_buffer(2, 11, 3, 5)
        big[:, 2:9] = x.to(DEV)
        xd = big[:, 2:9]
    gathered = None if seeded == "neither" else torch.cat([g0 if seeded == "both" else torch.zeros_like(g0), g1], 1)
    for with_pre in (False, True):
        ctx = A.Ctx([])
        pv = A.Var(xd)
        v0, v1 = A.split_channels(ctx, pv, (3, 4))
        assert v0.needs_grad and v1.needs_grad and v0.data.data_ptr() == xd.data_ptr()
        assert torch.equal(v0.data.cpu(), x[:, :3]) and torch.equal(v1.data.cpu(), x[:, 3:])
        if with_pre:
            A.acc(pv, pre.to(DEV))
        if seeded == "both":
            v0.grad = g0.to(DEV)
        if seeded != "neither":
            v1.grad = g1.to(DEV)
        ctx.backward()
        if gathered is None:
            assert (pv.grad is None) if not with_pre else torch.equal(pv.grad.cpu(), pre)
        else:
            assert torch.equal(pv.grad.cpu(), pre + gathered if with_pre else gathered), (parent, seeded, with_pre)
    assert not any(v.needs_grad for v in A.split_channels(A.Ctx([]), A.const(xd), (3, 4)))
    with pytest.raises(ValueError, match="split_channels"):
        A.split_channels(A.Ctx([]), A.Var(xd), (3, 3))


def test_join_channels():
    """Two parts written through `out=` into the slices (3, 4) of one buffer, the second a constant: the first takes its slice of the
    joined Var's gradient as a dense copy of its own, the constant none."""
    from dc_vic_amd import ops
    from dc_vic_amd.train import autograd as A
    a, b, c, g = rnd(2, 3, 3, 5, seed=74), rnd(2, 3, 3, 5, seed=75), rnd(2, 4, 3, 5, seed=76), rnd(2, 7, 3, 5, seed=77)
    buf = _nan_buffer(2, 7, 3, 5)
    ctx = A.Ctx([])
    av, bv = A.Var(a.to(DEV)), A.Var(b.to(DEV))
    p0 = A.add(ctx, av, bv, out=buf[:, :3])
    p1 = A.const(ops.add(c.to(DEV), c.to(DEV), out=buf[:, 3:]))
    joined = A.join_channels(ctx, buf, [p0, p1])
    assert joined.data is buf and torch.equal(buf.cpu(), torch.cat([a + b, c + c], 1))
    seed = g.to(DEV)
    joined.grad = seed
    ctx.backward()
    assert torch.equal(p0.grad.cpu(), g[:, :3]) and p0.grad.is_contiguous()
    assert p0.grad.untyped_storage().data_ptr() != seed.untyped_storage().data_ptr()
    assert p1.grad is None
    assert torch.equal(av.grad.cpu(), g[:, :3]) and torch.equal(bv.grad.cpu(), g[:, :3])
    with pytest.raises(ValueError, match="join_channels"):
        A.join_channels(A.Ctx([]), buf, [p0])


def test_add_into_a_view():
    from dc_vic_amd.train import autograd as A
    a, b, g = rnd(2, 3, 3, 5, seed=78), rnd(2, 3, 3, 5, seed=79), rnd(2, 3, 3, 5, seed=80)
    buf = _nan_buffer(2, 7, 3, 5)
    ctx = A.Ctx([])
    av, bv = A.Var(a.to(DEV)), A.Var(b.to(DEV))
    out = A.add(ctx, av, bv, out=buf[:, 2:5])
    assert out.data.data_ptr() == buf[:, 2:5].data_ptr() and tuple(out.shape) == (2, 3, 3, 5)
    assert torch.equal(buf[:, 2:5].cpu(), a + b)
    assert bool(torch.isnan(buf[:, :2]).all()) and bool(torch.isnan(buf[:, 5:]).all())          # the rest of the buffer is untouched
    out.grad = g.to(DEV)
    ctx.backward()
    assert torch.equal(av.grad.cpu(), g) and torch.equal(bv.grad.cpu(), g)


@pytest.mark.parametrize("source", ["dense", "view"])
def test_conv_forms_give_the_same_bits(source):
    """conv on a bare Var, on a one-element list and through the name conv_multi: the same output, data gradient and flat gradient,
    bit for bit; the source dense, or a channel-slice view with its own batch stride."""
    from dc_vic_amd.layers import Conv2d
    from dc_vic_amd.train import autograd as A
    x, g = rnd(2, 12, 4, 8, seed=81), rnd(2, 20, 4, 8, seed=82)
    mod = Conv2d(12, 20, 3, 1, 1).to(DEV)
    mod.weight.data.copy_(rnd(20, 12, 3, 3, seed=83, scale=0.1)); mod.bias.data.copy_(rnd(20, seed=84, scale=0.1))
    grp = A.ParamGroup([mod], DEV)
    if source == "dense":
        xd = x.to(DEV)
    else:
        big = _nan_buffer(2, 20, 4, 8)
        big[:, 4:16] = x.to(DEV)
        xd = big[:, 4:16]
    got = []
    for form in ("bare", "list", "conv_multi"):
        grp.zero_grad()
        ctx = A.Ctx([grp])
        xv = A.Var(xd)
        out = A.conv(ctx, xv, mod) if form == "bare" else A.conv(ctx, [xv], mod) if form == "list" else A.conv_multi(ctx, [xv], mod)
        out.grad = g.to(DEV)
        ctx.backward()
        got.append((out.data.cpu(), xv.grad.cpu(), grp.grad.cpu().clone()))
    y = F.conv2d(x.double(), mod.weight.detach().cpu().double(), mod.bias.detach().cpu().double(), padding=1)
    relclose(got[0][0], y, 1e-5, "forward")
    assert float(got[0][1].abs().max()) > 0 and float(got[0][2].abs().max()) > 0
    for other in got[1:]:
        for t0, t1, what in zip(got[0], other, ("out", "dx", "flat gradient")):
            assert torch.equal(t0, t1), what


def test_ctx_op_frame():
    """An op whose output never receives a gradient leaves its inputs alone; one that does gets that very tensor; backward() empties
    the tape either way."""
    from dc_vic_amd import ops
    from dc_vic_amd.train import autograd as A
    x = rnd(2, 4, 3, 5, seed=85).to(DEV)
    ctx = A.Ctx([])
    xv, seen = A.Var(x), []
    A.activation(ctx, A.add(ctx, xv, xv), ops.ACT_RELU)
    out = ctx.op(x, seen.append, needs_grad=False)
    assert out.data is x and out.grad is None and not out.needs_grad and len(ctx.tape) == 3
    ctx.backward()
    assert xv.grad is None and seen == [] and ctx.tape == []
    out = ctx.op(x, seen.append)
    g = torch.ones_like(x)
    out.grad = g
    ctx.backward()
    assert len(seen) == 1 and seen[0] is g and ctx.tape == []


def test_attention_backward():
    from dc_vic_amd.train import autograd as A
    N, C, H, W = 2, 128, 8, 16
    qkv = rnd(N, 3 * C, H, W, seed=60, scale=1.2)
    r = qkv.clone().requires_grad_(True)
    q, k, v = r[:, :C].flatten(2), r[:, C:2 * C].flatten(2), r[:, 2 * C:].flatten(2)
    w_ = F.softmax(torch.bmm(q.permute(0, 2, 1), k) * C ** -0.5, dim=2)
    o = torch.bmm(v, w_.permute(0, 2, 1)).view(N, C, H, W)
    g = rnd(N, C, H, W, seed=61); o.backward(g)
    ctx = A.Ctx([]); xv = A.Var(qkv.to(DEV)); out = A.attn_single_head(ctx, xv, C)
    relclose(out.data, o, 2e-4, "attn fwd"); out.grad = g.to(DEV); ctx.backward()
    relclose(xv.grad, r.grad, 2e-4, "attn dqkv")


@pytest.mark.parametrize("shift", [0, 4])
def test_swin_attention_backward(shift):
    from dc_vic_amd.train import autograd as A
    from oracle import dcvic_oracle as O
    N, C, H, W, heads, ws = 2, 128, 16, 24, 8, 8
    qkv, table = rnd(N, 3 * C, H, W, seed=62), 0.5 * rnd(225, heads, seed=63)
    qr, tr = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
    t = qr.flatten(2).transpose(1, 2).view(N, H, W, 3 * C)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    xw = t.view(N, H // ws, ws, W // ws, ws, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, 3 * C)
    B_, T, _ = xw.shape
    qh = xw.reshape(B_, T, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    att = (qh[0] * (C // heads) ** -0.5) @ qh[1].transpose(-2, -1)
    att = att + tr[O._rel_pos_index(ws).view(-1)].view(T, T, -1).permute(2, 0, 1).unsqueeze(0)
    if shift:
        mask = O._shift_mask(H, W, ws, shift); nW = mask.shape[0]
        att = (att.view(B_ // nW, nW, heads, T, T) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, T, T)
    xo = (F.softmax(att, dim=-1) @ qh[2]).transpose(1, 2).reshape(B_, T, C)
    xo = xo.view(N, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, C)
    if shift:
        xo = torch.roll(xo, shifts=(shift, shift), dims=(1, 2))
    o = xo.permute(0, 3, 1, 2)
    g = rnd(N, C, H, W, seed=64); o.backward(g)
    p = torch.nn.Parameter(table.to(DEV), requires_grad=False)
    holder = torch.nn.Module(); holder.t = p
    grp = A.ParamGroup([holder], DEV); ctx = A.Ctx([grp]); xv = A.Var(qkv.to(DEV))
    out = A.swin_attention(ctx, xv, holder.t, heads, ws, shift)
    relclose(out.data, o, 2e-5, "swin fwd"); out.grad = g.to(DEV); ctx.backward()
    relclose(xv.grad, qr.grad, 5e-5, "swin dqkv"); relclose(grp.grad_of(holder.t), tr.grad, 5e-5, "swin dtable")


def test_losses_and_adam():
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import kernels as K
    a, b = rnd(2, 3, 16, 16, seed=70), rnd(2, 3, 16, 16, seed=71)
    ar = a.clone().requires_grad_(True)
    l = 50 * F.mse_loss((ar + 1) / 2, (b + 1) / 2); l.backward()
    ctx = A.Ctx([]); av = A.Var(a.to(DEV)); v = A.mse_loss(ctx, av, b.to(DEV), 50 * 0.25)
    relclose(v, l.reshape(1), 1e-6, "mse value"); relclose(av.grad, ar.grad, 1e-5, "mse grad")
    x = rnd(2, 1, 30, 30, seed=72, scale=2.0)
    for real in (True, False):
        xr = x.clone().requires_grad_(True)
        l = 0.5 * F.binary_cross_entropy_with_logits(xr, torch.full_like(xr, 1.0 if real else 0.0)); l.backward()
        xv = A.Var(x.to(DEV)); v = A.bce_logits_loss(A.Ctx([]), xv, real, 0.5)
        relclose(v, l.reshape(1), 1e-6, "bce value"); relclose(xv.grad, xr.grad, 1e-5, "bce grad")
    lg, tg = rnd(2, 256, 8, 8, seed=73, scale=2.0), torch.randint(0, 256, (2, 8, 8), generator=torch.Generator().manual_seed(74))
    lr_ = lg.clone().requires_grad_(True); l = 0.5 * F.cross_entropy(lr_, tg); l.backward()
    lv = A.Var(lg.to(DEV)); v = A.cross_entropy_loss(A.Ctx([]), lv, tg.to(DEV), 0.5)
    relclose(v, l.reshape(1), 1e-6, "ce value"); relclose(lv.grad, lr_.grad, 1e-5, "ce grad")
    # Adam (3 steps, with the clip factor) vs torch.optim.Adam + clip_grad_norm_
    p0 = rnd(1000, seed=75); pt = p0.clone().requires_grad_(True); opt = torch.optim.Adam([pt], lr=1e-3)
    pd, m, vv = p0.to(DEV), torch.zeros(1000, device=DEV), torch.zeros(1000, device=DEV)
    for step in range(1, 4):
        gr = rnd(1000, seed=80 + step, scale=3.0)
        pt.grad = gr.clone(); torch.nn.utils.clip_grad_norm_([pt], 1.0); opt.step()
        gd = gr.to(DEV)
        gs = K.clip_scale(K.reduce_loss(2, gd, None, 1.0), 1.0)
        K.adam_step(pd, gd, m, vv, 1e-3, 0.9, 0.999, 1e-8, step, gs)
        relclose(pd, pt.detach(), 2e-6, f"adam step {step}")


def test_lpips_alex_value_and_gradient():
    """LPIPS(alex) term (architecture restated, synthetic weights -- parity unpinned against the package) vs torch autograd of
    the same restatement: value and d/d(fake), incl. the 11x11/s4 stem as a space-to-depth 3x3 convolution and MaxPool2d(3, 2)."""
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train.lpips import LPIPSAlex, lpips_loss
    from oracle import train_oracle as T
    L = LPIPSAlex(seed=0).to(DEV)
    lsd = {k: v.detach().cpu().clone() for k, v in L.state_dict().items()}
    assert set(lsd) >= {"net.slice1.0.weight", "net.slice2.3.bias", "net.slice5.10.weight", "lin3.model.1.weight", "scaling_layer.shift"}
    real = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(95)) * 2 - 1
    fake = (real + 0.3 * rnd(2, 3, 64, 96, seed=96)).clamp(-1, 1)
    fr = fake.clone().requires_grad_(True)
    ref = 0.7 * torch.mean(T.lpips_alex(lsd, real, fr)); ref.backward()
    ctx = A.Ctx([]); fv = A.Var(fake.to(DEV))
    val = lpips_loss(ctx, L, real.to(DEV), fv, 0.7)
    ctx.backward()
    relclose(val, ref.detach().reshape(1), 2e-5, "lpips value")
    relclose(fv.grad, fr.grad, 2e-4, "lpips d/dfake")


# ------------------------------------------------------------------------------------------------ networks vs the oracle
@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV})
    m = build_comp_model(opt)
    load_synth_weights(m, 1234)
    return m


def _disc(seed=5):
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator
    torch.manual_seed(seed)
    D = DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, L=10, cond_ch=8,
                                              use_pi=False, include_x=True)
    g = torch.Generator().manual_seed(seed)
    for p in D.parameters():          # deterministic, a bit larger than N(0, 0.02) so the logits carry signal
        p.data.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
    return D


def test_discriminator_and_losses_vs_reference_modules(train_golden):
    """the a20 pieces the reference lets us import, pinned.  tests/golden/train.npz holds the outputs of the
    reference's OWN DualBetaCondTamingNLayerDiscriminator (dual_beta_taming_nlayer_discriminator.py:16-89, kwargs of
    config/exp1_stage1_3.yaml:28-41) and of its VanillaGANLoss / MSELoss / VanillaMSELoss / CrossEntropyLoss modules with the
    YAML's kwargs.  Product side: dc_vic_amd.train.nets + the loss kernels, through the same calls the trainer makes
    (calc_g_loss / run_discriminator / calc_d_loss, dual_cond_gan_distortion_vq_code_trainer.py:192-300): logits, loss values,
    d(adv)/d(fake image) through the HIP data-gradient convs, d(ce)/d(logits)."""
    import json
    from conftest import train_golden_disc_state
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator, nets
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train.trainer import DEFAULT_LOSS
    G = train_golden
    kw = json.loads(str(G["d_kwargs"]))
    D = DualBetaCondTamingNLayerDiscriminator(**kw)             # the YAML's kwargs, unchanged
    sd = train_golden_disc_state(G)
    assert {k: tuple(v.shape) for k, v in D.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}      # same keys and shapes as the reference module
    D.load_state_dict(sd, strict=True)
    D = D.to(DEV)
    lk = json.loads(str(G["loss_kwargs"]))
    assert {"distortion": lk["distortion_loss"]["loss_weight"], "perceptual": lk["perceptual_loss"]["loss_weight"], "gan": lk["gan_loss"]["loss_weight"],
            "code_distortion": lk["code_distortion_loss"]["loss_weight"], "code_ce": lk["code_ce_loss"]["loss_weight"]} == DEFAULT_LOSS
    t = lambda k: torch.from_numpy(np.asarray(G[k])).to(DEV)
    real, fake, b1, b2 = t("real"), t("fake"), torch.from_numpy(G["beta_1"]), torch.from_numpy(G["beta_2"])
    grp = A.ParamGroup([D], DEV)
    # generator side: adv = gan_loss(D(fake), is_real=True, is_disc=False), gradient back to the image
    ctx = A.Ctx([])
    fv = A.Var(fake)
    g_fake = nets.discriminator_forward(ctx, D, fv, b1, b2)
    relclose(g_fake.data, G["d_fake_logits"], 2e-5, "D(fake) logits")
    adv = A.bce_logits_loss(ctx, g_fake, True, DEFAULT_LOSS["gan"])
    relclose(adv, np.asarray(G["adv_loss"]).reshape(1), 2e-5, "adv loss")
    ctx.backward()
    relclose(fv.grad, G["adv_grad_fake"], 2e-4, "d(adv)/d(fake)")
    # discriminator side: 0.5 * BCE(D(real), 1) + 0.5 * BCE(D(fake.detach()), 0)
    dctx = A.Ctx([grp])
    d_real = nets.discriminator_forward(dctx, D, A.const(real), b1, b2)
    d_fake = nets.discriminator_forward(dctx, D, A.const(fake), b1, b2)
    relclose(d_real.data, G["d_real_logits"], 2e-5, "D(real) logits")
    relclose(A.bce_logits_loss(dctx, d_real, True, 0.5), np.asarray(G["d_loss_real"]).reshape(1), 2e-5, "d_real loss")
    relclose(A.bce_logits_loss(dctx, d_fake, False, 0.5), np.asarray(G["d_loss_fake"]).reshape(1), 2e-5, "d_fake loss")
    dctx.tape = []
    # scalar betas
    ds = nets.discriminator_forward(A.Ctx([]), D, A.const(real), 1.51, 2.25)
    relclose(ds.data, G["d_real_logits_scalar_beta"], 2e-5, "D(real) logits, scalar betas")
    # image / code losses as calc_g_loss forms them (MSELoss(50, normalize_img, '0_1') = 50 * mse on [0, 1] = 50 * 0.25 * mse on [-1, 1])
    c2 = A.Ctx([])
    relclose(A.mse_loss(c2, A.Var(fake), real, DEFAULT_LOSS["distortion"] * 0.25), np.asarray(G["distortion_loss"]).reshape(1), 2e-5, "distortion loss")
    relclose(A.mse_loss(c2, A.Var(t("code_b")), t("code_a"), DEFAULT_LOSS["code_distortion"]), np.asarray(G["code_distortion_loss"]).reshape(1), 2e-5,
             "code distortion loss")
    lv = A.Var(t("ce_logits"))
    relclose(A.cross_entropy_loss(c2, lv, t("ce_target"), DEFAULT_LOSS["code_ce"]), np.asarray(G["ce_loss"]).reshape(1), 2e-5, "code CE loss")
    relclose(lv.grad, G["ce_grad"], 2e-5, "d(ce)/d(logits)")


def test_generator_and_discriminator_step_vs_oracle(model, synth_sd):
    """One full optimisation step of the stage-3 trainer on a seeded batch (2 x 64x64, per-sample beta pairs): every loss term,
    every trainable parameter's gradient (decoder / vq_estimator / fusion_module: 33.5 M parameters), the clipped Adam update
    and the D step, against torch autograd + torch.optim over the CPU oracle."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    from dc_vic_amd.train import autograd as A
    from oracle import train_oracle as T
    from oracle.entropy_oracle import EntropyBottleneckOracle
    D = _disc().to(DEV)
    dsd0 = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    tr = DualBetaCondGanDistortionVqCodeTrainer(model, D, lr_g=1e-4, lr_d=1e-4, clip_max_norm=1.0, seed=3)
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(90)) * 2 - 1
    b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
    # ---- oracle
    sd = {k: v.clone() for k, v in synth_sd.items()}
    names = [k for k in sd if k.startswith(T.TRAINABLE_PREFIXES) and sd[k].is_floating_point()]
    for k in names:
        sd[k].requires_grad_(True)
    dsd = {k: v.clone().requires_grad_(True) for k, v in dsd0.items()}
    eb = EntropyBottleneckOracle(synth_sd, "entropy_model_z")
    lsd = {k: v.detach().cpu().clone() for k, v in tr.lpips.state_dict().items()}
    L, oo = T.generator_losses(sd, dsd, x, b1, b2, eb, lsd=lsd)
    total = sum(L.values())
    total.backward()
    # ---- product: forward + losses + backward (no optimizer yet) for the gradient comparison
    tr.g_group.zero_grad()
    ctx = A.Ctx([tr.g_group])
    o = tr.generator_forward(ctx, x, None, b1, b2)
    assert torch.equal(o["gt_vq_indices"].cpu(), oo["gt_idx"]) and torch.equal(o["out_vq_indices"].cpu(), oo["out_idx"]), "integer decisions differ"
    relclose(o["fake"].data, oo["fake"], 2e-4, "fake images")
    glog = tr.calc_g_loss(ctx, o, b1, b2)
    for k in ("distortion", "perceptual", "adv", "code_distortion", "code_ce"):
        relclose(glog[k], L[k].detach().reshape(1), 2e-4, f"loss {k}")
    ctx.backward()
    own = dict(model.named_parameters())
    worst = 0.0
    checked = 0
    for k in names:
        gref = sd[k].grad
        if gref is None:
            continue                                     # e.g. decoder.conv4 (never executed) -> no gradient on either side
        gp = tr.g_group.grad_of(own[k])
        worst = max(worst, relclose(gp, gref, 3e-3, f"grad {k}"))
        checked += 1
    assert checked >= 400, checked          # 403 tensors carry gradients (decoder.conv4 and the unused heads do not)
    print(f'[train parity] {checked} parameter gradients, worst relative error {worst:.6e}')
    unused = [k for k in names if sd[k].grad is None]
    for k in unused:
        assert float(tr.g_group.grad_of(own[k]).abs().max()) == 0.0, k
    # ---- the real step (fresh gradients inside), then compare the updated parameters and the D step
    new = T.clip_and_adam({k: synth_sd[k] for k in names if sd[k].grad is not None}, {k: sd[k].grad for k in names if sd[k].grad is not None}, 1e-4, 1.0)
    log = tr.optimize_parameters(0, dict(real_images=x, beta_rate=b1, beta_vq=b2))
    assert log is not None and abs(log["total"] - float(total.detach())) < 2e-4 * abs(float(total.detach()))
    gnorm = float(torch.sqrt(sum((sd[k].grad.double() ** 2).sum() for k in new)))
    cscale = min(1.0, 1.0 / (gnorm + 1e-6))
    n_cmp = 0
    for k in list(new)[::5]:
        # the first Adam step is -lr * g / (|g| + 1e-8): elements whose clipped gradient is not >> eps amplify any fp32
        # difference in g, so the DELTA is compared where |g| >= 1e-6 (sign regime) and merely bounded by lr elsewhere
        da, db = (own[k].data.cpu() - synth_sd[k]).double(), (new[k] - synth_sd[k]).double()
        big = (sd[k].grad.abs() * cscale) >= 1e-6
        assert float(da.abs().max()) <= 1e-4 * (1 + 1e-3)
        if big.any():
            assert float((da - db)[big].abs().max()) <= 2e-2 * 1e-4, k
            n_cmp += int(big.sum())
    assert n_cmp > 10000, n_cmp
    l_real, l_fake, d_real, d_fake = T.discriminator_losses(dsd, x, oo["fake"], b1, b2)
    for p in dsd.values():
        p.grad = None
    (l_real + l_fake).backward()
    assert abs(log["d_real"] - float(l_real.detach())) < 1e-4 and abs(log["d_fake"] - float(l_fake.detach())) < 1e-4
    newd = T.clip_and_adam(dsd0, {k: dsd[k].grad for k in dsd0}, 1e-4, None)
    for k, p in D.state_dict().items():
        da, db = (p.cpu() - dsd0[k]).double(), (newd[k] - dsd0[k]).double()
        big = dsd[k].grad.abs() >= 1e-6
        if big.any():
            assert float((da - db)[big].abs().max()) <= 2e-2 * 1e-4, k


def test_generator_gradient_at_step2_uses_updated_discriminator(model, synth_sd):
    """inside the generator step the discriminator is not trainable, so its data-gradient plans (flipped /
    transposed weight copies) are cached on the modules; after the D Adam step they must be rebuilt.  GAN-only loss weights
    and a large D learning rate make the adversarial gradient the whole gradient and move D's weights by ~40 % in one step:
    the generator gradients of the SECOND iteration are compared with torch autograd over the oracle evaluated at the
    product's post-step-1 weights.  With a stale plan they are off by tens of percent."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    from dc_vic_amd.train import autograd as A
    from oracle import train_oracle as T
    from oracle.entropy_oracle import EntropyBottleneckOracle
    sd_before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        D = _disc(5).to(DEV)
        w = dict(distortion=0.0, perceptual=0.0, gan=1.0, code_distortion=0.0, code_ce=0.0)
        tr = DualBetaCondGanDistortionVqCodeTrainer(model, D, lr_g=1e-5, lr_d=2e-2, clip_max_norm=None, loss_weights=w, seed=3)
        x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(93)) * 2 - 1
        b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
        d0 = D.main[2].weight.detach().clone()
        assert tr.optimize_parameters(0, dict(real_images=x, beta_rate=b1, beta_vq=b2)) is not None
        moved = float((D.main[2].weight - d0).abs().mean() / d0.abs().mean())
        assert moved > 0.2, moved                      # the D step really changed the weights the G step back-propagates through
        # ---- oracle at the product's current weights
        sd = {k: v.clone() for k, v in synth_sd.items()}
        for k, v in model.state_dict().items():
            if k in sd and sd[k].is_floating_point():
                sd[k] = v.detach().cpu().clone()
        names = [k for k in sd if k.startswith(T.TRAINABLE_PREFIXES) and sd[k].is_floating_point()]
        for k in names:
            sd[k].requires_grad_(True)
        dsd = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
        eb = EntropyBottleneckOracle(synth_sd, "entropy_model_z")
        L, oo = T.generator_losses(sd, dsd, x, b1, b2, eb, w=w)
        sum(L.values()).backward()
        # ---- product: second iteration's forward / backward
        tr.g_group.zero_grad()
        ctx = A.Ctx([tr.g_group])
        o = tr.generator_forward(ctx, x, None, b1, b2)
        # Gradients are comparable only between evaluations that took the same integer decisions.  The oracle's own fp32 order
        # depends on torch's CPU thread count (tests/test_oracle_golden.py sets 8 at import, a lone run of this file does not), so
        # an estimator argmax or a symbol rounding on an fp32 near-tie can differ in either direction: such cases are itemised,
        # capped and bounded, and the oracle is re-evaluated on the product's decisions.
        idx_p, yh_p = o["out_vq_indices"].cpu(), o["y_hat"].data.cpu()
        d_idx = idx_p != oo["out_idx"]
        d_sym = (yh_p - oo["y_hat"]).abs() > 0.5        # (y_hat = round(y - mu) + mu: equal up to mu's 1e-7 unless a rounding flipped)
        if bool(d_idx.any()) or bool(d_sym.any()):
            n_idx, n_sym = int(d_idx.sum()), int(d_sym.sum())
            assert n_idx <= 2 and n_sym <= 2, f"{n_idx} estimator indices / {n_sym} symbols differ from the oracle's"
            lg = oo["logits"].detach()
            pos = d_idx.nonzero()
            for n_, i_, j_ in pos.tolist():
                margin = float(lg[n_, oo["out_idx"][n_, i_, j_], i_, j_] - lg[n_, idx_p[n_, i_, j_], i_, j_])
                assert 0.0 <= margin <= 1e-3 * float(lg.abs().max()), f"estimator index ({n_},{i_},{j_}): oracle margin {margin:.3e} is no near-tie"
            assert float((yh_p - oo["y_hat"])[d_sym].abs().max() if n_sym else 1.0) <= 1.0 + 1e-4    # one quantisation step
            print(f"[train parity] step-2: {n_idx} estimator near-tie(s), {n_sym} symbol near-tie(s): oracle re-evaluated on the product's decisions")
            for k in names:
                sd[k].grad = None
            L, oo = T.generator_losses(sd, dsd, x, b1, b2, eb, w=w, force_y_hat=yh_p, force_out_idx=idx_p)
            sum(L.values()).backward()
        glog = tr.calc_g_loss(ctx, o, b1, b2)
        relclose(glog["adv"], L["adv"].detach().reshape(1), 2e-4, "adv loss at step 2")
        ctx.backward()
        own = dict(model.named_parameters())
        checked, worst = 0, 0.0
        for k in names:
            gref = sd[k].grad
            if gref is None or float(gref.abs().max()) == 0.0:
                continue
            # 1e-2, not the 3e-3 of the first-step test: after the 40 % D step the ORACLE's own gradient of a tensor behind a ReLU
            # (decoder.attn2.trunk_block.1.c2.weight) differs by 4.4e-3 between torch CPU thread counts (8 when the whole suite is
            # collected -- tests/test_oracle_golden.py sets it at import -- against the box's default when this file runs alone:
            # a pre-activation on an fp32 near-zero changes sign and moves one pixel's whole contribution); the product is bit-stable
            # across runs and measures 1.7e-4 / 2.6e-4 / 4.5e-3 against those oracles.  A stale plan is off by tens of percent.
            worst = max(worst, relclose(tr.g_group.grad_of(own[k]), gref, 1e-2, f"step-2 grad {k}"))
            checked += 1
        assert checked >= 100, checked                 # fusion blocks + ELIC decoder taps (the estimator sits behind the argmax)
        print(f"[train parity] step-2 generator gradients through the updated D: {checked} tensors, worst relative error {worst:.6e}")
    finally:
        model.load_state_dict(sd_before)               # the fixture is shared: put the synthetic weights back
        for m in model.modules():
            if hasattr(m, "_plan"):
                m._plan = None
            if hasattr(m, "_qkv_plan"):
                m._qkv_plan = None
            if hasattr(m, "invalidate_caches"):
                m.invalidate_caches()


def test_training_steps_256_and_checkpoint(model, tmp_path):
    """BASELINE config 5's sample shape (256x256 crops), per-sample beta pairs drawn by the trainer: a few G + D steps run, every
    logged quantity is finite, the generator and discriminator weights move, the frozen sub-networks do not, the updated
    decoder is what the inference path then uses, and the model state dict round-trips through the reference's checkpoint
    format ({'iter', 'comp_model'}, model_saver.py:39-46)."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    D = _disc(7).to(DEV)
    tr = DualBetaCondGanDistortionVqCodeTrainer(model, D, seed=11)
    frozen0 = model.vq_model.decoder.conv_in.weight.detach().clone()
    enc0 = model.encoder.conv1.weight.detach().clone()
    w0 = model.fusion_module.fusion_modules["block_1_8"].scale[2].weight.detach().clone()
    d0 = D.main[0].weight.detach().clone()
    x = torch.rand((2, 3, 256, 256), generator=torch.Generator().manual_seed(91)) * 2 - 1
    logs = [tr.optimize_parameters(i, {"real_images": x}) for i in range(3)]
    for lg in logs:
        assert lg is not None and all(np.isfinite(v) for v in lg.values()), lg
        assert 0.0 <= lg["vq_acc"] <= 1.0 and lg["qbpp"] > 0
    assert torch.equal(model.vq_model.decoder.conv_in.weight, frozen0) and torch.equal(model.encoder.conv1.weight, enc0)
    assert not torch.equal(model.fusion_module.fusion_modules["block_1_8"].scale[2].weight, w0) and not torch.equal(D.main[0].weight, d0)
    # inference after training uses the updated weights (packed-weight caches were refreshed)
    model.codec_setup()
    r = model.compress(x[:1], 0)
    img, _, yh = model.decompress(r["string_list"])
    assert torch.equal(yh, r["y_hat"]) and img.shape == (1, 3, 256, 256)
    path = str(tmp_path / "comp_model_iter0000003.pth.tar")
    torch.save({"iter": 3, "comp_model": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}}, path)
    from dc_vic_amd import BaseConfig, build_comp_model
    m2 = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    m2.load_learned_weight(path)
    m2.codec_setup()
    r2 = m2.compress(x[:1], 0)
    assert r2["string_list"] == r["string_list"]
    img2, _, _ = m2.decompress(r2["string_list"])
    assert torch.equal(img2, img)


def test_training_step_invalidates_inference_graphs(model):
    """compress_batch / decompress_batch replay hipGraphs that hold the packed weights they were captured with; an optimizer step moves
    the decoder / estimator / fusion weights in place, so the trainer drops those graphs: inference right after a step equals the eager
    path on the NEW weights (and differs from the reconstruction before the step)."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    sd_before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        model.codec_setup()
        x = (torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(97)) * 2 - 1).to(DEV)
        model._graphs.clear()
        for _ in range(3):                                   # eager, capture, replay
            r = model.compress_batch(x, 0)
            rec0 = model.decompress_batch(r["string_lists"])[0].clone()
        assert {k[0] for k in model._graphs.entries} == {"enc", "dec"}, list(model._graphs.entries)
        tr = DualBetaCondGanDistortionVqCodeTrainer(model, _disc(5).to(DEV), lr_g=1e-3, lr_d=1e-4, clip_max_norm=None, seed=3)
        assert tr.optimize_parameters(0, dict(real_images=x.cpu(), beta_rate=torch.tensor([2.29, 2.29]), beta_vq=torch.tensor([3.0, 3.0]))) is not None
        assert len(model._graphs.entries) == 0
        rec1 = model.decompress_batch(r["string_lists"])[0].clone()
        model._graphs.disabled = True
        try:
            rec_eager = model.decompress_batch(r["string_lists"])[0]
        finally:
            model._graphs.disabled = False
        assert torch.equal(rec1, rec_eager)
        assert float((rec1 - rec0).abs().max()) > 1e-4      # the step really changed the decoder side
    finally:
        model.load_state_dict(sd_before)
        tr = None
