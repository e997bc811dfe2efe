"""The upsample-structured F(4x4, 3x3) convolution (csrc/wino44_ups.hip, route "wino44_ups") on a real MI355X against nearest x2 +
conv2d in fp64, its batch invariance, its GroupNorm statistics and its routing."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KERNEL = "conv3x3_wino44_ups_kernel(ConvKArgs)"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from dc_vic_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def plan_of(w, b, dev, f44="force"):
    from dc_vic_amd import ops
    p = ops.ConvPlan(w.to(dev), None if b is None else b.to(dev), "conv", pad=(1, 1), upsample=True)
    p.wino = "force"
    p.wino44 = f44
    return p


def run(plan, *args, **kw):
    from dc_vic_amd import ops
    ops.kernel_events_start()
    y = plan(*args, **kw)
    torch.cuda.synchronize()
    return y, list(ops.kernel_events_stop())


# (Cin, Cout, H, W low resolution, N, sources, residual, act): the decoder's Upsample layers it serves at batch 2 (256 @ 64^2 -> 128^2,
# 256 @ 128^2 -> 256^2; the 512-channel one at 32^2 -> 64^2 measured 1.8e-5 and stays on F(2x2): ops.WINO44_UPS_MAX_CIN), the
# 256-channel layer at 32^2, then ragged ones: one stage, odd stage counts, partial tiles in both directions (output
# 2H x 2W not a multiple of 16 x 32), Cout not a multiple of 64, a residual, ReLU / LeakyReLU, two sources, the persistent tile loop
CASES = [
    (256, 256, 32, 32, 2, None, False, 0), (256, 256, 64, 64, 2, None, False, 0), (256, 256, 128, 128, 2, None, False, 0),
    (8, 64, 4, 16, 1, None, False, 0), (24, 64, 7, 20, 2, None, True, 1), (40, 200, 13, 36, 3, None, False, 2),
    (64, 96, 9, 12, 2, [48, 16], True, 0), (136, 128, 33, 44, 1, None, True, 2), (256, 48, 16, 16, 5, None, False, 0)]


@pytest.mark.parametrize("case", CASES)
def test_wino44_ups_conv(dev, case):
    """dcvic_conv3x3_wino44_ups_f32 vs F.conv2d(F.interpolate(x, 2), w) in fp64: 1.2e-5 of the output's max, the bound of
    test_wino44_conv3x3; and the kernel that ran is the new one."""
    Cin, Cout, H, W, N, split, res, act = case
    x = rnd(N, Cin, H, W, seed=11)
    w = rnd(Cout, Cin, 3, 3, seed=12, scale=(Cin * 9) ** -0.5)
    b = rnd(Cout, seed=13, scale=0.1)
    r = rnd(N, Cout, 2 * H, 2 * W, seed=14) if res else None
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
    if act == 1:
        ref = torch.relu(ref)
    elif act == 2:
        ref = torch.where(ref > 0, ref, 0.2 * ref)
    if res:
        ref = ref + r.double()
    plan = plan_of(w, b, dev)
    xs = x.to(dev)
    srcs = xs if split is None else [t.contiguous() for t in torch.split(xs, split, dim=1)]
    y, ev = run(plan, srcs, act=act, res=None if r is None else r.to(dev))
    assert ev == [KERNEL], ev
    assert y.shape == ref.shape
    err = float((y.double().cpu() - ref).abs().max()) / float(ref.abs().max())
    assert err < 1.2e-5, err


def test_wino44_ups_batch_invariant_and_deterministic(dev):
    """An image alone, inside a batch and inside a batch large enough for the persistent workgroups to walk several tiles gives the same
    bits, and so do two runs."""
    x = rnd(9, 128, 24, 40, seed=21).to(dev)
    w = rnd(256, 128, 3, 3, seed=22, scale=(128 * 9) ** -0.5)
    b = rnd(256, seed=23)
    p = plan_of(w, b, dev)
    y9, y9b = p(x), p(x)
    y1 = p(x[3:4].contiguous())
    y64 = p(x.repeat(8, 1, 1, 1)[:64].contiguous())
    assert torch.equal(y9, y9b) and torch.equal(y9[3:4], y1) and torch.equal(y64[3:4], y1) and torch.equal(y64[9 + 3:9 + 4], y1)


def test_wino44_ups_groupnorm_statistics(dev):
    """The _stats variant writes per (image, channel, 16 x 32 output tile) the sum and the sum of squares of exactly the values it stores,
    in the layout of dcvic_conv3x3_wino44_stats_f32; checked against fp64 sums of the stored map (ragged: partial tiles, Cout not a
    multiple of 64, a residual), one ragged tile alone, and the GroupNorm fed by them against the two-pass GroupNorm (the bound of
    test_groupnorm_statistics_from_the_wino44_epilogue).  The map itself equals the one of the plain variant bit for bit."""
    from dc_vic_amd import ops
    N, Cin, Cout, H, W = 3, 64, 160, 20, 36                         # output 40 x 72: 3 x 3 tiles, the last row and column partial
    x = rnd(N, Cin, H, W, seed=31).to(dev)
    w = rnd(Cout, Cin, 3, 3, seed=32, scale=(Cin * 9) ** -0.5)
    b = rnd(Cout, seed=33, scale=0.5)
    r = rnd(N, Cout, 2 * H, 2 * W, seed=34).to(dev)
    plan = plan_of(w, b, dev)
    y, ev = run(plan, x, act=ops.ACT_LRELU02, res=r, gn_stats=True)
    assert ev == [KERNEL], ev
    part, n_pt = plan.last_gn_part
    assert n_pt == 3 * 3 and tuple(part.shape) == (N, Cout, n_pt, 2)
    assert torch.equal(y, plan(x, act=ops.ACT_LRELU02, res=r))
    assert plan.last_gn_part is None                                 # no statistics asked: nothing handed over
    yd = y.double()
    S = part[..., 0].double().sum(-1).cpu(); Q = part[..., 1].double().sum(-1).cpu()
    assert float((S - yd.sum((2, 3)).cpu()).abs().max()) < 1e-3 * float(yd.abs().sum((2, 3)).max()) * 1e-3
    assert float((Q - (yd * yd).sum((2, 3)).cpu()).abs().max()) < 1e-6 * float((yd * yd).sum((2, 3)).max())
    t = yd[:, :, 32:40, 64:72]                                        # tile 8: rows 32..39, columns 64..71
    assert float((part[:, :, 8, 0].double().cpu() - t.sum((2, 3)).cpu()).abs().max()) < 1e-4
    assert float((part[:, :, 8, 1].double().cpu() - (t * t).sum((2, 3)).cpu()).abs().max()) < 1e-4 * float((t * t).sum((2, 3)).max())
    g, be = (rnd(Cout, seed=35, scale=1.0) + 1.0).to(dev), rnd(Cout, seed=36, scale=0.3).to(dev)
    a = ops.groupnorm(y, g, be, 32, 1e-6, ops.ACT_SWISH)
    bq = ops.groupnorm(y, g, be, 32, 1e-6, ops.ACT_SWISH, part=(part, n_pt))
    assert float((a - bq).abs().max()) < 2e-6 * float(a.abs().max())


def test_wino44_ups_routing(dev):
    """Route "wino44_ups": only with the layer's wino44 flag, WINO44_ENABLED and an eligible output grid (a function of the layer and the
    image size, never of N); DCVIC_WINO44=0 (ops.WINO44_ENABLED) and layers without the flag keep the F(2x2) upsample kernel, the
    swish epilogue too."""
    from dc_vic_amd import ops
    w = rnd(128, 128, 3, 3, seed=41, scale=0.03)
    p44 = plan_of(w, None, dev, f44=True)
    p22 = plan_of(w, None, dev, f44=False)
    mk = lambda n, h, ww: [torch.empty((n, 128, h, ww), device=dev)]
    assert p44._wino44_ups_ok(mk(1, 64, 64), 64, 64) and p44._wino44_ups_ok(mk(32, 64, 64), 64, 64)
    assert p44._wino44_ups_ok(mk(1, 16, 16), 16, 16) == p44._wino44_ups_ok(mk(32, 16, 16), 16, 16)
    assert not p44._wino44_ups_ok(mk(1, 32, 30), 32, 30)               # width not a multiple of 4
    wide = plan_of(rnd(512, 512, 3, 3, seed=42, scale=0.01), None, dev, f44=True)
    assert not wide._wino44_ups_ok([torch.empty((1, 512, 32, 32), device=dev)], 32, 32)   # Cin > WINO44_UPS_MAX_CIN
    x = torch.zeros((1, 128, 64, 64), device=dev)
    assert run(p44, x)[1] == [KERNEL]
    assert run(p22, x)[1] == ["conv3x3_wino_ups_kernel(ConvKArgs)"]
    assert run(p44, x, act=ops.ACT_SWISH)[1] == ["conv3x3_wino_ups_kernel(ConvKArgs)"]
    old = ops.WINO44_ENABLED
    ops.WINO44_ENABLED = False
    try:
        assert run(p44, x)[1] == ["conv3x3_wino_ups_kernel(ConvKArgs)"]
    finally:
        ops.WINO44_ENABLED = old


def test_wino44_ups_in_the_decoder(dev):
    """The VQGAN decoder's Upsample layers run on the new kernel and hand their GroupNorm statistics to the next ResnetBlock's norm1:
    the decoder output equals (1e-5 of its max) the same decoder with the hand-off switched off (ops.GN_FUSED_STATS)."""
    from dc_vic_amd import ops
    from dc_vic_amd.vqgan import Decoder
    torch.manual_seed(0)
    dec = Decoder(ch=32, out_ch=3, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=(), in_channels=3, resolution=256,
                  z_channels=8).to(dev).eval()
    for p in dec.parameters():
        p.data.normal_(0.0, 0.05)
    z = torch.randn(2, 8, 64, 64, device=dev)                        # Upsample outputs 128^2 and 256^2: both eligible
    with torch.no_grad():
        ops.kernel_events_start()
        y = dec(z)
        torch.cuda.synchronize()
        ev = ops.kernel_events_stop()
        assert ev.get(KERNEL, {}).get("launches") == 2, list(ev)
        assert all(u.out_part is not None for u in (dec.up[1].upsample, dec.up[2].upsample))
        old = ops.GN_FUSED_STATS
        ops.GN_FUSED_STATS = False
        try:
            y2 = dec(z)
        finally:
            ops.GN_FUSED_STATS = old
    assert float((y - y2).abs().max()) < 1e-5 * float(y2.abs().max())
