"""Kernel-level parity on a real MI355X: every C-ABI compute entry point against the same operator
evaluated on the CPU (torch fp32 functional ops / the oracle's entropy formulas).  Tolerances are
written per test; integer outputs (indices, symbols, cdf indexes, bytes) are compared exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from dc_vic_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(a, b, rtol=1e-4, atol=1e-4):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


CONV_CASES = [
    # Cin, Cout, k, stride, pad, H, W, N
    (128, 128, 3, 1, 1, 40, 72, 2),     # cfg 0 (TC 128), ragged tiles
    (8, 256, 3, 1, 1, 16, 16, 1),       # two cout tiles
    (3, 192, 5, 2, 2, 64, 48, 2),       # ELIC conv1: Cin 3 (channel padding), cfg 3, 5x5 s2
    (192, 96, 1, 1, 0, 32, 32, 1),      # bottleneck 1x1, cfg 3
    (96, 96, 3, 1, 1, 17, 9, 3),        # odd sizes
    (192, 320, 3, 1, 1, 16, 16, 1),     # hyper encoder conv1 (3 cout tiles of 128)
    (320, 256, 5, 2, 2, 16, 16, 2),     # hyper encoder conv2
    (256, 192, 5, 2, 2, 8, 8, 2),       # -> 4x4 (tiny map, TW 4)
    (160, 224, 5, 1, 2, 16, 16, 2),     # CHARM 5x5 s1, tap groups, cfg 0 with Cout 224
    (128, 32, 3, 1, 1, 16, 16, 2),      # CHARM out, cfg 2
    (512, 4, 3, 1, 1, 32, 32, 1),       # conv_out -> 4 channels
    (4, 512, 3, 1, 1, 32, 32, 1),       # decoder conv_in: Cin 4
    (128, 3, 3, 1, 1, 64, 64, 1),       # final conv -> 3
    (64, 64, 3, 1, 1, 5, 3, 1),         # smaller than any tile
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d(dev, case):
    from dc_vic_amd import ops
    Cin, Cout, k, stride, pad, H, W, N = case
    x = rnd(N, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, k, k, seed=2, scale=(Cin * k * k) ** -0.5)
    b = rnd(Cout, seed=3, scale=0.1)
    ref = F.conv2d(x, w, b, stride=stride, padding=pad)
    plan = ops.ConvPlan(w.to(dev), b.to(dev), "conv", stride=stride, pad=(pad, pad))
    out = plan(x.to(dev))
    assert out.shape == ref.shape
    close(out, ref, rtol=2e-4, atol=2e-5)


def test_conv_epilogue_and_sources(dev):
    """bias -> act -> +res -> beta-FT affine; three concatenated sources with odd channel splits;
    output written into a channel slice of a larger buffer."""
    from dc_vic_amd import ops
    N, H, W = 2, 24, 40
    a, b_, c = rnd(N, 260, H, W, seed=4), rnd(N, 100, H, W, seed=5), rnd(N, 92, H, W, seed=6)
    w = rnd(192, 452, 3, 3, seed=7, scale=(452 * 9) ** -0.5)
    bias = rnd(192, seed=8, scale=0.1)
    res = rnd(N, 192, H, W, seed=9)
    sc, sh = rnd(N, 192, seed=10, scale=0.3), rnd(N, 192, seed=11, scale=0.3)
    ref = F.relu(F.conv2d(torch.cat([a, b_, c], 1), w, bias, padding=1)) + res
    ref = ref * (1 + sc[:, :, None, None]) + sh[:, :, None, None]
    big = torch.zeros(N, 300, H, W, device=dev)
    # sources as channel slices of bigger buffers (non-trivial batch strides)
    abuf = torch.zeros(N, 300, H, W, device=dev); abuf[:, 20:280] = a.to(dev)
    plan = ops.ConvPlan(w.to(dev), bias.to(dev), "conv", pad=(1, 1))
    plan([abuf[:, 20:280], b_.to(dev), c.to(dev)], out=big[:, 50:242], act=ops.ACT_RELU, res=res.to(dev),
         affine=(sc.to(dev).contiguous(), sh.to(dev).contiguous()))
    close(big[:, 50:242], ref, rtol=2e-4, atol=5e-5)
    assert float(big[:, :50].abs().max()) == 0.0 and float(big[:, 242:].abs().max()) == 0.0
    # shared (batch-1) affine vectors
    out2 = plan([abuf[:, 20:280], b_.to(dev), c.to(dev)], act=ops.ACT_NONE, affine=(sc[:1].to(dev).contiguous(), sh[:1].to(dev).contiguous()))
    ref2 = F.conv2d(torch.cat([a, b_, c], 1), w, bias, padding=1) * (1 + sc[:1, :, None, None]) + sh[:1, :, None, None]
    close(out2, ref2, rtol=2e-4, atol=5e-5)


@pytest.mark.parametrize("H,W", [(16, 16), (12, 20), (32, 64)])
def test_conv_upsample_fused(dev, H, W):
    """ldm Upsample: nearest x2 then conv3x3 (model.py:53-57), fused in the patch loader."""
    from dc_vic_amd import ops
    x = rnd(2, 64, H, W, seed=12)
    w = rnd(64, 64, 3, 3, seed=13, scale=(64 * 9) ** -0.5)
    b = rnd(64, seed=14, scale=0.1)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    out = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1), upsample=True)(x.to(dev))
    close(out, ref, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("H,W", [(32, 32), (17, 33), (64, 40)])
def test_conv_downsample_asym_pad(dev, H, W):
    """ldm Downsample: F.pad (0,1,0,1) then conv3x3 stride 2 pad 0 (model.py:72-76)."""
    from dc_vic_amd import ops
    x = rnd(2, 128, H, W, seed=15)
    w = rnd(128, 128, 3, 3, seed=16, scale=(128 * 9) ** -0.5)
    b = rnd(128, seed=17, scale=0.1)
    ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    out = ops.ConvPlan(w.to(dev), b.to(dev), "conv", stride=2, pad=(0, 0))(x.to(dev), out_hw=tuple(ref.shape[2:]))
    close(out, ref, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("Cin,Cout,k,H,W", [(192, 192, 5, 16, 16), (192, 256, 5, 4, 6), (256, 128, 3, 16, 24), (192, 192, 5, 9, 7)])
def test_conv_transpose(dev, Cin, Cout, k, H, W):
    """ConvTranspose2d(k5,s2,p2,op1) as four sub-pixel phases; (k3,s1,p1) as a flipped conv."""
    from dc_vic_amd import ops
    x = rnd(2, Cin, H, W, seed=18)
    w = rnd(Cin, Cout, k, k, seed=19, scale=(Cin * k * k / 4) ** -0.5)
    b = rnd(Cout, seed=20, scale=0.1)
    if k == 5:
        ref = F.conv_transpose2d(x, w, b, stride=2, padding=2, output_padding=1)
    else:
        ref = F.conv_transpose2d(x, w, b, stride=1, padding=1)
    out = ops.ConvPlan(w.to(dev), b.to(dev), "convT")(x.to(dev), act=ops.ACT_NONE)
    assert out.shape == ref.shape
    close(out, ref, rtol=2e-4, atol=2e-5)


def test_conv_batch_invariance(dev):
    """Bit-identical results for an image alone and inside a batch (encoder/decoder agreement)."""
    from dc_vic_amd import ops
    x = rnd(5, 160, 16, 16, seed=21).to(dev)
    w = rnd(224, 160, 5, 5, seed=22, scale=0.02).to(dev)
    plan = ops.ConvPlan(w, None, "conv", pad=(2, 2))
    full = plan(x)
    for i in (0, 3, 4):
        single = plan(x[i:i + 1].contiguous())
        assert torch.equal(single[0], full[i])


@pytest.mark.parametrize("C,H,W,act", [(128, 32, 32, 3), (704, 8, 12, 3), (256, 16, 16, 0), (96, 5, 7, 3)])
def test_groupnorm(dev, C, H, W, act):
    from dc_vic_amd import ops
    if C % 32:
        pytest.skip("32 groups")
    x = rnd(2, C, H, W, seed=23, scale=2.0) + 0.5
    g, b = 1 + 0.1 * rnd(C, seed=24), 0.1 * rnd(C, seed=25)
    ref = F.group_norm(x, 32, g, b, eps=1e-6)
    if act == 3:
        ref = ref * torch.sigmoid(ref)
    out = ops.groupnorm(x.to(dev), g.to(dev), b.to(dev), act=act)
    close(out, ref, rtol=1e-4, atol=1e-5)
    # channel-slice views in and out
    big = torch.zeros(2, C + 64, H, W, device=dev); big[:, 32:32 + C] = x.to(dev)
    o2 = torch.zeros(2, C + 10, H, W, device=dev)
    ops.groupnorm(big[:, 32:32 + C], g.to(dev), b.to(dev), act=act, out=o2[:, 10:])
    close(o2[:, 10:], ref, rtol=1e-4, atol=1e-5)


def test_layernorm_softmax_c(dev):
    from dc_vic_amd import ops
    x = rnd(2, 128, 12, 20, seed=26, scale=3.0)
    g, b = 1 + 0.1 * rnd(128, seed=27), 0.1 * rnd(128, seed=28)
    ref = F.layer_norm(x.permute(0, 2, 3, 1), (128,), g, b, eps=1e-5).permute(0, 3, 1, 2)
    close(ops.layernorm_c(x.to(dev), g.to(dev), b.to(dev)), ref, rtol=1e-4, atol=1e-5)
    s = rnd(3, 200, 77, seed=29, scale=4.0)
    out = ops.softmax_c_(s.to(dev).contiguous(), 3, 200, 77)
    close(out, F.softmax(s, dim=1), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("HW,C", [(256, 64), (150, 512)])
def test_attention_gemms(dev, HW, C):
    """AttnBlock score/value products (ldm model.py:186-196) through bgemm + softmax_c."""
    from dc_vic_amd import ops
    N = 2
    q, k, v = rnd(N, C, HW, seed=30), rnd(N, C, HW, seed=31), rnd(N, C, HW, seed=32)
    w_ = torch.bmm(q.permute(0, 2, 1), k) * (C ** -0.5)
    w_ = F.softmax(w_, dim=2)
    ref = torch.bmm(v, w_.permute(0, 2, 1))
    qkv = torch.cat([q, k, v], 1).to(dev).contiguous()       # [N, 3C, HW]
    qd, kd, vd = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    St = torch.empty(N, HW, HW, device=dev)
    bs = 3 * C * HW
    ops.bgemm(kd, (bs, 1, HW), qd, (bs, HW, 1), St, (HW * HW, HW), N, HW, HW, C, alpha=C ** -0.5)
    ops.softmax_c_(St, N, HW, HW)
    out = torch.empty(N, C, HW, device=dev)
    ops.bgemm(vd, (bs, HW, 1), St, (HW * HW, HW, 1), out, (C * HW, HW), N, C, HW, HW)
    close(out, ref, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("N,C,H,W", [(2, 512, 32, 32), (1, 512, 8, 16), (3, 256, 16, 16), (2, 128, 8, 8), (1, 512, 64, 96)])
def test_attention_fused(dev, N, C, H, W):
    """Fused single-head attention (csrc/attn.hip) vs the torch fp32 reference of ldm model.py:186-196.  Tolerance:
    fp32 re-association only (online softmax over 64-key tiles vs one softmax over the row): rtol 2e-4.  The result does
    not depend on the waves-per-workgroup variant nor on the batch an image travels in (bit-identical)."""
    from dc_vic_amd import ops
    HW = H * W
    q, k, v = 2.0 * rnd(N, C, HW, seed=35), 2.0 * rnd(N, C, HW, seed=36), rnd(N, C, HW, seed=37)
    w_ = torch.bmm(q.permute(0, 2, 1), k) * (C ** -0.5)
    w_ = F.softmax(w_, dim=2)
    ref = torch.bmm(v, w_.permute(0, 2, 1)).view(N, C, H, W)
    qkv = torch.cat([q, k, v], 1).view(N, 3 * C, H, W).to(dev).contiguous()
    out = ops.attn_fused(qkv, C)
    close(out, ref, rtol=2e-4, atol=2e-5)
    o2, o4 = ops.attn_fused(qkv, C, force_nw=2), ops.attn_fused(qkv, C, force_nw=4)
    assert torch.equal(o2, o4) and torch.equal(out, o4)
    one = ops.attn_fused(qkv[N - 1:N].contiguous(), C)
    assert torch.equal(one[0], out[N - 1])
    # the materialised-score path (bgemm + softmax + bgemm) agrees to fp32 slack
    from dc_vic_amd.vqgan import AttnBlock
    close(AttnBlock._attn_unfused(qkv, N, C, H, W), out, rtol=2e-4, atol=2e-5)
    with pytest.raises(Exception):
        ops.attn_fused(torch.zeros(1, 3 * 512, 5, 8, device=dev), 512)          # HW % 64 != 0 -> EINVAL, no launch


@pytest.mark.parametrize("n_e", [256, 1024, 16384])
def test_vq_sharded_codebook_mfma(dev, n_e, monkeypatch):
    """Sharded-codebook search (256-code shards through LDS, fp32 MFMA 16x16x4 dots with K = the code dimension, wavefront
    shuffle (d, idx) reduction): indices identical to the one-LDS-image kernel where that one applies, and -- at
    16 384 x 4, which fits no LDS image -- index-exact vs the oracle's VectorQuantizer2 restatement (quantize.py:271-312)
    up to expanded-form fp32 near-ties, itemised.  Includes a ragged pixel count and exact duplicate codes (first wins)."""
    from dc_vic_amd import ops
    from oracle import dcvic_oracle as O
    g = torch.Generator().manual_seed(60 + n_e % 7)
    cb = (torch.rand((n_e, 4), generator=g) * 2 - 1) / n_e
    cb[n_e // 2 + 3] = cb[5]                       # duplicate code: the first (index 5) must win every tie
    z = torch.randn((2, 4, 23, 41), generator=g) * (0.6 / n_e)
    z[0, :, 0, 0] = cb[5]                          # exact hit on the duplicated code
    zd, cbd = z.to(dev).contiguous(), cb.to(dev).contiguous()
    monkeypatch.setenv("DCVIC_VQ_KERNEL", "shard")
    idx_s, zq_s, _ = ops.vq_argmin(zd, cbd, want_zq=True)
    monkeypatch.delenv("DCVIC_VQ_KERNEL")
    assert int(idx_s[0, 0, 0]) == 5
    zq_o, idx_o = O.vq_quantize({"vq_model.quantize.embedding.weight": cb}, z)
    mism = (idx_s.cpu() != idx_o).nonzero()
    zf = z.permute(0, 2, 3, 1).double()
    for nn, y, x in mism.tolist():                 # a disagreement must be a near-tie of the expanded-form distance
        a, b = int(idx_s[nn, y, x]), int(idx_o[nn, y, x])
        da, db = ((zf[nn, y, x] - cb[a].double()) ** 2).sum(), ((zf[nn, y, x] - cb[b].double()) ** 2).sum()
        assert abs(float(da - db)) <= 4e-7 * float((zf[nn, y, x] ** 2).sum() + (cb[b].double() ** 2).sum()), (a, b, float(da - db))
    assert len(mism) <= 2
    ok = (idx_s.cpu() == idx_o)
    assert torch.equal(zq_s.cpu().permute(0, 2, 3, 1)[ok], zq_o.permute(0, 2, 3, 1)[ok])
    if n_e <= 1024:                                # same roundings as the other kernels: identical indices, always
        monkeypatch.setenv("DCVIC_VQ_KERNEL", "lds")
        idx_l, _, _ = ops.vq_argmin(zd, cbd, want_zq=False)
        monkeypatch.delenv("DCVIC_VQ_KERNEL")
        idx_d, _, _ = ops.vq_argmin(zd, cbd, want_zq=False)        # default (scalar-cache packed-fp32 kernel)
        assert torch.equal(idx_s, idx_l) and torch.equal(idx_s, idx_d)
        _, _, feat = ops.vq_argmin(zd, cbd, want_zq=False, want_feat=True)
        monkeypatch.setenv("DCVIC_VQ_KERNEL", "shard")
        _, _, feat_s = ops.vq_argmin(zd, cbd, want_zq=False, want_feat=True)
        assert torch.equal(feat, feat_s)


def test_device_mismatch_raises(dev, monkeypatch):
    """Kernels launch on the current device's stream: a tensor of another GPU must raise, not launch."""
    from dc_vic_amd import ops
    x = torch.zeros(1, 4, 8, 8, device=dev)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    with pytest.raises(ValueError, match="set_device"):
        ops.activation(x, ops.ACT_RELU)


@pytest.mark.parametrize("H,W,shift", [(16, 16, 0), (16, 16, 4), (8, 24, 4), (32, 32, 4)])
def test_swin_window_attention(dev, H, W, shift):
    from dc_vic_amd import ops
    from oracle import dcvic_oracle as O
    N, C, heads, ws = 2, 128, 8, 8
    qkv = rnd(N, 3 * C, H, W, seed=33)
    table = 0.5 * rnd(225, heads, seed=34)
    # reference: the window-attention part of SwinTransformerBlock on the [B, L, 3C] token view
    t = qkv.flatten(2).transpose(1, 2).view(N, H, W, 3 * C)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    xw = t.view(N, H // ws, ws, W // ws, ws, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, 3 * C)
    B_ = xw.shape[0]
    r = xw.reshape(B_, 64, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = r[0] * 0.25, r[1], r[2]
    attn = q @ k.transpose(-2, -1) + table[O._rel_pos_index(ws).view(-1)].view(64, 64, -1).permute(2, 0, 1).unsqueeze(0)
    if shift:
        mask = O._shift_mask(H, W, ws, shift)
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, 64, 64) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, 64, 64)
    o = (F.softmax(attn, -1) @ v).transpose(1, 2).reshape(B_, 64, C)
    o = o.view(N, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, C)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    ref = o.permute(0, 3, 1, 2)
    out = ops.swin_attn(qkv.to(dev), table.to(dev), heads, ws, shift)
    close(out, ref, rtol=1e-4, atol=1e-5)


def test_elementwise(dev):
    from dc_vic_amd import ops
    a, b, c = rnd(2, 48, 9, 11, seed=35), rnd(2, 48, 9, 11, seed=36), rnd(2, 48, 9, 11, seed=37)
    A, B, Cc = a.to(dev), b.to(dev), c.to(dev)
    close(ops.add(A, B), a + b, rtol=0, atol=0)
    close(ops.add_mul_sigmoid(A, B, Cc), a + b * torch.sigmoid(c), rtol=1e-6, atol=1e-6)
    close(ops.sft(A, B, Cc, w=1.0), a + 1.0 * (a * b + c), rtol=1e-6, atol=1e-6)
    close(ops.activation(A, ops.ACT_GELU), F.gelu(a), rtol=1e-5, atol=1e-6)
    close(ops.activation(A, ops.ACT_HALF_TANH), 0.5 * torch.tanh(a), rtol=1e-5, atol=1e-6)
    close(ops.activation(A, ops.ACT_LRELU02), F.leaky_relu(a, 0.2), rtol=0, atol=0)
    sc, sh = rnd(2, 48, seed=38), rnd(2, 48, seed=39)
    close(ops.chan_affine(A, sc.to(dev), sh.to(dev), add_=B), a * (1 + sc[:, :, None, None]) + sh[:, :, None, None] + b, rtol=1e-6, atol=1e-6)
    x = rnd(2, 3, 50, 70, seed=40)
    close(ops.pad_reflect(x.to(dev), 14, 58), F.pad(x, (0, 58, 0, 14), mode="reflect"), rtol=0, atol=0)
    y, y8 = ops.crop_clamp((x * 1.5).to(dev), 33, 41, want_u8=True)
    refc = (x * 1.5)[:, :, :33, :41].clamp(-1, 1)
    close(y, refc, rtol=0, atol=0)
    ref8 = ((refc + 1.0) / 2.0 * 255.0).numpy().transpose(0, 2, 3, 1).astype(np.uint8)
    assert np.array_equal(y8.cpu().numpy(), ref8)


def test_vq_argmin_index_exact(dev, synth_sd):
    """Index-exact against the oracle's restatement of VectorQuantizer2 on two clouds (reference-init
    codebook U(+-1/256)); disagreements, if any, must be fp32 near-ties and are itemised."""
    from dc_vic_amd import ops
    from oracle import dcvic_oracle as O
    cb_full = synth_sd["vq_model.quantize.embedding.weight"]
    for seed, scale, shape, n_e in ((41, 1.0, (2, 4, 64, 64), 256), (42, 0.01, (3, 4, 24, 40), 256),
                                    (43, 3.0, (1, 4, 7, 5), 256), (49, 0.02, (2, 4, 33, 31), 255),
                                    (50, 0.01, (1, 4, 16, 40), 1)):
        cb = cb_full[:n_e].contiguous()       # n_e = 255 and 1 are no multiple of 8: they go to the generic LDS kernel, 256 to the packed one
        z = rnd(*shape, seed=seed, scale=scale)
        zq_ref, idx_ref = O.vq_quantize({"vq_model.quantize.embedding.weight": cb}, z)
        idx, zq, feat = ops.vq_argmin(z.to(dev), cb.to(dev), want_zq=True, want_feat=True)
        idx_c = idx.cpu()
        mism = (idx_c != idx_ref)
        if mism.any():
            # itemise: both candidates must be within 2 ulp of the minimum distance
            zf = z.permute(0, 2, 3, 1).reshape(-1, 4).double()
            d = (zf ** 2).sum(1, keepdim=True) + (cb.double() ** 2).sum(1) - 2 * zf @ cb.double().t()
            m = mism.reshape(-1)
            gap = (d[m, idx_c.reshape(-1)[m]] - d[m, idx_ref.reshape(-1)[m]]).abs()
            assert float(gap.max()) < 1e-6 * float(d.abs().max()), "VQ mismatch that is not a near-tie"
        assert mism.float().mean() < 1e-3
        ok = ~mism
        assert torch.equal(zq.cpu().permute(0, 2, 3, 1)[ok], zq_ref.permute(0, 2, 3, 1)[ok])
        ref_feat = O.onehot_feat({}, zq.cpu(), idx_c, n_embed=n_e)
        assert torch.equal(feat.cpu(), ref_feat)


def test_argmax_lut(dev, synth_sd):
    from dc_vic_amd import ops
    from oracle import dcvic_oracle as O
    logits = rnd(2, 256, 12, 20, seed=44)
    logits[0, 7, 3, 3] = logits[0, 200, 3, 3] = 50.0     # tie -> first maximum
    idx, lat = ops.argmax_lut(logits.to(dev), synth_sd["vq_model.quantize.embedding.weight"].to(dev),
                              synth_sd["vq_model.post_quant_conv.weight"].to(dev).contiguous(),
                              synth_sd["vq_model.post_quant_conv.bias"].to(dev))
    ref_idx = torch.argmax(logits, 1)
    assert torch.equal(idx.cpu(), ref_idx) and int(idx[0, 3, 3]) == 7
    ref_lat = O._conv(synth_sd, "vq_model.post_quant_conv", O.vq_indices_to_latent(synth_sd, ref_idx))
    close(lat, ref_lat, rtol=1e-5, atol=1e-8)


def test_gaussian_rate(dev):
    """Symbols / cdf indexes exact, y_hat exact, likelihood and bits within fp32 erfc tolerance."""
    from dc_vic_amd import ops
    from oracle import entropy_oracle as eo
    N, C, H, W = 3, 32, 16, 16
    y = rnd(N, C, H, W, seed=45, scale=3.0)
    mu = rnd(N, C, H, W, seed=46)
    sigma = rnd(N, C, H, W, seed=47, scale=2.0).abs() * torch.exp(rnd(N, C, H, W, seed=48))
    sigma[0, 0, 0, :8] = torch.tensor([0.0, 0.05, 0.11, 0.110001, 255.9, 256.0, 300.0, 1e4])
    table = eo.get_scale_table()
    sym_ref = torch.round(y - mu)
    yh_ref = sym_ref + mu
    lik_ref = eo.gc_likelihood(yh_ref, sigma, mu)
    idx_ref = eo.gc_build_indexes(sigma)
    yh = torch.empty(N, C, H, W, device=dev)
    sym = torch.empty(N, C, H, W, dtype=torch.int32, device=dev)
    ix = torch.empty(N, C, H, W, dtype=torch.int32, device=dev)
    lik = torch.empty(N, C, H, W, device=dev)
    bits = torch.zeros(N, device=dev)
    ops.gaussian_rate(y.to(dev), None, mu.to(dev), sigma.to(dev), table.to(dev), yh, sym, ix, lik, bits)
    assert torch.equal(sym.cpu(), sym_ref.int())
    assert torch.equal(ix.cpu(), idx_ref)
    assert torch.equal(yh.cpu(), yh_ref)
    # p = Phi(a) - Phi(b) cancels: the absolute error is a few ulp of Phi (~6e-8), whatever p is
    close(lik, lik_ref, rtol=2e-4, atol=3e-7)
    bits_ref = -(torch.log(lik_ref).reshape(N, -1).double().sum(1)) / np.log(2)
    close(bits, bits_ref, rtol=2e-4, atol=1e-2)
    # decode mode reproduces y_hat bit-exactly from the symbols
    yh2 = torch.empty(N, C, H, W, device=dev)
    ops.gaussian_rate(None, sym, mu.to(dev), sigma.to(dev), table.to(dev), yh2, None, None, None, None)
    assert torch.equal(yh2, yh)


def test_eb_rate(dev, synth_sd):
    from dc_vic_amd import ops
    from dc_vic_amd.entropy import pack_entropy_bottleneck
    from oracle import entropy_oracle as eo
    eb = eo.EntropyBottleneckOracle(synth_sd, "entropy_model_z")
    z = rnd(2, 192, 4, 6, seed=49, scale=4.0)
    zh_ref, lik_ref = eb.forward(z)
    packs = pack_entropy_bottleneck({k: v.to(dev) for k, v in synth_sd.items() if k.startswith("entropy_model_z.")}, "entropy_model_z")
    zh = torch.empty(2, 192, 4, 6, device=dev)
    sym = torch.empty(2, 192, 4, 6, dtype=torch.int32, device=dev)
    lik = torch.empty(2, 192, 4, 6, device=dev)
    bits = torch.zeros(2, device=dev)
    ops.eb_rate(z.to(dev), packs, zh, sym, lik, bits)
    assert torch.equal(zh.cpu(), zh_ref)
    assert torch.equal(sym.cpu(), eb.symbols(z))
    close(lik, lik_ref, rtol=2e-4, atol=3e-7)
    close(bits, -(torch.log(lik_ref).reshape(2, -1).double().sum(1)) / np.log(2), rtol=2e-4, atol=1e-2)


def test_conv_variants_bit_identical(dev, monkeypatch):
    """The LDS-DMA 3x3 kernel, the generic kernel and every tile variant picked for different batch sizes give
    bit-identical outputs (one reduction order per layer) -- the batch an image travels in never changes it."""
    import subprocess, sys, os
    from dc_vic_amd import ops
    x = rnd(12, 256, 64, 64, seed=50).to(dev)
    w = rnd(256, 256, 3, 3, seed=51, scale=0.02).to(dev)
    b = rnd(256, seed=52, scale=0.1).to(dev)
    plan = ops.ConvPlan(w, b, "conv", pad=(1, 1))
    full = plan(x)                                   # N=12 @64x64 -> enough workgroups for the DMA kernel
    one = plan(x[5:6].contiguous())                  # N=1 -> a small-tile generic variant
    assert torch.equal(one[0], full[5])
    two = plan(x[4:6].contiguous())
    assert torch.equal(two[1], full[5])
    # forced generic kernel in a child process (the switch is read once per process)
    code = ("import torch,sys;sys.path.insert(0,%r);from dc_vic_amd import ops;"
            "g=torch.Generator().manual_seed(50);x=torch.randn(12,256,64,64,generator=g).cuda();"
            "g=torch.Generator().manual_seed(51);w=(torch.randn(256,256,3,3,generator=g)*0.02).cuda();"
            "g=torch.Generator().manual_seed(52);b=(torch.randn(256,generator=g)*0.1).cuda();"
            "o=ops.ConvPlan(w,b,'conv',pad=(1,1))(x);torch.save(o.cpu(),sys.argv[1])") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "o.pt")
        env = dict(os.environ, DCVIC_CONV_DMA="0")
        subprocess.check_call([sys.executable, "-c", code, p], env=env)
        gen = torch.load(p)
    assert torch.equal(gen, full.cpu())


def test_conv_async_twin_bit_identical(dev):
    """conv_async.hip (LDS-DMA double-buffered twin used for small grids) against conv_mfma_kernel on every layer
    geometry it can meet: 5x5, the 3x3 order family, multi-chunk 1x1 stages, stride 2, transposed-conv phases,
    ragged channels, several sources, init accumulators, residual + affine epilogue.  Bit-identical."""
    from dc_vic_amd import ops
    from dc_vic_amd._lib import lib
    L = lib()
    cases = [  # (Cin list, Cout, k, stride, kind, H, W, N)
        ([224], 128, 5, 1, "conv", 16, 16, 4),
        ([128], 32, 3, 1, "conv", 16, 16, 4),
        ([96], 96, 3, 1, "conv", 16, 16, 3),
        ([192], 96, 1, 1, "conv", 16, 16, 4),
        ([320], 256, 5, 2, "conv", 16, 16, 2),
        ([192], 192, 5, 2, "convT", 4, 4, 3),
        ([192], 256, 3, 1, "convT", 8, 8, 2),
        ([128, 32, 64], 224, 5, 1, "conv", 16, 16, 2),
        ([100], 77, 3, 1, "conv", 13, 11, 2),
        ([512], 128, 1, 1, "conv", 32, 32, 1),
        ([3], 192, 5, 2, "conv", 32, 32, 1),
    ]
    try:
        for ci, (cins, cout, k, stride, kind, H, W, N) in enumerate(cases):
            cin = sum(cins)
            srcs = [rnd(N, c, H, W, seed=900 + 10 * ci + j).to(dev) for j, c in enumerate(cins)]
            wshape = (cin, cout, k, k) if kind == "convT" else (cout, cin, k, k)
            w = rnd(*wshape, seed=950 + ci, scale=(cin * k * k) ** -0.5).to(dev)
            b = rnd(cout, seed=960 + ci, scale=0.1).to(dev)
            plan = ops.ConvPlan(w, b, kind, stride=stride, pad=(k // 2, k // 2))
            outs = {}
            for mode, (use_async, fill) in {"generic": (0, 2), "async": (1, 1 << 20), "async32": (2, 1 << 20)}.items():
                L.dcvic_conv_set_tuning(-1, use_async, fill)
                y0 = plan(srcs)
                v0 = int(L.dcvic_conv_last_variant())
                res = rnd(*y0.shape, seed=970 + ci).to(dev)
                aff = (rnd(N, cout, seed=980 + ci, scale=0.2).to(dev), rnd(N, cout, seed=990 + ci, scale=0.2).to(dev))
                y1 = plan(srcs, act=ops.ACT_RELU, res=res, affine=aff)
                y2 = plan(srcs, init=y0, use_bias=False) if kind == "conv" else y0
                outs[mode] = (y0, y1, y2, v0)
            assert outs["async"][3] >= 8000 and outs["async"][3] < 9000, (ci, outs["async"][3])
            assert outs["generic"][3] < 8000 or outs["generic"][3] == 9000, (ci, outs["generic"][3])
            assert 8000 <= outs["async32"][3] < 8500, (ci, outs["async32"][3])
            for mode in ("async", "async32"):
                for a_, g_ in zip(outs[mode][:3], outs["generic"][:3]):
                    assert torch.equal(a_, g_), f"case {ci}: {mode} twin differs from the generic kernel"
    finally:
        L.dcvic_conv_set_tuning(-1, 1, 2)


def test_conv1x1_dma_bit_identical(dev):
    """conv1x1_dma_kernel (flat-pixel DMA-pipelined GEMM) against the generic kernel: all three channel-tile classes,
    odd chunk counts, channels not a multiple of 8, several sources, ragged plane (H*W % 256 != 0), residual +
    affine epilogue, and the ineligible case (H*W % 4 != 0) falling back."""
    from dc_vic_amd import ops
    from dc_vic_amd._lib import lib
    L = lib()
    cases = [  # (Cin list, Cout, H, W, N, expect_dma)
        ([512], 1536, 32, 32, 8, True),
        ([96], 192, 64, 64, 10, True),
        ([192], 96, 64, 64, 20, True),
        ([200], 128, 36, 52, 36, True),          # 25 chunks (odd), ragged plane 1872 = 7.3 tiles
        ([128, 64, 60], 64, 40, 40, 40, True),   # three sources, Cin 252 not a multiple of 8, class 1
        ([64], 128, 15, 15, 40, False),          # H*W = 225 not a multiple of 4 -> generic
    ]
    try:
        for ci, (cins, cout, H, W, N, expect) in enumerate(cases):
            cin = sum(cins)
            srcs = [rnd(N, c, H, W, seed=1200 + 10 * ci + j).to(dev) for j, c in enumerate(cins)]
            w = rnd(cout, cin, 1, 1, seed=1250 + ci, scale=cin ** -0.5).to(dev)
            b = rnd(cout, seed=1260 + ci, scale=0.1).to(dev)
            plan = ops.ConvPlan(w, b, "conv")
            res = rnd(N, cout, H, W, seed=1270 + ci).to(dev)
            aff = (rnd(N, cout, seed=1280 + ci, scale=0.2).to(dev), rnd(N, cout, seed=1290 + ci, scale=0.2).to(dev))
            outs = {}
            for mode, use_dma in (("generic", 0), ("dma", 1)):
                L.dcvic_conv_set_tuning(use_dma, 0, -1)
                y0 = plan(srcs)
                v0 = int(L.dcvic_conv_last_variant())
                y1 = plan(srcs, act=ops.ACT_GELU, res=res, affine=aff)
                outs[mode] = (y0, y1, v0)
            assert (7000 <= outs["dma"][2] < 8000) == expect, (ci, outs["dma"][2])
            assert outs["generic"][2] < 7000, (ci, outs["generic"][2])
            assert torch.equal(outs["dma"][0], outs["generic"][0]), f"case {ci}"
            assert torch.equal(outs["dma"][1], outs["generic"][1]), f"case {ci} (epilogue)"
            ref = torch.nn.functional.conv2d(torch.cat(srcs, 1).cpu(), w.cpu(), b.cpu())
            close(outs["dma"][0], ref, rtol=2e-5, atol=2e-5)
    finally:
        L.dcvic_conv_set_tuning(1, 1, 2)


def test_conv_upsample_phases_dma_bit_identical(dev):
    """nearest-x2 upsample + conv3x3 runs as four 2x2 sub-pixel phases; with enough work they go to the DMA tap kernel
    (<2,2,8>).  Same values as the generic kernel, and close to torch's upsample + conv."""
    from dc_vic_amd import ops
    from dc_vic_amd._lib import lib
    L = lib()
    x = rnd(24, 128, 64, 64, seed=1300).to(dev)
    w = rnd(128, 128, 3, 3, seed=1301, scale=0.03).to(dev)
    b = rnd(128, seed=1302, scale=0.1).to(dev)
    plan = ops.ConvPlan(w, b, "conv", pad=(1, 1), upsample=True)
    try:
        L.dcvic_conv_set_tuning(0, 0, -1)
        gen = plan(x)
        vg = int(L.dcvic_conv_last_variant())
        L.dcvic_conv_set_tuning(1, 0, -1)
        dma = plan(x)
        vd = int(L.dcvic_conv_last_variant())
    finally:
        L.dcvic_conv_set_tuning(1, 1, 2)
    assert vd == 9001 and vg < 7000, (vd, vg)
    assert torch.equal(gen, dma)
    ref = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x.cpu(), scale_factor=2.0, mode="nearest"), w.cpu(), b.cpu(), padding=1)
    close(dma, ref, rtol=1e-4, atol=1e-4)


def test_conv3x3_dma_epilogues_bit_identical(dev):
    """The DMA tap kernel's epilogue against the generic kernel's: bias / activation / residual / affine combinations
    (each its own compile-time path), partial tiles (W = 36, W = 34) and a channel-offset output view."""
    from dc_vic_amd import ops
    from dc_vic_amd._lib import lib
    L = lib()
    try:
        for ci, (H, W, N) in enumerate(((64, 64, 24), (40, 36, 40), (40, 34, 40))):
            C = 128
            x = rnd(N, C, H, W, seed=1400 + ci).to(dev)
            w = rnd(C, C, 3, 3, seed=1410 + ci, scale=0.03).to(dev)
            b = rnd(C, seed=1420 + ci, scale=0.1).to(dev)
            res = rnd(N, C, H, W, seed=1430 + ci).to(dev)
            aff = (rnd(N, C, seed=1440 + ci, scale=0.2).to(dev), rnd(N, C, seed=1450 + ci, scale=0.2).to(dev))
            plan = ops.ConvPlan(w, b, "conv", pad=(1, 1))
            big = torch.empty((N, C + 1, H, W), device=dev)                    # channel-offset view: misaligned unless H*W % 4 == 0
            outs = {}
            for mode, use_dma in (("generic", 0), ("dma", 1)):
                L.dcvic_conv_set_tuning(use_dma, 0, -1)
                y0 = plan(x)
                v0 = int(L.dcvic_conv_last_variant())
                y1 = plan(x, act=ops.ACT_SWISH, res=res)
                y2 = plan(x, act=ops.ACT_RELU, res=res, affine=aff)
                y3 = plan(x, affine=aff, use_bias=False)
                y4 = plan(x, out=big[:, 1:], res=res).clone()
                outs[mode] = (y0, y1, y2, y3, y4, v0)
            assert outs["dma"][5] == 9000 and outs["generic"][5] < 7000, (ci, outs["dma"][5], outs["generic"][5])
            for k in range(5):
                assert torch.equal(outs["dma"][k], outs["generic"][k]), f"case {ci} output {k}"
    finally:
        L.dcvic_conv_set_tuning(1, 1, 2)


def test_bgemm_tile_sizes_bit_identical(dev):
    """The batched GEMM picks 64x64 tiles when 128x128 ones would leave CUs idle (small batch); an item computed alone
    (64-tiles) equals the same item inside a large batch (128-tiles) bit for bit, ragged sizes included."""
    from dc_vic_amd import ops
    Nb, M, Nn, K = 72, 200, 330, 96
    A = rnd(Nb, M, K, seed=1500).to(dev); B = rnd(Nb, K, Nn, seed=1501).to(dev)
    big = torch.empty(Nb, M, Nn, device=dev)
    ops.bgemm(A, (M * K, K, 1), B, (K * Nn, Nn, 1), big, (M * Nn, Nn), Nb, M, Nn, K, alpha=0.37)
    one = torch.empty(1, M, Nn, device=dev)
    ops.bgemm(A[5:6].contiguous(), (M * K, K, 1), B[5:6].contiguous(), (K * Nn, Nn, 1), one, (M * Nn, Nn), 1, M, Nn, K, alpha=0.37)
    assert torch.equal(one[0], big[5])
    close(big, 0.37 * torch.bmm(A.cpu(), B.cpu()), rtol=1e-4, atol=1e-4)


def test_conv_dispatch_fuzz_bit_identical(dev):
    """Random layer geometries through the full dispatcher (DMA tap / 1x1 kernels, async twins, small tiles) against the
    generic kernel alone: bit-identical; and against torch's conv2d within fp32 re-association tolerance."""
    from dc_vic_amd import ops
    from dc_vic_amd._lib import lib
    L = lib()
    rs = np.random.RandomState(20261004)
    seen = set()
    try:
        for it in range(48):
            k = int(rs.choice([1, 1, 3, 3, 3, 5]))
            stride = int(rs.choice([1, 1, 1, 2])) if k > 1 else 1
            cin = int(rs.choice([3, 8, 24, 96, 100, 128, 192, 256, 320]))
            cout = int(rs.choice([3, 32, 64, 96, 128, 192, 256]))
            H = int(rs.choice([4, 8, 13, 16, 32, 40, 64])); W = int(rs.choice([4, 8, 12, 16, 32, 36, 64]))
            N = int(rs.choice([1, 2, 5, 16, 33]))
            if N * cin * H * W > 24e6 or N * cout * H * W > 24e6:
                N = max(1, int(24e6 // (max(cin, cout) * H * W)))
            nsplit = int(rs.choice([1, 1, 2, 3])) if cin >= 24 and cin % 8 == 0 else 1
            cuts = sorted(rs.choice(np.arange(8, cin, 8), size=nsplit - 1, replace=False).tolist()) if nsplit > 1 else []
            parts = [b - a for a, b in zip([0] + cuts, cuts + [cin])]
            srcs = [rnd(N, c, H, W, seed=5000 + 7 * it + j).to(dev) for j, c in enumerate(parts)]
            w = rnd(cout, cin, k, k, seed=6000 + it, scale=(cin * k * k) ** -0.5).to(dev)
            b = rnd(cout, seed=7000 + it, scale=0.1).to(dev)
            plan = ops.ConvPlan(w, b, "conv", stride=stride, pad=(k // 2, k // 2))
            with_res = bool(rs.randint(2))
            outs = {}
            for mode, (dma, asy) in (("generic", (0, 0)), ("full", (1, 1))):
                L.dcvic_conv_set_tuning(dma, asy, 2)
                y = plan(srcs)
                res = rnd(*y.shape, seed=8000 + it).to(dev) if with_res else None
                y2 = plan(srcs, act=ops.ACT_LRELU02, res=res)
                outs[mode] = (y, y2, int(L.dcvic_conv_last_variant()))
            seen.add(outs["full"][2] // 100)
            assert torch.equal(outs["full"][0], outs["generic"][0]) and torch.equal(outs["full"][1], outs["generic"][1]), \
                (it, k, stride, parts, cout, H, W, N, outs["full"][2], outs["generic"][2])
            ref = F.conv2d(torch.cat(srcs, 1).cpu(), w.cpu(), b.cpu(), stride=stride, padding=k // 2)
            close(outs["full"][0], ref, rtol=2e-4, atol=2e-4)
    finally:
        L.dcvic_conv_set_tuning(1, 1, 2)
    assert len(seen) >= 4, f"the fuzz run should reach several kernel families, got variant groups {sorted(seen)}"


def test_conv3x3_dma_96_channel_tiles_bit_identical(dev):
    """The DMA tap kernel's 96-channel-tile build (ELIC 96 / 192-channel 3x3 layers) against the generic kernel."""
    from dc_vic_amd import ops
    from dc_vic_amd._lib import lib
    L = lib()
    try:
        for ci, (cin, cout, H, W, N) in enumerate(((96, 96, 64, 64, 24), (192, 192, 48, 40, 16), (96, 192, 64, 64, 12))):
            x = rnd(N, cin, H, W, seed=1600 + ci).to(dev)
            w = rnd(cout, cin, 3, 3, seed=1610 + ci, scale=0.03).to(dev)
            b = rnd(cout, seed=1620 + ci, scale=0.1).to(dev)
            res = rnd(N, cout, H, W, seed=1630 + ci).to(dev)
            plan = ops.ConvPlan(w, b, "conv", pad=(1, 1))
            outs = {}
            for mode, use_dma in (("generic", 0), ("dma", 1)):
                L.dcvic_conv_set_tuning(use_dma, 0, -1)
                y0 = plan(x, act=ops.ACT_RELU)
                v0 = int(L.dcvic_conv_last_variant())
                y1 = plan(x, res=res)
                outs[mode] = (y0, y1, v0)
            assert outs["dma"][2] == 9003 and outs["generic"][2] < 7000, (ci, outs["dma"][2], outs["generic"][2])
            assert torch.equal(outs["dma"][0], outs["generic"][0]) and torch.equal(outs["dma"][1], outs["generic"][1]), f"case {ci}"
    finally:
        L.dcvic_conv_set_tuning(1, 1, 2)


# ------------------------------------------------------------------------------------------- Winograd F(2x2, 3x3)
WINO_CASES = [
    # Cin, Cout, H, W, N, n_src split, residual, act
    (8, 64, 8, 32, 1, None, False, 0),            # exactly one workgroup tile, one stage
    (16, 64, 10, 28, 2, None, False, 0),          # ragged tile, rows / columns masked
    (64, 128, 33, 72, 2, None, True, 3),          # odd height, residual + swish, three column tiles
    (128, 192, 64, 64, 2, None, True, 0),         # three 64-channel tiles
    (256, 96, 40, 48, 1, [192, 64], False, 2),    # two sources (virtual concat), Cout not a multiple of 64
    (704, 512, 32, 32, 2, [192, 512], False, 0),  # the 1/8-level fusion block: cat[cond 192, dec 512] -> 512
    (128, 128, 256, 256, 2, None, True, 0),       # the 256^2 decoder layer: more tiles than workgroups (persistent loop)
]


@pytest.mark.parametrize("case", WINO_CASES)
def test_wino_conv3x3(dev, case):
    """dcvic_conv3x3_wino_f32 vs torch conv2d evaluated in fp64.  Winograd re-associates the sum, so the comparison is a
    tolerance: 2e-6 of the output's max -- 4x the largest error measured on MI355X over these cases (4.8e-7), and never
    worse than the direct kernel's own error against the same fp64 reference (checked alongside)."""
    from dc_vic_amd import ops
    Cin, Cout, H, W, N, split, res, act = case
    x = rnd(N, Cin, H, W, seed=11)
    w = rnd(Cout, Cin, 3, 3, seed=12, scale=(Cin * 9) ** -0.5)
    b = rnd(Cout, seed=13, scale=0.1)
    r = rnd(N, Cout, H, W, seed=14) if res else None
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    if act == 3:
        ref = ref * torch.sigmoid(ref)
    elif act == 2:
        ref = torch.where(ref > 0, ref, 0.2 * ref)
    if res:
        ref = ref + r.double()
    direct = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1))
    wino = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1))
    wino.wino = "force"
    xs = x.to(dev)
    srcs = xs if split is None else [t.contiguous() for t in torch.split(xs, split, dim=1)]
    rd = r.to(dev) if res else None
    yd = direct(srcs, act=act, res=rd)
    yw = wino(srcs, act=act, res=rd)
    sc = float(ref.abs().max())
    ed = float((yd.double().cpu() - ref).abs().max()) / sc
    ew = float((yw.double().cpu() - ref).abs().max()) / sc
    assert ew < 2e-6, (ew, ed)
    assert ew < 4 * ed + 1e-7, (ew, ed)


def test_wino_batch_invariant_and_deterministic(dev):
    """The tile grid and the per-position reduction order never depend on N: an image convolved alone or inside a batch
    gives the same bits, and so do two runs."""
    from dc_vic_amd import ops
    x = rnd(5, 128, 64, 96, seed=21).to(dev)
    w = rnd(256, 128, 3, 3, seed=22, scale=(128 * 9) ** -0.5).to(dev)
    b = rnd(256, seed=23).to(dev)
    plan = ops.ConvPlan(w, b, "conv", pad=(1, 1))
    plan.wino = "force"
    y5 = plan(x)
    y5b = plan(x)
    y1 = plan(x[3:4].contiguous())
    assert torch.equal(y5, y5b)
    assert torch.equal(y5[3:4], y1)


def test_wino_eligibility_is_a_function_of_layer_and_image_only(dev):
    """ConvPlan._wino_ok must not look at N (a reconstruction may not depend on its batch), must refuse odd widths,
    unaligned sources, and maps that waste the 8 x 32 tiles; such layers run on the direct kernels."""
    from dc_vic_amd import ops
    w = rnd(128, 128, 3, 3, seed=31, scale=0.03).to(dev)
    plan = ops.ConvPlan(w, None, "conv", pad=(1, 1))
    plan.wino = True
    mk = lambda n, c, h, ww: [torch.empty((n, c, h, ww), device=dev)]
    assert plan._wino_ok(mk(1, 128, 256, 256), 1, 256, 256) and plan._wino_ok(mk(32, 128, 256, 256), 32, 256, 256)
    assert plan._wino_ok(mk(1, 128, 32, 32), 1, 32, 32) == plan._wino_ok(mk(32, 128, 32, 32), 32, 32, 32)
    assert not plan._wino_ok(mk(1, 128, 64, 62), 1, 64, 62)          # width not a multiple of 4
    assert not plan._wino_ok(mk(1, 128, 8, 8), 1, 8, 8)              # 8 x 8 map in an 8 x 32 tile
    assert not plan._wino_ok([torch.empty((1, 124, 64, 64), device=dev), torch.empty((1, 4, 64, 64), device=dev)], 1, 64, 64)
    y_auto = plan(torch.zeros((1, 128, 8, 8), device=dev))            # falls back to the direct kernel
    assert y_auto.shape == (1, 128, 8, 8)


@pytest.mark.parametrize("case", [(8, 64, 4, 16, 1), (16, 64, 6, 12, 2), (64, 128, 17, 36, 2), (256, 192, 32, 32, 2), (24, 64, 64, 64, 3)])
def test_wino_upsample_conv(dev, case):
    """dcvic_conv3x3_wino_ups_f32 (nearest x2 + conv3x3 as the 9-position structured Winograd) vs torch in fp64: same
    tolerance as test_wino_conv3x3; odd stage counts exercise both operand-set parities, (24, ..., 3) the persistent tile loop."""
    from dc_vic_amd import ops
    Cin, Cout, H, W, N = case
    x = rnd(N, Cin, H, W, seed=41)
    w = rnd(Cout, Cin, 3, 3, seed=42, scale=(Cin * 9) ** -0.5)
    b = rnd(Cout, seed=43, scale=0.1)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
    phases = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1), upsample=True)
    wino = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1), upsample=True)
    wino.wino = "force"
    yp = phases(x.to(dev))
    yw = wino(x.to(dev))
    assert yw.shape == ref.shape
    sc = float(ref.abs().max())
    ep = float((yp.double().cpu() - ref).abs().max()) / sc
    ew = float((yw.double().cpu() - ref).abs().max()) / sc
    assert ew < 2e-6, (ew, ep)
    y1 = wino(x[:1].contiguous().to(dev))
    assert torch.equal(y1, yw[:1])            # batch-invariant


def test_wino_fuzz_vs_direct(dev):
    """40 random layer geometries (channels, ragged sizes, 1-3 sources, residual, activation, batch) through both Winograd
    kernels against the direct kernels: 5e-6 of the output's max (two fp32 evaluations of the same sum; each is within 2e-6 of
    fp64 in test_wino_conv3x3).  Exercises the persistent tile loop (more tiles than workgroups), partial tiles in both
    directions, channel tiles beyond Cout and source switches inside a tile's stage stream."""
    from dc_vic_amd import ops
    rng = np.random.RandomState(7)
    for it in range(40):
        ups = it % 4 == 3
        n_src = int(rng.randint(1, 4))
        cs = [8 * int(rng.randint(1, 9)) for _ in range(n_src)]
        Cin = sum(cs)
        Cout = int(rng.choice([48, 64, 96, 128, 192, 200, 256]))
        H = int(rng.randint(3, 41))
        W = 4 * int(rng.randint(1, 25))
        N = int(rng.randint(1, 6))
        act = int(rng.choice([0, 1, 2, 3]))
        res = bool(rng.randint(0, 2)) and not ups
        x = rnd(N, Cin, H, W, seed=100 + it)
        w = rnd(Cout, Cin, 3, 3, seed=200 + it, scale=(Cin * 9) ** -0.5)
        b = rnd(Cout, seed=300 + it, scale=0.1)
        Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
        r = rnd(N, Cout, Ho, Wo, seed=400 + it).to(dev) if res else None
        direct = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1), upsample=ups)
        wino = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1), upsample=ups)
        wino.wino = "force"
        xs = x.to(dev)
        srcs = [t.contiguous() for t in torch.split(xs, cs, dim=1)] if n_src > 1 else xs
        yd = direct(srcs, act=act, res=r)
        yw = wino(srcs, act=act, res=r)
        sc = float(yd.abs().max())
        err = float((yd - yw).abs().max()) / max(sc, 1e-6)
        assert err < 5e-6, (it, ups, cs, Cout, H, W, N, act, res, err)


# ------------------------------------------------------------------------------------------- Winograd F(4x4, 3x3) (csrc/wino44.hip)
@pytest.mark.parametrize("case", [
    (8, 64, 8, 32, 1, None, False, 0), (16, 64, 10, 28, 2, None, False, 1), (64, 128, 33, 72, 2, None, True, 2),
    (128, 192, 64, 64, 2, None, True, 0), (256, 128, 40, 48, 1, [192, 64], False, 0), (704, 512, 32, 32, 2, [192, 512], False, 0),
    (8, 200, 19, 36, 3, None, True, 0)])
def test_wino44_conv3x3(dev, case):
    """dcvic_conv3x3_wino44_f32 (F(4x4, 3x3), points 0, +-3/4, +-3/2, inf) vs torch conv2d in fp64: 1.2e-5 of the output's max -- 4x the
    largest error measured on MI355X over these cases (2.9e-6); the direct kernel's error against the same reference is 2.8e-7 ..
    1.8e-6, F(2x2)'s 1.4e-7 .. 4.8e-7 (test_wino_conv3x3).  Cases: one stage, several stages, ragged maps with partial tiles in both
    directions, residual, ReLU / LeakyReLU epilogues, two sources switching inside the stage stream (the SFT fusion's 192 + 512
    channel concat buffer), Cout not a multiple of 64."""
    from dc_vic_amd import ops
    Cin, Cout, H, W, N, split, res, act = case
    x = rnd(N, Cin, H, W, seed=51)
    w = rnd(Cout, Cin, 3, 3, seed=52, scale=(Cin * 9) ** -0.5)
    b = rnd(Cout, seed=53, scale=0.1)
    r = rnd(N, Cout, H, W, seed=54) if res else None
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    if act == 1:
        ref = torch.relu(ref)
    elif act == 2:
        ref = torch.where(ref > 0, ref, 0.2 * ref)
    if res:
        ref = ref + r.double()
    plan = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1))
    plan.wino = plan.wino44 = "force"
    xs = x.to(dev)
    srcs = xs if split is None else [t.contiguous() for t in torch.split(xs, split, dim=1)]
    rd = r.to(dev) if res else None
    ops.kernel_events_start()
    y = plan(srcs, act=act, res=rd)
    torch.cuda.synchronize()
    ev = ops.kernel_events_stop()
    assert list(ev) == ["conv3x3_wino44_kernel(ConvKArgs)"], list(ev)           # the F(4x4) kernel really ran
    err = float((y.double().cpu() - ref).abs().max()) / float(ref.abs().max())
    assert err < 1.2e-5, err


def test_wino44_batch_invariant_deterministic_and_variants(dev):
    """The tile grid and the per-position reduction order never depend on N: an image convolved alone, inside a batch, or in a batch
    large enough for the persistent workgroups to walk several tiles gives the same bits, and so do two runs.  The result stays within
    5e-6 of the F(2x2) kernel and 1.2e-5 of the direct one on the same data."""
    from dc_vic_amd import ops
    x = rnd(9, 128, 64, 96, seed=61).to(dev)
    w = rnd(256, 128, 3, 3, seed=62, scale=(128 * 9) ** -0.5).to(dev)
    b = rnd(256, seed=63).to(dev)
    p44 = ops.ConvPlan(w, b, "conv", pad=(1, 1)); p44.wino = p44.wino44 = "force"
    p22 = ops.ConvPlan(w, b, "conv", pad=(1, 1)); p22.wino = "force"
    pd = ops.ConvPlan(w, b, "conv", pad=(1, 1))
    y9, y9b = p44(x), p44(x)
    y1 = p44(x[3:4].contiguous())
    y64 = p44(x.repeat(8, 1, 1, 1)[:64].contiguous())
    assert torch.equal(y9, y9b) and torch.equal(y9[3:4], y1) and torch.equal(y64[3:4], y1) and torch.equal(y64[9 + 3:9 + 4], y1)
    sc = float(pd(x).abs().max())
    assert float((y9 - p22(x)).abs().max()) / sc < 1.2e-5 and float((y9 - pd(x)).abs().max()) / sc < 1.2e-5


def test_wino44_eligibility_and_fallbacks(dev):
    """ConvPlan._wino44_ok is a function of the layer and the image size only (never of N), refuses widths that are not a multiple of 4,
    Cin not a multiple of 8, maps that waste the 16 x 32 tiles, and the transcendental epilogues; such launches run on F(2x2) or the
    direct kernels.  DCVIC_WINO44=0 (ops.WINO44_ENABLED) switches the layer class back to F(2x2)."""
    from dc_vic_amd import ops
    w = rnd(128, 128, 3, 3, seed=71, scale=0.03).to(dev)
    plan = ops.ConvPlan(w, None, "conv", pad=(1, 1))
    plan.wino = plan.wino44 = True
    mk = lambda n, c, h, ww: [torch.empty((n, c, h, ww), device=dev)]
    assert plan._wino44_ok(mk(1, 128, 256, 256), 1, 256, 256) and plan._wino44_ok(mk(32, 128, 256, 256), 32, 256, 256)
    assert plan._wino44_ok(mk(1, 128, 32, 32), 1, 32, 32) == plan._wino44_ok(mk(32, 128, 32, 32), 32, 32, 32)
    assert not plan._wino44_ok(mk(1, 128, 64, 62), 1, 64, 62)          # width not a multiple of 4
    assert not plan._wino44_ok(mk(1, 128, 8, 8), 1, 8, 8)              # 8 x 8 map in a 16 x 32 tile
    assert not plan._wino44_ok([torch.empty((1, 124, 64, 64), device=dev), torch.empty((1, 4, 64, 64), device=dev)], 1, 64, 64)

    def kernel_of(p, x, **kw):
        ops.kernel_events_start()
        p(x, **kw)
        torch.cuda.synchronize()
        return list(ops.kernel_events_stop())
    x = torch.zeros((1, 128, 128, 128), device=dev)
    assert kernel_of(plan, x) == ["conv3x3_wino44_kernel(ConvKArgs)"]
    assert kernel_of(plan, x, act=ops.ACT_SWISH) == ["conv3x3_wino_kernel(ConvKArgs)"]       # swish epilogue: F(2x2)
    assert "wino" not in kernel_of(plan, torch.zeros((1, 128, 8, 8), device=dev))[0]                   # tiny map: direct kernel
    old = ops.WINO44_ENABLED
    ops.WINO44_ENABLED = False
    try:
        assert kernel_of(plan, x) == ["conv3x3_wino_kernel(ConvKArgs)"]
    finally:
        ops.WINO44_ENABLED = old


def test_wino44_only_behind_the_last_integer_decision(dev):
    """F(4x4) has ~3x the rounding error of F(2x2): the model may enable it ONLY on the frozen VQGAN decoder and the SFT fusion
    blocks (after the estimator's argmax).  Encoder-side and entropy-side layers must never carry the flag."""
    import os
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.layers import Conv2d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = build_comp_model(BaseConfig.fromfile(os.path.join(root, "config", "dc_vic_synthetic.yaml"), {"device": dev}))
    on = {n for n, mod in m.named_modules() if isinstance(mod, Conv2d) and getattr(mod, "wino44", False)}
    assert on and all(n.startswith(("vq_model.decoder.", "fusion_module.")) for n in on), sorted(on)[:5]
    for prefix in ("vq_model.encoder.", "encoder.", "decoder.", "hyperencoder.", "hyperdecoder.", "context_model.", "vq_estimator."):
        assert not any(n.startswith(prefix) for n in on), prefix
    assert any(n.startswith("vq_model.decoder.up.") for n in on) and any(n.startswith("fusion_module.fusion_modules.") for n in on)


def test_wino44_fuzz_vs_direct(dev):
    """30 random layer geometries (channels, ragged sizes, 1-3 sources, residual, ReLU / LeakyReLU, batch) through the F(4x4) kernel
    against the direct kernels: 1.5e-5 of the output's max.  Exercises the persistent tile loop (more tiles than workgroups), partial
    tiles in both directions, channel tiles beyond Cout and source switches inside a tile's stage stream."""
    from dc_vic_amd import ops
    rng = np.random.RandomState(17)
    for it in range(30):
        n_src = int(rng.randint(1, 4))
        cs = [8 * int(rng.randint(1, 9)) for _ in range(n_src)]
        Cin = sum(cs)
        Cout = int(rng.choice([48, 64, 96, 128, 192, 200, 256]))
        H = int(rng.randint(3, 41))
        W = 4 * int(rng.randint(1, 25))
        N = int(rng.randint(1, 6))
        act = int(rng.choice([0, 1, 2]))
        res = bool(rng.randint(0, 2))
        x = rnd(N, Cin, H, W, seed=500 + it)
        w = rnd(Cout, Cin, 3, 3, seed=600 + it, scale=(Cin * 9) ** -0.5)
        b = rnd(Cout, seed=700 + it, scale=0.1)
        r = rnd(N, Cout, H, W, seed=800 + it).to(dev) if res else None
        direct = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1))
        f44 = ops.ConvPlan(w.to(dev), b.to(dev), "conv", pad=(1, 1))
        f44.wino = f44.wino44 = "force"
        xs = x.to(dev)
        srcs = [t.contiguous() for t in torch.split(xs, cs, dim=1)] if n_src > 1 else xs
        yd = direct(srcs, act=act, res=r)
        yw = f44(srcs, act=act, res=r)
        sc = float(yd.abs().max())
        err = float((yd - yw).abs().max()) / max(sc, 1e-6)
        assert err < 1.5e-5, (it, cs, Cout, H, W, N, act, res, err)


# route -> (kernel, upsample, F(4x4), output tile rows, batch): 18 workgroup tiles per image on the 8 x 32-pixel tiles, 12 on the 16 x 32
WINO_FAMILY = {
    "wino": ("conv3x3_wino_kernel(ConvKArgs)", False, False, 8, 48),
    "wino_ups": ("conv3x3_wino_ups_kernel(ConvKArgs)", True, False, 8, 48),
    "wino44": ("conv3x3_wino44_kernel(ConvKArgs)", False, True, 16, 66),
    "wino44_ups": ("conv3x3_wino44_ups_kernel(ConvKArgs)", True, True, 16, 66),
}


@pytest.mark.parametrize("route", list(WINO_FAMILY))
def test_wino_family_split_sources_equal_concatenated(dev, route):
    """The persistent stage stream of the four Winograd kernels (csrc/wino_stream.h) only moves pointers.  So a layer fed three sources
    gives the same BITS as the same layer fed their concatenation, and an image gives the same bits alone as at the end of a batch in
    which every workgroup walks an uneven 3 - 4 tiles (the tile count of a workgroup, the bias parity flip, the X stream running ahead
    into the next image and co-tile).  Sources of 8, 16 and 8 channels (a source switch at every stage but one), Cout = 136 (three
    co-tiles, the last with 8 live channels), LeakyReLU, a residual on the same-size routes, tiles ragged in both directions."""
    from dc_vic_amd import ops
    kernel, ups, f44, th, N = WINO_FAMILY[route]
    cs, Cout = [8, 16, 8], 136
    H, W = (10, 20) if ups else (20, 36)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    n_tiles = N * ((Ho + th - 1) // th) * ((Wo + 31) // 32) * ((Cout + 63) // 64)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert n_tiles > 3 * n_cu and n_tiles % n_cu != 0, (n_tiles, n_cu)
    x = rnd(N, sum(cs), H, W, seed=901).to(dev)
    w = rnd(Cout, sum(cs), 3, 3, seed=902, scale=(sum(cs) * 9) ** -0.5).to(dev)
    b = rnd(Cout, seed=903, scale=0.1).to(dev)
    r = None if ups else rnd(N, Cout, Ho, Wo, seed=904).to(dev)
    plan = ops.ConvPlan(w, b, "conv", pad=(1, 1), upsample=ups)
    plan.wino = "force"
    plan.wino44 = "force" if f44 else False
    split = lambda t: [s.contiguous() for s in torch.split(t, cs, dim=1)]
    ops.kernel_events_start()
    y = plan(split(x), act=ops.ACT_LRELU02, res=r)
    y_cat = plan(x, act=ops.ACT_LRELU02, res=r)
    y_last = plan(split(x[N - 1:]), act=ops.ACT_LRELU02, res=None if r is None else r[N - 1:].contiguous())
    torch.cuda.synchronize()
    ev = ops.kernel_events_stop()
    assert list(ev) == [kernel], list(ev)
    assert y.shape == (N, Cout, Ho, Wo)
    assert torch.equal(y, y_cat)
    assert torch.equal(y[N - 1:], y_last)


# ------------------------------------------------------------------------------------------- thin layers (csrc/thin.hip)
@pytest.mark.parametrize("case", [(128, 3, 70, 100, 2, True, 0), (128, 3, 256, 256, 1, False, 0), (64, 4, 9, 130, 3, False, 3), (8, 1, 5, 7, 1, True, 1),
                                  (3, 128, 70, 100, 2, False, 0), (3, 128, 256, 256, 1, False, 0), (4, 40, 9, 130, 3, True, 2), (1, 16, 5, 7, 2, False, 3)])
def test_thin_conv_bit_identical_to_the_mfma_kernels(dev, case):
    """dcvic_conv3x3_thin_f32 (VQGAN conv_in 3 -> 128, conv_out 128 -> 3: HBM-bound VALU kernels) runs the fmaf chain in exactly the
    order of the MFMA kernels it replaces, so the outputs are equal BIT FOR BIT (incl. ragged sizes, bias / residual / activation
    epilogues) -- no tolerance, no parity question up- or downstream."""
    from dc_vic_amd import ops
    Cin, Cout, H, W, N, res, act = case
    x = rnd(N, Cin, H, W, seed=91).to(dev)
    w = rnd(Cout, Cin, 3, 3, seed=92, scale=(Cin * 9) ** -0.5).to(dev)
    b = rnd(Cout, seed=93, scale=0.1).to(dev)
    r = rnd(N, Cout, H, W, seed=94).to(dev) if res else None
    plan = ops.ConvPlan(w, b, "conv", pad=(1, 1))
    old_min, ops.THIN_MIN_PIXELS = ops.THIN_MIN_PIXELS, 0         # (the model uses the thin kernels on full-resolution maps only)
    ops.kernel_events_start()
    y_thin = plan(x, act=act, res=r)
    torch.cuda.synchronize()
    ev = list(ops.kernel_events_stop())
    assert len(ev) == 1 and "thin_" in ev[0], ev
    old = ops.THIN_ENABLED
    ops.THIN_ENABLED = False
    try:
        ops.kernel_events_start()
        y_mfma = plan(x, act=act, res=r)
        torch.cuda.synchronize()
        ev2 = list(ops.kernel_events_stop())
    finally:
        ops.THIN_ENABLED = old
    assert "thin_" not in ev2[0]
    assert torch.equal(y_thin, y_mfma), float((y_thin - y_mfma).abs().max())
    y1 = plan(x[:1].contiguous(), act=act, res=None if r is None else r[:1].contiguous())
    ops.THIN_MIN_PIXELS = old_min
    assert torch.equal(y1, y_thin[:1])                            # batch-invariant


def test_groupnorm_statistics_from_the_wino44_epilogue(dev):
    """the F(4x4) convolution's epilogue writes per (image, channel, pixel tile) partial sums of exactly the values it
    stores (bias, LeakyReLU and residual included); dcvic_groupnorm_part_f32 adds them in fp64 and skips its own statistics pass.
    Checked: the partials against fp64 sums of the stored map (ragged size: partial tiles, Cout not a multiple of 64), and the
    GroupNorm + swish output against the two-pass kernel on the same map (1e-6 relative: fp32 tile sums instead of one fp64 sum)."""
    from dc_vic_amd import ops
    N, Cin, Cout, H, W = 3, 64, 160, 40, 72
    x = rnd(N, Cin, H, W, seed=95).to(dev)
    w = rnd(Cout, Cin, 3, 3, seed=96, scale=(Cin * 9) ** -0.5).to(dev)
    b = rnd(Cout, seed=97, scale=0.5).to(dev)
    r = rnd(N, Cout, H, W, seed=98).to(dev)
    plan = ops.ConvPlan(w, b, "conv", pad=(1, 1))
    plan.wino = plan.wino44 = "force"
    y = plan(x, act=ops.ACT_LRELU02, res=r, gn_stats=True)
    part, n_pt = plan.last_gn_part
    assert n_pt == 3 * 3 and tuple(part.shape) == (N, Cout, n_pt, 2)
    yd = y.double()
    S = part[..., 0].double().sum(-1).cpu(); Q = part[..., 1].double().sum(-1).cpu()
    assert float((S - yd.sum((2, 3)).cpu()).abs().max()) < 1e-3 * float(yd.abs().sum((2, 3)).max()) * 1e-3
    assert float((Q - (yd * yd).sum((2, 3)).cpu()).abs().max()) < 1e-6 * float((yd * yd).sum((2, 3)).max())
    # one tile alone: rows 32..39 of the map (the ragged last tile row), columns 64..71
    t = yd[:, :, 32:40, 64:72]
    assert float((part[:, :, 8, 0].double().cpu() - t.sum((2, 3)).cpu()).abs().max()) < 1e-4
    g, be = (rnd(Cout, seed=99, scale=1.0) + 1.0).to(dev), rnd(Cout, seed=100, scale=0.3).to(dev)
    a = ops.groupnorm(y, g, be, 32, 1e-6, ops.ACT_SWISH)
    bq = ops.groupnorm(y, g, be, 32, 1e-6, ops.ACT_SWISH, part=(part, n_pt))
    assert float((a - bq).abs().max()) < 2e-6 * float(a.abs().max())
    # no statistics asked / not an F(4x4) launch: nothing handed over
    plan(x, act=ops.ACT_LRELU02, res=r)
    assert plan.last_gn_part is None
    p2 = ops.ConvPlan(w, b, "conv", pad=(1, 1)); p2.wino = "force"
    p2(x, gn_stats=True)
    assert p2.last_gn_part is None
    with pytest.raises(ValueError):
        ops.groupnorm(y[:, :128].contiguous(), g[:128], be[:128], 32, 1e-6, ops.ACT_SWISH, part=(part, n_pt))


@pytest.mark.parametrize("shape", [(3, 192, 16, 16), (1, 192, 80, 128), (2, 5, 3, 7)])
def test_absmax_matches_torch(dev, shape):
    """max |y_hat| per image (the header's third byte, codec_utils.py:16-47): split over workgroups that meet in an order-free
    atomic max -- exact, also through a batch-strided view."""
    from dc_vic_amd import ops
    x = rnd(*shape, seed=77, scale=7.0)
    x[0, 0, 0, 0] = -123.5                                   # the maximum is a negative value's magnitude
    got = ops.absmax(x.to(dev)).cpu()
    assert torch.equal(got, x.abs().amax(dim=(1, 2, 3)))
    big = rnd(shape[0], shape[1] + 3, shape[2], shape[3], seed=78).to(dev)
    view = big[:, 1:1 + shape[1]]
    assert torch.equal(ops.absmax(view).cpu(), view.cpu().abs().amax(dim=(1, 2, 3)))
