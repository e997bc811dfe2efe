"""The entropy-model and data-movement kernels (csrc/rate.hip, csrc/ew.hip) called the way the codec calls them, on a real MI355X.

test_gpu_kernels.py runs each of these kernels once, on dense tensors, in one mode.  The codec reaches them differently:
 * gaussian_rate on CHARM channel slices (charm.py: y[:, sl], sym[:, sl], idx[:, sl], lik[:, sl]) with mu / sigma the two halves of one
   hyper output, in encode, index-only (charm.py, entropy.py build_indexes) and decode mode, adding each slice's bits onto bits[n];
 * both gaussian_rate kernels: the float4 one needs C*HW, every batch stride and every pointer to be multiples of 4 / 16 B, the scalar one
   takes the rest (ragged images, misaligned slices);
 * eb_rate decode (EntropyBottleneck.decompress) and its accumulated bits;
 * neglog2_sum, the rate of the training / eval path;
 * copy_window (tile cut and stitch), crop, copy_planes into a channel slice (fusion.py), pad_reflect and crop_clamp through views.
Integer outputs and copies are compared exactly; floating outputs against float64 with the bound stated at each check.  Every region a
kernel must not write holds a sentinel that is checked afterwards."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
F_SENT = -12345.0       # sentinel of float buffers
I_SENT = -7777          # sentinel of int32 buffers


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from dc_vic_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ratio(got, ref, rtol, atol):
    """Worst |got - ref| / (atol + rtol |ref|) (<= 1 passes), got against a float64 reference."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def outside_untouched(big, sl, sent):
    """Every channel of `big` outside the slice `sl` still holds the sentinel."""
    keep = torch.ones(big.shape[1], dtype=torch.bool)
    keep[sl] = False
    rest = big.cpu()[:, keep]
    return bool((rest == sent).all())


# ------------------------------------------------------------------------------------------- gaussian_rate
def _vec_path(CHW, ptrs, strides):
    """csrc/rate.hip's dispatch rule: the float4 kernel iff C*HW, every batch stride and every pointer are multiples of 4 / 16 B."""
    return CHW % 4 == 0 and all(s % 4 == 0 for s in strides) and all(p % 16 == 0 for p in ptrs)


# (N, C, H, W, a, Cbig, vector kernel?): slices [a, a+C) and [a+C, a+2C) of [N, Cbig, H, W] buffers
RATE_CASES = [
    (2, 32, 16, 16, 8, 80, True),       # float4 kernel
    (3, 21, 7, 9, 3, 47, False),        # odd C*HW (1323): scalar kernel
    (2, 16, 6, 5, 2, 35, False),        # C*HW 480 and 16-B aligned slices, but a batch stride (1050) not divisible by 4
    (2, 16, 6, 5, 1, 34, False),        # batch strides divisible by 4, slice offsets (30, 510 floats) misalign the pointers
    (1, 40, 64, 64, 4, 88, True),       # N = 1, C*HW 163840 > 64 * 2048: dcvic_rate_blocks saturates at 64 (float4)
    (1, 33, 63, 65, 1, 68, False),      # the same saturation on the scalar kernel (C*HW 135135)
]
# sigma edges (the 0.11 bound, the table ends, far past the table), then y - mu large against a small sigma: p at the 1e-9 floor
SIGMA_EDGES = [0.0, 0.05, 0.11, 0.110001, 255.9, 256.0, 300.0, 1e4]


def _rate_data(N, C, H, W, seed):
    """y [N, C, H, W] and the hyper output ms = cat(mu, sigma) [N, 2C, H, W] of one slice, with the sigma edges and the floor cases at
    the start of image 0 and at the end of image N-1 (the scalar kernel's tail)."""
    y = rnd(N, C, H, W, seed=seed, scale=3.0)
    mu = rnd(N, C, H, W, seed=seed + 1)
    sigma = rnd(N, C, H, W, seed=seed + 2, scale=2.0).abs() * torch.exp(rnd(N, C, H, W, seed=seed + 3))
    yf, mf, sf = y.view(N, -1), mu.view(N, -1), sigma.view(N, -1)
    for n, base in ((0, 0), (N - 1, C * H * W - 12)):
        sf[n, base:base + 8] = torch.tensor(SIGMA_EDGES)
        # |y - mu| / sigma of 300 and more: both Phi terms underflow and p = max(0, 1e-9)
        sf[n, base + 8:base + 12] = torch.tensor([0.11, 0.2, 0.5, 1.0])
        yf[n, base + 8:base + 12] = mf[n, base + 8:base + 12] + torch.tensor([40.0, -60.0, 250.0, -1000.0])
    return y, torch.cat([mu, sigma], 1)


def _gc_lik64(yh, mu, sigma):
    """GaussianConditional likelihood in float64 from the kernel's fp32 operands: v = |y_hat - mu| as the kernel forms it (fp32),
    s = max(sigma, 0.11f), p = max(Phi((0.5 - v) / s) - Phi((-0.5 - v) / s), 1e-9)."""
    v = (yh - mu).abs().double()
    s = torch.clamp(sigma, min=torch.tensor(0.11, dtype=torch.float32)).double()
    cdf = lambda t: 0.5 * torch.erfc(-t / math.sqrt(2.0))
    return torch.clamp(cdf((0.5 - v) / s) - cdf((-0.5 - v) / s), min=float(np.float32(1e-9)))


class _Bufs:
    """The codec's buffers: y / y_hat / sym / idx / lik are [N, Cbig, H, W] tensors holding a sentinel; slices are views into them."""

    def __init__(self, N, Cbig, H, W, dev, Cy=None, Cyh=None):
        f = lambda c: torch.full((N, c, H, W), F_SENT, device=dev)
        self.y, self.yh = f(Cy or Cbig), f(Cyh or Cbig)
        self.lik = f(Cbig)
        self.sym = torch.full((N, Cbig, H, W), I_SENT, dtype=torch.int32, device=dev)
        self.idx = torch.full((N, Cbig, H, W), I_SENT, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("case", RATE_CASES, ids=lambda c: "N%d_C%d_%dx%d_a%d_big%d_%s" % (*c[:6], "vec" if c[6] else "scalar"))
def test_gaussian_rate_codec_views(dev, case):
    """Encode, index-only and decode mode on CHARM-style slices, on both kernels, adding two slices' bits onto a non-zero start.

    Symbols, cdf indexes and y_hat equal the oracle's fp32 formulas exactly.  The likelihood keeps test_gaussian_rate's bound against the
    float64 formula, |p - p64| <= 3e-7 + 2e-4 p64: p = Phi(a) - Phi(b) cancels, so erfcf's few ulp of Phi (~6e-8 each) are an absolute
    error whatever p is.  bits[n] of a slice keeps test_gaussian_rate's 1e-2 + 2e-4 |bits64| against float64 -sum(log2 p64), and is held
    much tighter against the kernel's own likelihoods: float64 -sum(log2 lik) within 2^-22 sum|log2 lik| (logf: <= 1 ulp a term, the
    sum in fp64) + 2^-24 |bits| (the one fp32 rounding of the result)."""
    from dc_vic_amd import ops
    from oracle import entropy_oracle as eo
    N, C, H, W, a, Cbig, vec = case
    CHW = C * H * W
    table = eo.get_scale_table().to(dev)
    sls = [slice(a, a + C), slice(a + C, a + 2 * C)]
    # y is read from a wider buffer than the outputs and y_hat written into a third width: each stream has its own batch stride
    B = _Bufs(N, Cbig, H, W, dev, Cy=Cbig + 2, Cyh=Cbig + (4 if vec else 6))
    data = [_rate_data(N, C, H, W, seed=100 + 10 * k) for k in range(2)]
    ms_dev = [d[1].to(dev) for d in data]
    for k, sl in enumerate(sls):
        B.y[:, sl] = data[k][0].to(dev)

    def encode(k, bits):
        mu_d, sg_d = ms_dev[k].chunk(2, 1)            # like hyper_out.chunk(2, 1): batch stride 2 C HW
        sl = sls[k]
        ops.gaussian_rate(B.y[:, sl], None, mu_d, sg_d, table, B.yh[:, sl], B.sym[:, sl], B.idx[:, sl], B.lik[:, sl], bits)

    for k, sl in enumerate(sls):
        ptrs = [t.data_ptr() for t in (B.y[:, sl], ms_dev[k], ms_dev[k][:, C:], B.yh[:, sl], B.sym[:, sl], B.idx[:, sl], B.lik[:, sl])]
        assert _vec_path(CHW, ptrs, [B.y.stride(0), ms_dev[k].stride(0), B.yh.stride(0), B.sym.stride(0)]) == vec, \
            "the case does not reach the kernel it is meant for"

    # encode both slices into one bits buffer that starts at a non-zero value
    start = torch.tensor([1000.25, -3.5, 7.0][:N])
    bits = start.clone().to(dev)
    encode(0, bits)
    after0 = bits.cpu()
    encode(1, bits)
    acc = bits.cpu()
    # each slice alone, from zero, with the same arguments (the same kernel and layout; outputs are rewritten with the same values)
    alone = []
    for k in range(2):
        z = torch.zeros(N, device=dev)
        encode(k, z)
        alone.append(z.cpu())
    assert torch.equal(after0, start + alone[0]), "bits_out is not accumulated (+=)"
    assert torch.equal(acc, (start + alone[0]) + alone[1]), "bits_out is not accumulated (+=)"

    worst = {"lik": 0.0, "bits": 0.0, "bits_own": 0.0}
    for k, sl in enumerate(sls):
        y, ms = data[k]
        mu, sigma = ms[:, :C], ms[:, C:]
        sym_ref = torch.round(y - mu)
        yh_ref = sym_ref + mu
        assert torch.equal(B.sym[:, sl].cpu(), sym_ref.int())
        assert torch.equal(B.idx[:, sl].cpu(), eo.gc_build_indexes(sigma))
        assert torch.equal(B.yh[:, sl].cpu(), yh_ref)
        lik = B.lik[:, sl].cpu().reshape(N, -1)
        lik64 = _gc_lik64(yh_ref, mu, sigma).reshape(N, -1)
        assert float(lik[0, 8]) == np.float32(1e-9) and float(lik[N - 1, -1]) == np.float32(1e-9), "the 1e-9 floor was not reached"
        worst["lik"] = max(worst["lik"], ratio(lik, lik64, 2e-4, 3e-7))
        worst["bits"] = max(worst["bits"], ratio(alone[k], -torch.log(lik64).sum(1) / LN2, 2e-4, 1e-2))
        own = -torch.log(lik.double()).sum(1) / LN2
        bound = 2.0 ** -22 * (torch.log(lik.double()).abs().sum(1) / LN2) + 2.0 ** -24 * own.abs()
        worst["bits_own"] = max(worst["bits_own"], float(((alone[k].double() - own).abs() / bound).max()))
    for buf, sent in ((B.y, F_SENT), (B.yh, F_SENT), (B.lik, F_SENT), (B.sym, I_SENT), (B.idx, I_SENT)):
        assert outside_untouched(buf, slice(a, a + 2 * C), sent), "a channel outside the slices was written"

    # index-only, as charm.py (the slice's own symbols as a placeholder sym_in) and entropy.py build_indexes (zeros, mu = sigma = scales)
    snap = {n: getattr(B, n).clone() for n in ("y", "yh", "lik", "sym")}
    B.idx.fill_(I_SENT)
    for k, sl in enumerate(sls):
        ops.gaussian_rate(None, B.sym[:, sl], ms_dev[k][:, :C], ms_dev[k][:, C:], table, None, None, B.idx[:, sl], None, None)
    for k, sl in enumerate(sls):
        assert torch.equal(B.idx[:, sl].cpu(), eo.gc_build_indexes(data[k][1][:, C:]))
    assert outside_untouched(B.idx, slice(a, a + 2 * C), I_SENT)
    for n, t in snap.items():
        assert torch.equal(getattr(B, n), t), f"the index-only call wrote {n}"
    from dc_vic_amd.entropy import GaussianMeanScaleConditional
    gc = GaussianMeanScaleConditional().to(dev)
    for k in range(2):
        assert torch.equal(gc.build_indexes(ms_dev[k][:, C:]).cpu(), eo.gc_build_indexes(data[k][1][:, C:]))

    # decode: y_hat from the symbols into the slices of a fresh sentinel buffer, bit-identical to encode mode
    yh2 = torch.full_like(B.yh, F_SENT)
    for k, sl in enumerate(sls):
        ops.gaussian_rate(None, B.sym[:, sl], ms_dev[k][:, :C], ms_dev[k][:, C:], table, yh2[:, sl], None, None, None, None)
    assert torch.equal(yh2[:, a:a + 2 * C], B.yh[:, a:a + 2 * C])
    assert outside_untouched(yh2, slice(a, a + 2 * C), F_SENT)
    assert torch.equal(B.sym, snap["sym"])

    # scalar kernel against float4 kernel: a scalar case whose C*HW is a multiple of 4 (the two C*HW = 480 cases) is rerun on the same
    # logical data in dense 16-B aligned tensors, which take the float4 kernel.  Elementwise outputs must be bit-identical.  bits[n] is
    # the same fp64 sum taken in another order (four elements per lane against one), so it may differ by the final fp32 rounding
    # (1 ulp) only.  The float4 cases are already on the float4 kernel and have nothing to compare against here.
    if not vec and CHW % 4 == 0:
        for k, sl in enumerate(sls):
            ms_d = ms_dev[k].clone()
            yd = data[k][0].to(dev)
            yh, lk = torch.empty(N, C, H, W, device=dev), torch.empty(N, C, H, W, device=dev)
            sy, ix = (torch.empty(N, C, H, W, dtype=torch.int32, device=dev) for _ in range(2))
            bd = torch.zeros(N, device=dev)
            assert _vec_path(CHW, [t.data_ptr() for t in (yd, ms_d, ms_d[:, C:], yh, lk, sy, ix)], [CHW, 2 * CHW])
            ops.gaussian_rate(yd, None, ms_d[:, :C], ms_d[:, C:], table, yh, sy, ix, lk, bd)
            assert torch.equal(yh, B.yh[:, sl]) and torch.equal(sy, B.sym[:, sl]) and torch.equal(lk, B.lik[:, sl])
            assert torch.equal(ix.cpu(), eo.gc_build_indexes(data[k][1][:, C:]))
            assert bool(((bd.cpu() - alone[k]).abs() <= alone[k].abs() * 2.0 ** -23).all())
    print(f"gaussian_rate {case}: worst error / bound: lik {worst['lik']:.3f}, bits {worst['bits']:.3f}, "
          f"bits against its own likelihoods {worst['bits_own']:.3f}")
    assert worst["lik"] <= 1.0 and worst["bits"] <= 1.0 and worst["bits_own"] <= 1.0


# ------------------------------------------------------------------------------------------- eb_rate
@pytest.fixture(scope="module")
def eb(dev, synth_sd):
    from dc_vic_amd.entropy import pack_entropy_bottleneck
    from oracle import entropy_oracle as eo
    orc = eo.EntropyBottleneckOracle(synth_sd, "entropy_model_z")
    orc64 = eo.EntropyBottleneckOracle(synth_sd, "entropy_model_z")
    orc64.p = {k: v.double() for k, v in orc64.p.items()}
    packs = pack_entropy_bottleneck({k: v.to(dev) for k, v in synth_sd.items() if k.startswith("entropy_model_z.")}, "entropy_model_z")
    return orc, orc64, packs


def _eb_run(ops, packs, z, bits_start):
    N, C, H, W = z.shape
    zh = torch.empty(N, C, H, W, device=z.device)
    sym = torch.empty(N, C, H, W, dtype=torch.int32, device=z.device)
    lik = torch.empty(N, C, H, W, device=z.device)
    bits = bits_start.clone().to(z.device)
    ops.eb_rate(z, packs, zh, sym, lik, bits)
    return zh, sym, lik, bits


@pytest.mark.parametrize("N,H,W", [(1, 5, 7), (3, 5, 7), (3, 1, 3)])
def test_eb_rate_roundtrip(dev, eb, N, H, W):
    """EntropyBottleneck encode against the oracle, decode (EntropyBottleneck.decompress's call) back to z_hat, bits accumulated onto a
    non-zero start, and each image's outputs equal to that image run alone.

    z_hat and the symbols are exact.  The likelihood keeps test_eb_rate's bound, |p - p64| <= 3e-7 + 2e-4 p64, against the oracle's
    formula in float64 on the same z_hat; bits against float64 -sum(log2 p64) keeps its 1e-2 + 2e-4 |bits64|."""
    from dc_vic_amd import ops
    orc, orc64, packs = eb
    C = orc.C
    z = rnd(N, C, H, W, seed=60 + N, scale=4.0)
    z.view(-1)[:4] = torch.tensor([1e3, -1e3, 40.0, -40.0])     # far in the tails: the 1e-9 floor
    zh_ref, _ = orc.forward(z)
    start = torch.tensor([512.5, -2.25, 3.0][:N])
    zh, sym, lik, bits = _eb_run(ops, packs, z.to(dev), start)
    assert torch.equal(zh.cpu(), zh_ref)
    assert torch.equal(sym.cpu(), orc.symbols(z))
    assert float(lik.view(-1)[0]) == np.float32(1e-9)
    v = zh_ref.double().permute(1, 0, 2, 3).reshape(C, 1, -1)     # the likelihood at the kernel's (exact) fp32 z_hat
    lik64 = orc64._likelihood(v).clamp(min=float(np.float32(1e-9))).reshape(C, N, H, W).permute(1, 0, 2, 3)
    r_lik = ratio(lik, lik64, 2e-4, 3e-7)
    zero = _eb_run(ops, packs, z.to(dev), torch.zeros(N))[3].cpu()
    assert torch.equal(bits.cpu(), start + zero), "bits_out is not accumulated (+=)"
    r_bits = ratio(zero, -torch.log(lik64).reshape(N, -1).sum(1) / LN2, 2e-4, 1e-2)
    # decode: z_hat from the symbols, bit for bit; nothing else requested, nothing else written
    zh2 = torch.full((N, C, H, W), F_SENT, device=dev)
    ops.eb_rate(None, packs, zh2, None, None, None, sym_in=sym)
    assert torch.equal(zh2, zh)
    # batch invariance: every output of image n equals image n run alone
    for n in range(N):
        zh1, sym1, lik1, bits1 = _eb_run(ops, packs, z[n:n + 1].to(dev), start[n:n + 1])
        assert torch.equal(zh1, zh[n:n + 1]) and torch.equal(sym1, sym[n:n + 1]) and torch.equal(lik1, lik[n:n + 1])
        assert torch.equal(bits1.cpu(), bits.cpu()[n:n + 1])
    print(f"eb_rate N={N} {H}x{W}: worst error / bound: lik {r_lik:.3f}, bits {r_bits:.3f}")
    assert r_lik <= 1.0 and r_bits <= 1.0


# ------------------------------------------------------------------------------------------- neglog2_sum
def _likelihoods(N, C, H, W, seed):
    """p in [1e-9, 1]: exp(-3 |x|) with some entries exactly at the floor and at 1."""
    p = torch.exp(-3.0 * rnd(N, C, H, W, seed=seed).abs()).clamp(min=1e-9)
    f = p.view(N, -1)
    f[:, :3] = torch.tensor([1e-9, 1.0, 1e-9])
    f[:, -2:] = torch.tensor([1.0, 1e-9])
    f[:, 7::97] = 1.0
    return p


@pytest.mark.parametrize("N,C,H,W", [(1, 3, 5, 7), (5, 3, 5, 7), (1, 7, 19, 23), (5, 7, 19, 23), (1, 8, 16, 16), (5, 8, 16, 16),
                                     (1, 36, 64, 64), (5, 36, 64, 64)])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slice"])
def test_neglog2_sum(dev, N, C, H, W, strided):
    """Per-image -sum(log2 p) against float64 (C*HW below one block, not a multiple of 256, exactly 2048, above 64 * 2048).

    Bound: each term is an fp32 logf, within 1 ulp (<= 2^-23 |ln p|); the sum is fp64; the result is rounded to fp32 once:
    |bits - bits64| <= 2^-23 sum|log2 p| + 2^-24 |bits64|.  Two runs, and each image run alone, give identical bits."""
    from dc_vic_amd import ops
    p = _likelihoods(N, C, H, W, seed=70 + C + N)
    if strided:
        big = torch.full((N, C + 5, H, W), 0.5, device=dev)
        big[:, 2:2 + C] = p.to(dev)
        x = big[:, 2:2 + C]
    else:
        x = p.to(dev)
    bits = ops.neglog2_sum(x)
    lp = torch.log(p.double()).reshape(N, -1)
    ref = -lp.sum(1) / LN2
    bound = 2.0 ** -23 * lp.abs().sum(1) / LN2 + 2.0 ** -24 * ref.abs()
    r = float(((bits.cpu().double() - ref).abs() / bound).max())
    assert torch.equal(ops.neglog2_sum(x), bits)
    for n in range(N):
        assert torch.equal(ops.neglog2_sum(x[n:n + 1]), bits[n:n + 1])
    print(f"neglog2_sum N={N} C={C} {H}x{W} {'slice' if strided else 'dense'}: worst error / bound {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------- data movement (exact)
def test_copy_window_tile_cut_and_stitch(dev):
    """copy_window between windows of two larger tensors whose batch, channel and row strides all differ, as comp_model's tile cut
    (window of the image -> dense tile batch) and stitch (window of a tile -> window of the output).  Everything outside stays."""
    from dc_vic_amd import ops
    src_big = rnd(3, 7, 20, 23, seed=80).to(dev)
    dst_big = torch.full((4, 9, 17, 31), F_SENT, device=dev)
    win_s = src_big[1:3, 2:6, 3:14, 5:18]         # [2, 4, 11, 13]
    win_d = dst_big[1:3, 4:8, 2:13, 9:22]
    assert len({win_s.stride(i) for i in range(3)} | {win_d.stride(i) for i in range(3)}) == 6
    ops.copy_window(win_d, win_s)
    ref = torch.full((4, 9, 17, 31), F_SENT)
    ref[1:3, 4:8, 2:13, 9:22] = src_big.cpu()[1:3, 2:6, 3:14, 5:18]
    assert torch.equal(dst_big.cpu(), ref)
    # cut into a dense tile batch (crop[k*N:(k+1)*N] = image[:, :, y0:y0+p, x0:x0+p]) and stitch back into a sentinel image
    tiles = torch.full((4, 7, 8, 8), F_SENT, device=dev)
    ops.copy_window(tiles[2:4], src_big[1:3, :, 9:17, 4:12])
    assert torch.equal(tiles[2:4].cpu(), src_big.cpu()[1:3, :, 9:17, 4:12]) and bool((tiles[:2].cpu() == F_SENT).all())
    out = torch.full((2, 7, 20, 23), F_SENT, device=dev)
    ops.copy_window(out[:, :, 10:15, 6:12], tiles[2:4, :, 1:6, 2:8])
    ref = torch.full((2, 7, 20, 23), F_SENT)
    ref[:, :, 10:15, 6:12] = src_big.cpu()[1:3, :, 10:15, 6:12]
    assert torch.equal(out.cpu(), ref)


def test_crop_and_copy_planes_into_a_channel_slice(dev):
    """crop (comp_model, swin) from a batch-strided source, copy_planes into cat_buf[:, :c] (fusion.py), and a copy region smaller than
    the destination planes: exact, and nothing outside the region written."""
    from dc_vic_amd import ops
    N, c, H, W = 3, 5, 13, 17
    big = rnd(N, c + 4, H, W, seed=81)
    src = big.to(dev)[:, 1:1 + c]
    assert torch.equal(ops.crop(src, 9, 11).cpu(), big[:, 1:1 + c, :9, :11])
    assert torch.equal(ops.crop(src, H, W).cpu(), big[:, 1:1 + c])
    cat_buf = torch.full((N, c + 6, H, W), F_SENT, device=dev)
    ops.copy_planes(cat_buf[:, :c], src, H, W)
    assert torch.equal(cat_buf[:, :c].cpu(), big[:, 1:1 + c]) and bool((cat_buf[:, c:].cpu() == F_SENT).all())
    dst = torch.full((N, c, H + 2, W + 3), F_SENT, device=dev)
    ops.copy_planes(dst, src, H - 1, W - 2)
    ref = torch.full((N, c, H + 2, W + 3), F_SENT)
    ref[:, :, :H - 1, :W - 2] = big[:, 1:1 + c, :H - 1, :W - 2]
    assert torch.equal(dst.cpu(), ref)


@pytest.mark.parametrize("N,C,H,W,pH,pW,strided", [(2, 3, 6, 9, 5, 8, False),    # pad = H - 1, W - 1: the limit of 'reflect'
                                                    (3, 4, 7, 1, 3, 0, False),    # a 1-pixel-wide plane, pad 0 in W
                                                    (3, 4, 7, 1, 6, 0, True),
                                                    (3, 5, 11, 10, 10, 9, True)])   # batch-strided source at the limit
def test_pad_reflect_edges(dev, N, C, H, W, pH, pW, strided):
    from dc_vic_amd import ops
    x = rnd(N, C + 3, H, W, seed=82)
    xs = x[:, 2:2 + C] if strided else x[:, :C].contiguous()
    xd = x.to(dev)[:, 2:2 + C] if strided else xs.to(dev)
    assert torch.equal(ops.pad_reflect(xd, pH, pW).cpu(), F.pad(xs, (0, pW, 0, pH), mode="reflect"))


def test_crop_clamp_views_and_uint8_edges(dev):
    """crop_clamp with N = 3 from a batch-strided view: clamp exact at and past +-1, and the uint8 image truncated as the reference
    (test_elementwise's ((v + 1) / 2 * 255).astype(uint8)), with values on and one ulp either side of every uint8 step."""
    from dc_vic_amd import ops
    N, C, H, W = 3, 3, 16, 40
    big = rnd(N, C + 2, H + 3, W + 5, seed=83, scale=1.2)
    steps = torch.arange(256, dtype=torch.float32) * 2 / 255 - 1            # (v + 1) / 2 * 255 = k
    edges = torch.cat([steps, torch.nextafter(steps, torch.tensor(-2.0)), torch.nextafter(steps, torch.tensor(2.0)),
                       torch.tensor([-1.0, 1.0, -1.0000001, 1.0000001, -3.0, 3.0, 0.0, -0.0])])
    v = big[:, 1:1 + C, :H, :W].reshape(-1)
    v[:edges.numel()] = edges
    v[-edges.numel():] = edges.flip(0)
    big[:, 1:1 + C, :H, :W] = v.view(N, C, H, W)
    x = big.to(dev)[:, 1:1 + C]
    y, y8 = ops.crop_clamp(x, H, W, want_u8=True)
    refc = big[:, 1:1 + C, :H, :W].clamp(-1, 1)
    assert torch.equal(y.cpu(), refc)
    ref8 = ((refc + 1.0) / 2.0 * 255.0).numpy().transpose(0, 2, 3, 1).astype(np.uint8)
    assert np.array_equal(y8.cpu().numpy(), ref8)
    assert ref8.min() == 0 and ref8.max() == 255


# ------------------------------------------------------------------------------------------- argument checks
def test_bad_arguments_raise_before_any_write(dev):
    """Argument errors reach Python as ValueError (ops.py) or DcvicError (the library's checks) and write nothing."""
    from dc_vic_amd import ops
    from dc_vic_amd._lib import DcvicError
    from oracle import entropy_oracle as eo
    x = rnd(2, 3, 6, 5, seed=84).to(dev)
    dst = torch.full((2, 3, 12, 10), F_SENT, device=dev)
    with pytest.raises(DcvicError, match="reflect"):
        ops.copy_planes(dst, x, 12, 5, reflect=True)          # a reflection by H
    with pytest.raises(DcvicError, match="reflect"):
        ops.copy_planes(dst, x, 6, 10, reflect=True)          # ... by W
    with pytest.raises(DcvicError):
        ops.pad_reflect(x, 6, 0)
    with pytest.raises(DcvicError, match="exceeds source"):
        ops.copy_planes(dst, x, 7, 5)
    with pytest.raises(DcvicError, match="exceeds source"):
        ops.crop(x, 6, 6)
    with pytest.raises(ValueError, match="copy_window"):
        ops.copy_window(dst[:, :, :6, :4], x[:, :, :, :5])
    torch.cuda.synchronize()
    assert bool((dst.cpu() == F_SENT).all())

    table = eo.get_scale_table().to(dev)
    ms = torch.rand(2, 6, 6, 5, device=dev) + 0.5
    other = torch.rand(2, 4, 6, 5, device=dev) + 0.5
    yh = torch.full((2, 3, 6, 5), F_SENT, device=dev)
    with pytest.raises(ValueError, match="batch stride"):
        ops.gaussian_rate(x, None, ms[:, :3], other[:, 1:], table, yh, None, None, None, None)
    n_big = 1025
    mu = torch.zeros(n_big, 1, 1, 4, device=dev)
    sg = torch.ones(n_big, 1, 1, 4, device=dev)
    yb = torch.full((n_big, 1, 1, 4), F_SENT, device=dev)
    bits = torch.full((n_big,), 5.0, device=dev)
    with pytest.raises(DcvicError, match="1024"):
        ops.gaussian_rate(mu, None, mu, sg, table, yb, None, None, None, bits)
    torch.cuda.synchronize()
    assert bool((yh.cpu() == F_SENT).all()) and bool((yb.cpu() == F_SENT).all()) and bool((bits.cpu() == 5.0).all())
