"""The kernels that compress / decompress run (csrc/norm.hip, ew.hip, gemm.hip, attn.hip, swin.hip and the four Winograd routes) called
directly, past toy sizes and off N(0, 1) inputs, against torch fp64 on the CPU, element by element.

Two kinds of bound, no others:
  derived   where the kernel's arithmetic is a short fp32 expression around fp64 or exact parts: k * 2^-24 * sum|terms|, sum|terms| in fp64
            from the test and k stated next to the check from the code;
  measured  where the result hangs on a long fp32 chain or on expf of a difference: 4 x the worst error, against fp64 on the same input,
            of a plain fp32 restatement on the CPU that accumulates in the kernel's order class (tests/infer_kernels_ref.py), never below
            16 * 2^-24 * max|ref|.  The margin 4 covers fma against mul + add and the device's expf.  The yardstick is never the kernel.
Operations the kernels restate exactly are compared with torch.equal.  Inputs come from the named regimes of tests/kernel_bounds.py; the
shapes are the smallest that reach each loop (tests/test_infer_kernels_host.py asserts on the CPU that they do).  Every test ends with
a rerun that must give the same bits.

Set DCVIC_TEST_RATIOS=<file> to have the worst error / bound per family and regime, and the fused-statistics table, written there."""
import pytest
import torch

import infer_kernels_ref as R
from kernel_bounds import DEV, FEATURE_REGIMES, U, cpu64, ratios_mark, regime, rnd, view_on_device, within, write_ratios

pytestmark = pytest.mark.gpu
EXTRA = {}                        # further records for the ratios file


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    mark = ratios_mark()
    yield
    write_ratios(EXTRA, since=mark)


def O():
    from dc_vic_amd import ops
    return ops


def dev_view(t, view):
    return t.to(DEV) if view is None else view_on_device(t, *view)


# ------------------------------------------------------------------------------------------------ GroupNorm forward
@pytest.mark.parametrize("c", R.GN_CASES, ids=lambda c: "{path}_N{N}_C{C}_{H}x{W}_g{groups}".format(**c))
def test_groupnorm_forward(c):
    """Derived.  Statistics in fp64 inside the kernel, then mean and var rounded to fp32, rstd = 1 / sqrtf(var + eps) and
    ((x - mean) rstd gamma + beta): about 8 roundings relative to e_xh |gamma| + |beta| (tests/test_gpu_train_kernels.py gn_ref's
    magnitudes), k = 16 as there; swish adds its own roundings relative to |y| and carries h's error with |swish'| <= 1.1.
    Without swish into a fresh map, with swish into a channel slice of a wider map (out=)."""
    ops = O()
    N, Cc, H, W, groups = c["N"], c["C"], c["H"], c["W"], c["groups"]
    eps = 1e-6
    gamma, beta = rnd(Cc, seed=3) + 1, rnd(Cc, seed=4)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    for name in FEATURE_REGIMES:
        x = regime(name, (N, Cc, H, W), seed=7)
        for swish in (False, True):
            ref, _, _, _, terms = R.gn_forward64(x, gamma, beta, groups, eps, swish)
            outs = []
            for view in R.GN_VIEWS:
                xd = dev_view(x, view)
                out = None
                if swish:
                    wide = torch.full((N, Cc + 5, H, W), float("nan"), device=DEV)
                    out = wide[:, 3:3 + Cc]
                y = ops.groupnorm(xd, gd, bd, groups, eps, ops.ACT_SWISH if swish else ops.ACT_NONE, out=out)
                within(f"groupnorm/{name}", y, ref, 16 * U * terms, f"{c['path']} swish={swish} view={view}")
                if swish:
                    assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, 3 + Cc:]).all(), "wrote outside the channel slice"
                outs.append(y.clone())
            # dense and the aligned view: the same bits (one reduction order); rerun: the same bits
            assert torch.equal(outs[0], outs[1]), "groupnorm depends on the batch stride"
            again = ops.groupnorm(dev_view(x, None), gd, bd, groups, eps, ops.ACT_SWISH if swish else ops.ACT_NONE)
            assert torch.equal(again, outs[0]), "groupnorm not reproducible"


# ------------------------------------------------------------------------------------------------ GroupNorm from fused statistics
@pytest.mark.parametrize("ups", [False, True], ids=["wino44", "wino44_ups"])
def test_groupnorm_from_fused_statistics(ups):
    """The forced F(4x4) (and F(4x4)-upsample) convolution hands its epilogue's partial sums to GroupNorm (part=): ragged 40 x 72 output
    (3 x 3 tiles, the last row and column partial), Cout = 160.  The residual is shifted per group so that the stored map's
    |mean| / std is 0, 3, 10, 30, 100.  Against the two-pass kernel on the same map the existing 2e-6 of the maximum must hold up to
    ratio 10; every ratio keeps the derived bound of test_groupnorm_forward plus the statistics term: the partials are fp32 chains of
    32 terms and 4 shuffle levels, so S and Q carry up to 36 U of their magnitudes.  The mean then moves by up to 36 U E|x|, which is
    36 U E|x| rstd <= 36 U E[x^2] / var of xh; var = Q/L - mean^2 moves by up to 36 U E[x^2] from Q and half as much again with the
    mean's share, and rstd by half of that relative to var: 0.75 * 36 U E[x^2] / var of |xh|.  Together (1 + 0.75 |xh|) * 36 U
    E[x^2] / var, times |gamma| and swish's slope (<= 1.1).  A worst-case term: every rounding of the chain at its limit and in the
    same direction, so the measured error sits far below it; the sharper statement for ratios up to 10 is the 2e-6 above."""
    ops = O()
    N, Cin, Cout, groups = 2, 64, 160, 32
    H, W = (20, 36) if ups else (40, 72)
    Ho, Wo = 40, 72
    x = rnd(N, Cin, H, W, seed=95).to(DEV)
    w = rnd(Cout, Cin, 3, 3, seed=96, scale=(Cin * 9) ** -0.5).to(DEV)
    b = rnd(Cout, seed=97, scale=0.5).to(DEV)
    r0 = rnd(N, Cout, Ho, Wo, seed=98)
    plan = ops.ConvPlan(w, b, "conv", pad=(1, 1), upsample=ups)
    plan.wino = plan.wino44 = "force"
    gamma, beta = rnd(Cout, seed=99) + 1.0, rnd(Cout, seed=100, scale=0.3)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y0 = cpu64(plan(x, act=ops.ACT_LRELU02, res=r0.to(DEV))).reshape(N, groups, -1)
    m0, s0 = y0.mean(-1), y0.std(-1, unbiased=False)
    table = {}
    for ratio in R.FUSED_RATIOS:
        shift = (ratio * s0 - m0).float()                               # per (image, group)
        r = (r0 + shift.repeat_interleave(Cout // groups, 1)[:, :, None, None]).to(DEV)
        y = plan(x, act=ops.ACT_LRELU02, res=r, gn_stats=True)
        part, n_pt = plan.last_gn_part
        assert n_pt == 9 and tuple(part.shape) == (N, Cout, n_pt, 2)
        yc = y.cpu()
        yg = yc.double().reshape(N, groups, -1)
        got_ratio = (yg.mean(-1).abs() / yg.std(-1, unbiased=False))
        assert float((got_ratio - ratio).abs().max()) < 0.01 * max(ratio, 1), (ratio, got_ratio)
        two_pass = ops.groupnorm(y, gd, bd, groups, 1e-6, ops.ACT_SWISH)
        fused = ops.groupnorm(y, gd, bd, groups, 1e-6, ops.ACT_SWISH, part=(part, n_pt))
        rel = float((two_pass - fused).abs().max()) / float(two_pass.abs().max())
        table[str(ratio)] = rel
        print(f"fused statistics {'wino44_ups' if ups else 'wino44'} |mean|/std = {ratio}: {rel:.3g} of the maximum against the two-pass kernel")
        ref, _, xh, ex2_var, terms = R.gn_forward64(yc, gamma, beta, groups, 1e-6, True)
        stat = 36 * U * ex2_var * (1 + 0.75 * xh.abs()) * gamma.double().abs()[:, None, None] * 1.1
        within(f"groupnorm_fused/ratio{ratio}", fused, ref, 16 * U * terms + stat, f"ups={ups}")
        within(f"groupnorm/ratio{ratio}", two_pass, ref, 16 * U * terms, f"two-pass ups={ups}")
        if ratio <= R.FUSED_HOLDS_TO:
            assert rel < R.FUSED_TOL, (ratio, rel)
        again = ops.groupnorm(y, gd, bd, groups, 1e-6, ops.ACT_SWISH, part=(part, n_pt))
        assert torch.equal(again, fused), "groupnorm from partials not reproducible"
    EXTRA["fused_statistics_vs_two_pass/" + ("wino44_ups" if ups else "wino44")] = table


# ------------------------------------------------------------------------------------------------ softmax over C
@pytest.mark.parametrize("Cc", R.SOFTMAX_CS)
def test_softmax_c(Cc):
    """Measured, against the one-pass max / sum restatement.  C < 4 leaves waves without a row (the -inf branch of the merge); P = 1,
    63, 64, 65, 257: one lane, a ragged block, exactly one, one more, five blocks.  N = 3."""
    ops = O()
    N = 3
    for P in R.SOFTMAX_PS:
        for name in R.SOFTMAX_REGIMES:
            x = R.softmax_input(name, N, Cc, P, seed=Cc + P)
            ref = R.softmax_c_onepass(x, torch.float64)
            bound, _ = R.measured_bound(R.softmax_c_onepass(x), ref)
            xd = x.to(DEV)
            ops.softmax_c_(xd, N, Cc, P)
            within(f"softmax_c/{name}", xd, ref, bound, f"C={Cc} P={P}")
            x2 = x.to(DEV)
            ops.softmax_c_(x2, N, Cc, P)
            assert torch.equal(x2, xd), "softmax_c not reproducible"


# ------------------------------------------------------------------------------------------------ bgemm
def _place(t, transposed, in_map, slot):
    """The logical [b, R, S] matrix t on the device, stored row-major or transposed, dense or as third `slot` of a [b, 3, R*S] map.
    -> (tensor that starts at the matrix, batch stride, row stride, column stride)."""
    b, Rr, S = t.shape
    m = (t.transpose(1, 2) if transposed else t).contiguous().reshape(b, Rr * S)
    rs, cs = (1, Rr) if transposed else (S, 1)
    if not in_map:
        return m.to(DEV), Rr * S, rs, cs
    buf = torch.full((b, 3, Rr * S), float("nan"), device=DEV)
    buf[:, slot] = m.to(DEV)
    return buf[:, slot], 3 * Rr * S, rs, cs


def _bgemm(pattern, A, B, alpha):
    ops = O()
    at, bt, amap, bmap, cmap = R.GEMM_PATTERNS[pattern]
    b, M, K = A.shape
    N = B.shape[2]
    Ad, a_bs, a_ms, a_ks = _place(A, at, amap, 1)
    Bd, b_bs, b_ks, b_ns = _place(B, bt, bmap, 0)
    if cmap:
        cbuf = torch.full((b, 3, M * N), float("nan"), device=DEV)
        Cd, c_bs = cbuf[:, 2], 3 * M * N
    else:
        cbuf = torch.full((b, M * N), float("nan"), device=DEV)
        Cd, c_bs = cbuf, M * N
    ops.bgemm(Ad, (a_bs, a_ms, a_ks), Bd, (b_bs, b_ks, b_ns), Cd, (c_bs, N), b, M, N, K, alpha=alpha)
    if cmap:
        assert torch.isnan(cbuf[:, :2]).all(), "bgemm wrote outside its third of the map"
    return Cd.reshape(b, M, N).clone()


@pytest.mark.parametrize("pattern", list(R.GEMM_PATTERNS))
def test_bgemm_stride_patterns(pattern):
    """Every (M, N) of {1, 63, 64, 65, 150}^2 with K cycling through {1, 15, 16, 17, 150} (each K meets each M and each N), batch 2,
    alpha = 0.37, operands laid out as the call site lays them out.  Sums: measured, against one sequential fp32 chain over k.
    Epilogue: derived, k = 1: C = fl(alpha * acc) is one rounding of the product, checked against alpha times the alpha = 1 result
    of the same launch geometry."""
    alpha = 0.37
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    for im, M in enumerate(R.GEMM_SIZES):
        for jn, N in enumerate(R.GEMM_SIZES):
            K = R.GEMM_KS[(im + jn) % len(R.GEMM_KS)]
            A, B = regime("offset", (2, M, K), seed=M * 7 + K), regime("normal", (2, K, N), seed=N * 5 + K)
            ref, _ = R.gemm_ref64(A, B, alpha)
            bound, _ = R.measured_bound(R.gemm_chain(A, B, alpha), ref)
            got = _bgemm(pattern, A, B, alpha)
            within(f"bgemm/{pattern}", got, ref, bound, f"M={M} N={N} K={K}")
            one = _bgemm(pattern, A, B, 1.0)
            prod = a32 * cpu64(one)
            within("bgemm/epilogue", got, prod, 1 * U * prod.abs(), f"{pattern} M={M} N={N} K={K}")
            assert torch.equal(_bgemm(pattern, A, B, alpha), got), "bgemm not reproducible"


def test_bgemm_large_batch_takes_the_128_tile_and_equals_the_item_alone():
    """batch 64 of 256 x 256 x 32: 4 tiles of 128 x 128 per item x 64 >= the CU count, so the 128-tile kernel runs; one item alone runs
    on 64-tiles.  One k-ordered chain per output either way: bit-identical.  Measured bound against the chain on item 5."""
    ops = O()
    A, B = regime("swish", (64, 256, 32), seed=1), regime("normal", (64, 32, 256), seed=2)
    Ad, Bd = A.to(DEV), B.to(DEV)
    out = torch.full((64, 256, 256), float("nan"), device=DEV)
    ops.bgemm(Ad, (256 * 32, 32, 1), Bd, (32 * 256, 256, 1), out, (256 * 256, 256), 64, 256, 256, 32, alpha=0.5)
    one = torch.full((1, 256, 256), float("nan"), device=DEV)
    ops.bgemm(Ad[5:6], (256 * 32, 32, 1), Bd[5:6], (32 * 256, 256, 1), one, (256 * 256, 256), 1, 256, 256, 32, alpha=0.5)
    assert torch.equal(one[0], out[5]), "bgemm depends on the tile size / the batch"
    ref, _ = R.gemm_ref64(A[5:6], B[5:6], 0.5)
    bound, _ = R.measured_bound(R.gemm_chain(A[5:6], B[5:6], 0.5), ref)
    within("bgemm/tile128", out[5:6], ref, bound)
    again = torch.full((64, 256, 256), float("nan"), device=DEV)
    ops.bgemm(Ad, (256 * 32, 32, 1), Bd, (32 * 256, 256, 1), again, (256 * 256, 256), 64, 256, 256, 32, alpha=0.5)
    assert torch.equal(again, out)


# ------------------------------------------------------------------------------------------------ fused attention
def _attn(qkv_d, in_bs, Cc, N, HW, out, out_bs, force_nw=0):
    """dcvic_attn_fused_f32 on a q | k | v map whose images lie in_bs floats apart."""
    from dc_vic_amd._lib import check, lib
    base = qkv_d.data_ptr()
    check(lib().dcvic_attn_fused_f32(base, base + 4 * Cc * HW, base + 8 * Cc * HW, in_bs, out.data_ptr(), out_bs, N, Cc, HW,
                                     float(int(Cc) ** (-0.5)), force_nw, torch.cuda.current_stream().cuda_stream), "attn_fused")
    return out


@pytest.mark.parametrize("Cc,hw,N", R.ATTN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_attn_fused(Cc, hw, N):
    """Measured, against the online softmax over 64-key tiles restated in fp32 (scores as one chain over the channels, the value
    product as one chain over the keys), at the queries R.attn_queries picks.  HW = 64 is one key tile (nkt = 1); peak_last leaves
    the alpha != 1 rescale as the last thing that happens to the output; N * HW / 64 is a multiple of 8 for some cases (the XCD
    remap) and not for others.  Each regime runs through ops.attn_fused (dense) and through the C ABI with the map as a batch-strided
    slice of a larger buffer and out= a batch-strided, misaligned view: the same bits.  NW = 2 against NW = 4 (C < 512) and an image
    alone against the same image in its batch: the same bits."""
    ops = O()
    H, W = hw
    HW = H * W
    qs = R.attn_queries(HW)
    for name in R.ATTN_REGIMES:
        qkv = R.attn_inputs(name, N, Cc, HW, seed=Cc + HW)
        ref = R.attn_ref64(qkv, Cc, qs)
        bound, _ = R.measured_bound(R.attn_online(qkv, Cc, qs), ref)
        qd = qkv.reshape(N, 3 * Cc, H, W).to(DEV)
        out = ops.attn_fused(qd, Cc)
        within(f"attn_fused/{name}", out.reshape(N, Cc, HW)[:, :, qs.to(DEV)], ref, bound, f"C={Cc} HW={HW} N={N}")
        # the map as a slice of a larger buffer (in_bs != 3 C HW), out= a strided misaligned view (out_bs != C HW)
        in_bs = 3 * Cc * HW + 64
        big = torch.full((8 + N * in_bs,), float("nan"), device=DEV)
        qv = big.as_strided((N, 3 * Cc * HW), (in_bs, 1), 8)
        qv.copy_(qd.reshape(N, -1))
        out_bs = Cc * HW + 3
        obuf = torch.full((1 + N * out_bs,), float("nan"), device=DEV)
        ov = obuf.as_strided((N, Cc * HW), (out_bs, 1), 1)
        _attn(qv, in_bs, Cc, N, HW, ov, out_bs)
        assert torch.equal(ov.reshape(N, Cc, H, W), out), f"{name}: attn_fused depends on the batch strides"
        assert torch.isnan(obuf[0]) and torch.isnan(obuf.as_strided((N, 3), (out_bs, 1), 1 + Cc * HW)).all(), "wrote between the images"
        if Cc != 512:
            o2, o4 = ops.attn_fused(qd, Cc, force_nw=2), ops.attn_fused(qd, Cc, force_nw=4)
            assert torch.equal(o2, o4) and torch.equal(o2, out), f"{name}: NW = 2 and NW = 4 differ"
        n = N - 1
        assert torch.equal(ops.attn_fused(qd[n:n + 1].contiguous(), Cc)[0], out[n]), f"{name}: an image alone differs from the batch"
        assert torch.equal(ops.attn_fused(qd, Cc), out), "attn_fused not reproducible"


# ------------------------------------------------------------------------------------------------ Swin window attention
@pytest.mark.parametrize("hw", R.SWIN_MAPS, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("Cc", R.SWIN_CS)
def test_swin_attn(Cc, hw):
    """Measured, against the kernel's arithmetic restated in fp32 (score chain over the 16 channels of a head, bias, -100 mask, one
    max / sum pass, the output as one chain over the 64 tokens).  Heads 2, 6, 8; one window, a row of three, 3 x 2; shift 0 and 4;
    N = 1 and 3; bias tables of std 0.5 and 8; scores of std 1 and 20."""
    ops = O()
    H, W = hw
    heads = Cc // 16
    for shift in (0, 4):
        for N in (1, 3):
            for tstd in (0.5, 8.0):
                table = rnd(225, heads, seed=3, scale=tstd)
                for name in R.SWIN_REGIMES:
                    qkv = R.swin_inputs(name, N, Cc, H, W, seed=Cc + H + W)
                    ref = R.swin_forward(qkv, table, heads, shift, torch.float64)
                    bound, _ = R.measured_bound(R.swin_forward(qkv, table, heads, shift), ref)
                    out = ops.swin_attn(qkv.to(DEV), table.to(DEV), heads, 8, shift)
                    within(f"swin_attn/{name}", out, ref, bound, f"C={Cc} {H}x{W} shift={shift} N={N} table std {tstd}")
                    assert torch.equal(ops.swin_attn(qkv.to(DEV), table.to(DEV), heads, 8, shift), out), "swin_attn not reproducible"


# ------------------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("shape", [R.EW_BIG, R.EW_SMALL], ids=["grid_stride", "ragged"])
def test_elementwise(shape):
    """ew_kernel above its grid-stride threshold (C*HW > 2048 * 256: a second pass) and on 385 elements, dense and through batch-strided
    misaligned views.  add, ReLU, LeakyReLU, absmax: exact.  sft = a + w (a b + c): four roundings, derived k = 4 on |a| + |w| (|a b| + |c|).
    add_mul_sigmoid = a + b / (1 + expf(-c)): expf, the sum, the division, the product, the sum: derived k = 8 on |a| + |b| sigmoid(c).
    swish, GELU, sigmoid, tanh / 2: measured, against the same expression in fp32 on the CPU."""
    ops = O()
    a, b, c = regime("offset", shape, 1), regime("outlier", shape, 2), regime("normal", shape, 3) * 3
    A, B, Cd = a.double(), b.double(), c.double()
    w = 0.37
    wf = float(torch.tensor(w, dtype=torch.float32))
    for view in (None, (3, 1)):
        ad, bd, cd = dev_view(a, view), dev_view(b, view and (5, 3)), dev_view(c, view and (1, 2))
        out = dev_view(torch.zeros(shape), view and (7, 1)) if view else None
        y = ops.add(ad, bd, out=out)
        assert torch.equal(y.cpu(), a + b), "add"
        y = ops.activation(ad, ops.ACT_RELU)
        assert torch.equal(y.cpu(), torch.relu(a)), "relu"
        y = ops.activation(ad, ops.ACT_LRELU02)
        assert torch.equal(y.cpu(), R.act(R.ACT_LRELU02, a)), "leaky relu"
        assert torch.equal(ops.activation(ad, ops.ACT_NONE).cpu(), a), "identity"
        assert torch.equal(ops.absmax(bd).cpu(), b.abs().amax((1, 2, 3))), "absmax"      # 32 workgroups per image / one
        y = ops.sft(ad, bd, cd, w=w, out=out)
        within("sft", y, A + wf * (A * B + Cd), 4 * U * (A.abs() + abs(wf) * ((A * B).abs() + Cd.abs())), f"view={view}")
        y = ops.add_mul_sigmoid(ad, bd, cd, out=out)
        within("add_mul_sigmoid", y, A + B * torch.sigmoid(Cd), 8 * U * (A.abs() + B.abs() * torch.sigmoid(Cd)), f"view={view}")
        first = y.clone()
        for actn, aname in ((ops.ACT_SWISH, "swish"), (ops.ACT_GELU, "gelu"), (ops.ACT_SIGMOID, "sigmoid"), (ops.ACT_HALF_TANH, "half_tanh")):
            ref = R.act(actn, Cd)
            bound, _ = R.measured_bound(R.act(actn, c), ref)
            within(f"activation/{aname}", ops.activation(cd, actn), ref, bound, f"view={view}")
        assert torch.equal(ops.add_mul_sigmoid(ad, bd, cd), first), "ew not reproducible"


@pytest.mark.parametrize("shape", [R.PLANE_BIG, R.PLANE_SMALL], ids=["grid_stride", "ragged"])
def test_chan_affine_and_plane_copies(shape):
    """chan_affine, copy_planes (crop and reflect pad) and copy_window with more than 64 * 256 pixels per plane (a second pass per
    workgroup) and on 7 x 11 planes.  chan_affine = x (1 + scale) + shift (+ add): the rounding of 1 + scale, the product, the sums:
    derived k = 4 on |x| (1 + |scale|) + |shift| + |add|; vectors of batch 1 and batch N.  The copies are exact."""
    ops = O()
    N, Cc, H, W = shape
    x, ad = regime("offset", shape, 4), regime("swish", shape, 5)
    X, AD = x.double(), ad.double()
    for view in (None, (3, 1)):
        xd, add_d = dev_view(x, view), dev_view(ad, view and (2, 3))
        for nb in (1, N):
            sc, sh = rnd(nb, Cc, seed=6), rnd(nb, Cc, seed=7, scale=2.0)
            S, T = sc.double()[:, :, None, None], sh.double()[:, :, None, None]
            for use_add in (False, True):
                y = ops.chan_affine(xd, sc.to(DEV), sh.to(DEV), add_=add_d if use_add else None)
                ref = X * (1 + S) + T + (AD if use_add else 0)
                mag = X.abs() * (1 + S.abs()) + T.abs() + (AD.abs() if use_add else 0)
                within("chan_affine", y, ref, 4 * U * mag, f"{shape} batch {nb} add={use_add} view={view}")
        assert torch.equal(ops.chan_affine(xd, sc.to(DEV), sh.to(DEV), add_=add_d), y), "chan_affine not reproducible"
        # crop (copy_planes) and reflect pad
        assert torch.equal(ops.crop(xd, H - 1, W - 1).cpu(), x[:, :, :H - 1, :W - 1]), "crop"
        ph, pw = min(5, H - 1), min(6, W - 1)
        want = torch.nn.functional.pad(x, (0, pw, 0, ph), mode="reflect")
        got = ops.pad_reflect(xd, ph, pw)
        assert torch.equal(got.cpu(), want), "pad_reflect"
        assert torch.equal(ops.pad_reflect(xd, ph, pw), got)
        # copy_window: a window of one strided buffer into a window of another
        src = torch.full((N, Cc + 1, H + 3, W + 5), float("nan"), device=DEV)
        src[:, 1:, 2:2 + H, 1:1 + W] = xd
        dst = torch.full((N, Cc, H + 1, W + 2), float("nan"), device=DEV)
        ops.copy_window(dst[:, :, 1:, 2:], src[:, 1:, 2:2 + H, 1:1 + W])
        assert torch.equal(dst[:, :, 1:, 2:].cpu(), x), "copy_window"
        assert torch.isnan(dst[:, :, 0]).all() and torch.isnan(dst[:, :, :, :2]).all(), "copy_window wrote outside its window"


@pytest.mark.parametrize("shape,crop", [(R.CROP_BIG, R.CROP_BIG_OUT), (R.CROP_SMALL, R.CROP_SMALL_OUT)], ids=["grid_stride", "ragged"])
def test_crop_clamp(shape, crop):
    """crop + clamp(-1, 1) and the uint8 HWC form ((v + 1) / 2 * 255 truncated) with more than 1024 * 256 elements per image (a second
    pass) and on a 7 x 10 crop: each a few single fp32 roundings that torch on the CPU repeats in the same order -- exact."""
    ops = O()
    x = regime("normal", shape, 8) * 0.8
    x[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, 0.0, 0.999999])
    h, w = crop
    want = x[:, :, :h, :w].clamp(-1, 1)
    want8 = ((want + 1.0) / 2.0 * 255.0).to(torch.int32).to(torch.uint8).permute(0, 2, 3, 1)
    for view in (None, (3, 1)):
        xd = dev_view(x, view)
        y, y8 = ops.crop_clamp(xd, h, w, want_u8=True)
        assert torch.equal(y.cpu(), want), "crop_clamp float"
        assert torch.equal(y8.cpu(), want8), "crop_clamp uint8"
        assert torch.equal(ops.crop_clamp(xd, h, w), y)


# ------------------------------------------------------------------------------------------------ Winograd routes off N(0, 1)
@pytest.mark.parametrize("name", R.WINO_REGIMES)
@pytest.mark.parametrize("route", list(R.WINO_ROUTE_CASES))
def test_wino_routes_off_normal_inputs(route, name):
    """The four forced Winograd routes at one ragged shape each (partial tiles in both directions, Cout = 96) under the offset, outlier
    and swish regimes and under offset with weights that sum to zero over Cin, against fp64: the bounds the existing tests state for
    N(0, 1) data -- 1.2e-5 of the output's maximum for F(4x4) (tests/test_gpu_kernels.py test_wino44_conv3x3, test_gpu_wino44_ups.py),
    2e-6 for F(2x2), and for the plain F(2x2) also test_wino_conv3x3's 4 x the direct kernel's own error + 1e-7."""
    ops = O()
    Cin, Cout, H, W, N, ups, res = R.WINO_ROUTE_CASES[route]
    x, w, b, r = R.wino_inputs(name, route, seed=31)
    ref = R.conv_ref64(x, w, b, r, ups)
    plan = ops.ConvPlan(w.to(DEV), b.to(DEV), "conv", pad=(1, 1), upsample=ups)
    plan.wino = "force"
    if route.startswith("wino44"):
        plan.wino44 = "force"
    xd, rd = x.to(DEV), None if r is None else r.to(DEV)
    ops.kernel_events_start()
    y = plan(xd, res=rd)
    torch.cuda.synchronize()
    ev = list(ops.kernel_events_stop())
    assert ev == [f"conv3x3_{route}_kernel(ConvKArgs)"], ev
    sc = float(ref.abs().max())
    err = float((cpu64(y) - ref).abs().max()) / sc
    print(f"{route} under {name}: {err:.3g} of the output's maximum")
    within(f"{route}/{name}", y, ref, R.WINO_BOUND[route] * sc)
    if route == "wino":
        direct = ops.ConvPlan(w.to(DEV), b.to(DEV), "conv", pad=(1, 1))
        ed = float((cpu64(direct(xd, res=rd)) - ref).abs().max()) / sc
        print(f"direct under {name}: {ed:.3g}")
        assert err < 4 * ed + 1e-7, (err, ed)
    assert torch.equal(plan(xd, res=rd), y), f"{route} not reproducible"
