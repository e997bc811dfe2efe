"""Training-step kernels (csrc/train.hip) called directly, at the trainer's shapes and at the edges of their index arithmetic,
against torch fp64 on the CPU.

Every comparison is per element.  A reduction's bound is k * 2^-24 * sum|terms|, with sum|terms| computed in fp64 by the test and
k stated next to each check from how the kernel accumulates: fp64 accumulation inside (chan_reduce, the GroupNorm statistics and
channel sums, the loss partials) leaves the fp32 roundings of the operands and the result; an fp32 chain of L additions can lose
up to about L * 2^-24 of the sum of the magnitudes it has added.  Operations that the kernels restate exactly (data movement,
single roundings) are compared with torch.equal against an fp32 CPU restatement in the same order, and the reductions that
claim determinism are rerun and compared bit for bit.

Set DCVIC_TEST_RATIOS=<file> to have the worst error / bound of each kernel family written there as JSON."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_bounds import DEV, U, TINY, cpu64, rnd, urnd, view_on_device, within, ratios_mark, write_ratios  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    mark = ratios_mark()
    yield
    write_ratios(since=mark)


def K():
    from dc_vic_amd.train import kernels
    return kernels


def L():
    from dc_vic_amd._lib import lib
    return lib()


def wgrad_slabs(N, M, Cx, KH, KW, Hg):
    s = C.c_int(0)
    L().dcvic_conv_wgrad_workspace_floats(N, M, Cx, KH, KW, Hg, C.byref(s))
    return s.value


# ------------------------------------------------------------------------------------------------ conv weight gradient
def wgrad_ref(G, X, KH, KW, s, p, rows=None):
    """fp64 dW[m][c][ky][kx] = sum_{n,oy,ox} G[n][m][oy][ox] X[n][c][oy*s+ky-p][ox*s+kx-p] (zero outside X) and sum|terms|."""
    N, M, Hg, Wg = G.shape
    Cx, Hx, Wx = X.shape[1:]
    if rows is not None:
        G = G[:, rows]
    Mr = G.shape[1]
    ref = torch.zeros(Mr, Cx, KH, KW, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    hp, wp = (Hg - 1) * s + KH, (Wg - 1) * s + KW          # padded extent every read falls into
    for n in range(N):
        g = G[n].double().reshape(Mr, -1)
        xp = F.pad(X[n].double(), (p, max(0, wp - Wx - p), p, max(0, hp - Hx - p)))
        for ky in range(KH):
            for kx in range(KW):
                xs = xp[:, ky:ky + (Hg - 1) * s + 1:s, kx:kx + (Wg - 1) * s + 1:s].reshape(Cx, -1)
                ref[:, :, ky, kx] += g @ xs.T
                mag[:, :, ky, kx] += g.abs() @ xs.abs().T
    return ref, mag


# N, M, Cx, Hg, Wg, KH, KW, stride, pad, views (G / X batch-stride extra, storage offset), accumulate
WGRAD_CASES = [
    dict(N=1, M=1, Cx=1, Hg=1, Wg=7, KH=1, KW=1, s=1, p=0, view=None, acc=False),
    dict(N=8, M=72, Cx=3, Hg=2, Wg=9, KH=2, KW=2, s=2, p=0, view=(3, 1), acc=True),
    dict(N=8, M=128, Cx=31, Hg=5, Wg=40, KH=3, KW=3, s=1, p=1, view=(4 * 40, 4), acc=False),     # aligned view: a_vec
    dict(N=1, M=129, Cx=33, Hg=17, Wg=17, KH=4, KW=4, s=2, p=1, view=None, acc=True),
    dict(N=8, M=256, Cx=64, Hg=17, Wg=20, KH=5, KW=5, s=1, p=2, view=(20, 1), acc=False),       # misaligned view, Wg % 4 == 0
    dict(N=1, M=72, Cx=33, Hg=5, Wg=11, KH=5, KW=5, s=3, p=2, view=None, acc=False),
    dict(N=8, M=129, Cx=1, Hg=17, Wg=3, KH=3, KW=3, s=3, p=0, view=(1, 0), acc=True),
    dict(N=8, M=256, Cx=31, Hg=1, Wg=64, KH=3, KW=3, s=2, p=1, view=None, acc=False),
    dict(N=2, M=64, Cx=5, Hg=17, Wg=33, KH=1, KW=3, s=1, p=1, view=None, acc=False),
    dict(N=1, M=33, Cx=64, Hg=2, Wg=31, KH=5, KW=2, s=2, p=2, view=(2, 3), acc=True),
    dict(N=2, M=64, Cx=16, Hg=5, Wg=13, KH=3, KW=3, s=4, p=2, view=None, acc=False),            # stride 4
    dict(N=1, M=72, Cx=33, Hg=3, Wg=9, KH=5, KW=5, s=4, p=1, view=(5, 1), acc=True),            # stride 4, largest LDS image
]


def _wgrad_run(c, seed):
    N, M, Cx, Hg, Wg, KH, KW, s, p = (c[k] for k in ("N", "M", "Cx", "Hg", "Wg", "KH", "KW", "s", "p"))
    Hx, Wx = max(1, (Hg - 1) * s + KH - 2 * p + (seed % s)), max(1, (Wg - 1) * s + KW - 2 * p)
    G, X = rnd(N, M, Hg, Wg, seed=seed), rnd(N, Cx, Hx, Wx, seed=seed + 1)
    if c["view"]:
        Gd, Xd = view_on_device(G, *c["view"]), view_on_device(X, c["view"][0] + 2, c["view"][1])
    else:
        Gd, Xd = G.to(DEV), X.to(DEV)
    dW0 = rnd(M, Cx, KH, KW, seed=seed + 2) if c["acc"] else torch.zeros(M, Cx, KH, KW)
    dW = dW0.to(DEV)
    K().conv_wgrad(Gd, Xd, dW, KH, KW, s, p, accumulate=c["acc"])
    return G, X, Gd, Xd, dW0, dW


@pytest.mark.parametrize("c", WGRAD_CASES, ids=lambda c: "N{N}_M{M}_C{Cx}_H{Hg}x{Wg}_k{KH}x{KW}_s{s}_p{p}".format(**c))
def test_conv_wgrad(c):
    """fp32 MFMA chains over each slab's pixels (rows_per_slab * Wg, padded to 32-pixel chunks), then the slabs (and the
    accumulated dW) added in fp32 in slab order: k = chunk-padded pixels per slab + slabs + 4."""
    G, X, Gd, Xd, dW0, dW = _wgrad_run(c, seed=11)
    N, M, Cx, Hg, Wg, KH, KW = (c[k] for k in ("N", "M", "Cx", "Hg", "Wg", "KH", "KW"))
    ref, mag = wgrad_ref(G, X, KH, KW, c["s"], c["p"])
    slabs = wgrad_slabs(N, M, Cx, KH, KW, Hg)
    rows = -(-Hg // (slabs // N))
    k = rows * (-(-Wg // 32) * 32) + slabs + 4
    within("conv_wgrad", dW, ref + dW0.double(), k * U * (mag + dW0.double().abs()), str(c))
    # rerun, and rerun after a larger call left the grow-only workspace dirty (and after it was filled with NaN): same bits
    first = dW.clone()
    for dirty in ("rerun", "larger", "nan"):
        if dirty == "larger":
            big = rnd(8, 256, 32, 32, seed=5).to(DEV)
            K().conv_wgrad(big, big, torch.zeros(256, 256, 3, 3, device=DEV), 3, 3, 1, 1, accumulate=False)
        elif dirty == "nan":
            ws = K()._WS[("wgrad", str(Gd.device))]
            ws.fill_(float("nan"))
        dW2 = dW0.to(DEV)
        K().conv_wgrad(Gd, Xd, dW2, KH, KW, c["s"], c["p"], accumulate=c["acc"])
        assert torch.equal(dW2, first), f"conv_wgrad not reproducible ({dirty})"


def test_conv_wgrad_trained_shape_full_size():
    """A trained 3x3 layer at full size: N = 8, 128 -> 128 channels, 256 x 256 maps (the slab split then gives long chains).
    Rows 0, 31, 32 and 127 (first / last row of a wave and of the 128-row block) checked against fp64; k as in test_conv_wgrad."""
    N, M, Cx, H, W = 8, 128, 128, 256, 256
    G, X = rnd(N, M, H, W, seed=21), rnd(N, Cx, H, W, seed=22)
    dW = torch.full((M, Cx, 3, 3), float("nan"), device=DEV)
    K().conv_wgrad(G.to(DEV), X.to(DEV), dW, 3, 3, 1, 1, accumulate=False)
    rows = [0, 31, 32, 127]
    ref, mag = wgrad_ref(G, X, 3, 3, 1, 1, rows=rows)
    slabs = wgrad_slabs(N, M, Cx, 3, 3, H)
    k = -(-H // (slabs // N)) * W + slabs + 4
    within("conv_wgrad", dW[rows], ref, k * U * mag, "full size")


# ------------------------------------------------------------------------------------------------ per-channel reductions
@pytest.mark.parametrize("HW", [1, 255, 256, 257, 65536])
def test_chan_reduce_and_sum_rows(HW):
    """chan_reduce accumulates the exact fp32 x fp32 products in fp64 and rounds once: bound = 2^-24 |ref| + L * 2^-53 sum|terms|
    (the fp64 chain).  sum_rows adds rows in fp32 in ascending order: equal to the same chain on the CPU."""
    H, W = (256, 256) if HW == 65536 else (1, HW)
    N, Cc = 3, 5
    a, b = rnd(N, Cc, H, W, seed=HW), rnd(N, Cc, H, W, seed=HW + 1)
    ad, bd = view_on_device(a, 2 * HW, 1), view_on_device(b, 7, 0)      # batch-strided, one misaligned
    for use_b in (False, True):
        out = K().chan_reduce(ad, bd if use_b else None)
        t = a.double() * (b.double() if use_b else 1.0)
        ref = t.sum((2, 3))
        mag = t.abs().sum((2, 3))
        within("chan_reduce", out, ref, U * ref.abs() + HW * 2.0 ** -53 * mag, f"HW={HW} b={use_b}")
        # determinism: each image's partial is the same bits alone and in the batch
        for n in range(N):
            alone = K().chan_reduce(ad[n:n + 1], bd[n:n + 1] if use_b else None)
            assert torch.equal(alone[0], out[n]), "chan_reduce partial depends on the batch"
    # sum_rows over R rows of length HW * 3, with and without accumulate; one row is a copy / one addition
    for R in (1, 2, 9):
        x = rnd(R, 3 * HW, seed=R)
        o0 = rnd(3 * HW, seed=99)
        for acc in (False, True):
            o = o0.to(DEV)
            K().sum_rows(x.to(DEV), o, acc)
            s = o0.clone() if acc else torch.zeros(3 * HW)
            for r in range(R):
                s = s + x[r]
            assert torch.equal(o.cpu(), s), f"sum_rows R={R} acc={acc}"


# ------------------------------------------------------------------------------------------------ elementwise backward forms
def _act_grad64(act, v):
    from dc_vic_amd import ops
    if act == ops.ACT_RELU:
        return (v > 0).double()
    if act == ops.ACT_LRELU02:
        return torch.where(v > 0, 1.0, 0.2).double()
    if act == ops.ACT_SIGMOID:
        return v * (1 - v)
    if act == ops.ACT_HALF_TANH:
        return 0.5 * (1 - 4 * v * v)
    if act == ops.ACT_SWISH:
        s = torch.sigmoid(v)
        return s * (1 + v * (1 - s))
    if act == ops.ACT_GELU:
        return 0.5 * (1 + torch.erf(v / math.sqrt(2))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
    return torch.ones_like(v)


def test_ew_bwd_all_ops():
    """All 12 ops on 1155 elements (not a multiple of 256).  Single-rounding ops 6, 10, 11 equal the fp32 CPU restatement; the
    others are a few fp32 roundings of expf / erff / products: bound 8 * 2^-24 * (magnitude of the terms).  Activations whose
    derivative cancels (1 - s, erf near -1) are bounded by the absolute term |g| (1 + |x|)."""
    from dc_vic_amd import ops
    shape = (3, 5, 7, 11)
    g, a, b = rnd(*shape, seed=1), rnd(*shape, seed=2, scale=3.0), rnd(*shape, seed=3, scale=3.0)
    gd, ad, bd = g.to(DEV), a.to(DEV), b.to(DEV)
    G, A, B = g.double(), a.double(), b.double()
    w = 0.37
    wf = torch.tensor(w, dtype=torch.float32)
    # op 0: every activation; the output-referenced ones get outputs in their range, swish / GELU inputs up to |x| = 100
    wide = torch.cat([rnd(1155 - 15, seed=4, scale=4.0), torch.tensor([-100., -80., -30., -9., -5., -1e-3, 0., 1e-3, 5., 9., 30.,
                                                                       80., 100., -17.5, 17.5])]).reshape(shape)
    refs = {ops.ACT_NONE: a, ops.ACT_RELU: a, ops.ACT_LRELU02: a, ops.ACT_SWISH: wide, ops.ACT_GELU: wide,
            ops.ACT_SIGMOID: torch.sigmoid(a), ops.ACT_HALF_TANH: 0.5 * torch.tanh(a)}
    for act, v in refs.items():
        out = K().ew(0, gd, v.to(DEV), act=act)
        V = v.double()
        within("ew_bwd", out, G * _act_grad64(act, V), 8 * U * G.abs() * (1 + V.abs()), f"op 0 act {act}")
    S = torch.sigmoid(B)
    cases = {
        1: (G * A, 2 * U * (G * A).abs()),
        2: (G * torch.sigmoid(A), 8 * U * G.abs()),
        3: (G * A * S * (1 - S), 12 * U * (G * A).abs() * S),
        4: (G * (1 + w * A), 4 * U * G.abs() * (1 + abs(w) * A.abs())),
        5: (w * G * A, 4 * U * (w * G * A).abs()),
        8: (2 * w * (A - B), 4 * U * abs(2 * w) * (A.abs() + B.abs())),
    }
    for op, (ref, bound) in cases.items():
        out = K().ew(op, gd, ad, bd, w=w)
        within("ew_bwd", out, ref, bound, f"op {op}")
    for t in (0, 1):                                   # op 9: BCE-with-logits gradient, target in `act`
        out = K().ew(9, None, ad, w=w, act=t)
        within("ew_bwd", out, w * (torch.sigmoid(A) - t), 8 * U * abs(w) * (1 + torch.sigmoid(A)), f"op 9 t={t}")
    # op 7: per-channel vector, per image (vec_bs = C) or shared (vec_bs = 0)
    for vec_bs in (0, 5):
        vec = rnd(3 if vec_bs else 1, 5, seed=7)
        out = K().ew(7, gd, vec.to(DEV), vec_bs=vec_bs)
        Vb = vec.double()[:, :, None, None].expand(3, 5, 1, 1) if vec_bs else vec.double()[0][None, :, None, None]
        within("ew_bwd", out, G * (1 + Vb), 2 * U * G.abs() * (1 + Vb.abs()), f"op 7 vec_bs={vec_bs}")
    # exact ops, and 10 / 11 in place (the trainer's K.ew(10, None, gw, tmp, out=gw) / K.ew(11, ..., out=flat))
    assert torch.equal(K().ew(6, gd, w=w).cpu(), wf * g)
    assert torch.equal(K().ew(10, None, ad, bd).cpu(), a + b)
    assert torch.equal(K().ew(11, None, ad, w=w).cpu(), a * wf)
    x = ad.clone()
    K().ew(10, None, x, bd, out=x)
    assert torch.equal(x.cpu(), a + b), "ew op 10 in place"
    x = ad.clone()
    K().ew(11, None, x, w=w, out=x)
    assert torch.equal(x.cpu(), a * wf), "ew op 11 in place"


# ------------------------------------------------------------------------------------------------ GroupNorm backward
def gn_ref(x, dy, gamma, beta, groups, eps, swish):
    """fp64: dx by autograd; per-image dgamma = sum dh * xh, dbeta = sum dh; the magnitudes the bounds are built from."""
    X, DY, Ga, Be = x.double(), dy.double(), gamma.double(), beta.double()
    Xr = X.clone().requires_grad_(True)
    y = F.group_norm(Xr, groups, Ga, Be, eps)
    if swish:
        y = y * torch.sigmoid(y)
    y.backward(DY)
    N, Cc, H, W = x.shape
    xg = X.reshape(N, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(xg.var(-1, unbiased=False, keepdim=True) + eps)
    xh = ((xg - mean) * rstd).reshape(N, Cc, H, W)
    h = xh * Ga[:, None, None] + Be[:, None, None]
    if swish:
        s = torch.sigmoid(h)
        dh = DY * s * (1 + h * (1 - s))
    else:
        dh = DY
    e_xh = xh.abs() + ((X.abs().reshape(N, groups, -1) + mean.abs()) * rstd).reshape(N, Cc, H, W)
    a_dh = DY.abs() * (1 + (h.abs() + Ga.abs()[:, None, None] * e_xh if swish else 0))
    return Xr.grad, (dh * xh).sum((2, 3)), dh.sum((2, 3)), xh, e_xh, a_dh, rstd.reshape(N, groups, 1)


GN_CASES = [  # N, C, HW, groups, swish, view (batch-stride extra, offset)
    dict(N=1, C=32, H=256, W=256, groups=32, swish=True, view=(64, 0)),        # channels per group 1, HW 65536
    dict(N=8, C=64, H=64, W=64, groups=32, swish=False, view=None),            # cpg 2, HW 4096 (8 passes of 512 threads)
    dict(N=2, C=176, H=7, W=9, groups=8, swish=True, view=(3, 1)),             # cpg 22, HW 63: scalar path
    dict(N=8, C=512, H=8, W=8, groups=8, swish=True, view=None),               # cpg 64, HW 64
    dict(N=2, C=128, H=64, W=64, groups=32, swish=True, view=(8, 1)),          # HW % 4 == 0 but misaligned: scalar path
    dict(N=1, C=64, H=8, W=8, groups=1, swish=False, view=(4, 4)),             # cpg 64, aligned view: vector path
]


@pytest.mark.parametrize("c", GN_CASES, ids=lambda c: "N{N}_C{C}_{H}x{W}_g{groups}_swish{swish}".format(**c))
def test_groupnorm_bwd(c):
    """Statistics and channel sums in fp64 from fp32 xh / dh: the per-term error is a few roundings of xh (relative to
    (|x| + |mean|) rstd) and of dh (relative to |dy| (1 + |h|)), so dgamma / dbeta: 16 * 2^-24 * sum of those magnitudes.  dx is
    rstd (dh gamma - (m1 + xh m2)) in fp32 from those: 16 * 2^-24 * rstd * (each term's magnitude + the group means')."""
    from dc_vic_amd import ops
    N, Cc, H, W, groups = c["N"], c["C"], c["H"], c["W"], c["groups"]
    eps = 1e-6
    x, dy = rnd(N, Cc, H, W, seed=1, scale=2.0) + 0.5, rnd(N, Cc, H, W, seed=2)
    gamma, beta = rnd(Cc, seed=3) + 1, rnd(Cc, seed=4)
    xd, dyd = (view_on_device(x, *c["view"]), view_on_device(dy, c["view"][0] + 4, c["view"][1])) if c["view"] else (x.to(DEV), dy.to(DEV))
    act = ops.ACT_SWISH if c["swish"] else ops.ACT_NONE
    dx, dg, db = K().groupnorm_bwd(xd, dyd, gamma.to(DEV), beta.to(DEV), groups, eps, act)
    rdx, rdg, rdb, xh, e_xh, a_dh, rstd = gn_ref(x, dy, gamma, beta, groups, eps, c["swish"])
    Ga = gamma.double().abs()[:, None, None]
    within("groupnorm_bwd dgamma/dbeta", dg, rdg, 16 * U * (a_dh * e_xh).sum((2, 3)), "dgamma")
    within("groupnorm_bwd dgamma/dbeta", db, rdb, 16 * U * a_dh.sum((2, 3)), "dbeta")
    Lg = Cc // groups * H * W
    m1 = (a_dh * Ga).reshape(N, groups, -1).sum(-1, keepdim=True) / Lg
    m2 = (a_dh * Ga * e_xh).reshape(N, groups, -1).sum(-1, keepdim=True) / Lg
    per = (a_dh * Ga).reshape(N, groups, -1) + m1 + e_xh.reshape(N, groups, -1) * m2
    within("groupnorm_bwd dx", dx, rdx, (16 * U * rstd * per).reshape(N, Cc, H, W), "dx")
    # rerun: same bits; each image alone: the same bits as in the batch
    dx2, dg2, db2 = K().groupnorm_bwd(xd, dyd, gamma.to(DEV), beta.to(DEV), groups, eps, act)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)
    n = N - 1
    dx1, dg1, db1 = K().groupnorm_bwd(xd[n:n + 1], dyd[n:n + 1], gamma.to(DEV), beta.to(DEV), groups, eps, act)
    assert torch.equal(dx1[0], dx[n]) and torch.equal(dg1[0], dg[n]) and torch.equal(db1[0], db[n])


# ------------------------------------------------------------------------------------------------ channel LayerNorm
@pytest.mark.parametrize("Cc,N,H,W", [(1, 3, 10, 10), (3, 2, 15, 9), (96, 3, 10, 10), (128, 2, 13, 11), (129, 3, 10, 10),
                                      (1024, 2, 7, 5)])
def test_layernorm_c_forward_and_backward(Cc, N, H, W):
    """Per pixel over C in fp32 chains (mean, variance, the two backward sums: length C), then per workgroup a 64-lane shuffle
    tree, 4 waves, and sum_rows over the workgroups.  N * HW is not a multiple of 256 and workgroup 0 straddles images.
    Bounds: 2 (C + 8) * 2^-24 * magnitudes for y / dx; dgamma / dbeta: the same per term + (10 + blocks) * 2^-24 * sum|terms|."""
    from dc_vic_amd import ops
    eps = 1e-5
    x, dy = rnd(N, Cc, H, W, seed=Cc, scale=1.5) + 0.25, rnd(N, Cc, H, W, seed=Cc + 1)
    gamma, beta = rnd(Cc, seed=2) + 1, rnd(Cc, seed=3)
    X, DY, Ga, Be = x.double(), dy.double(), gamma.double(), beta.double()
    mean = X.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(X.var(1, unbiased=False, keepdim=True) + eps)
    xh = (X - mean) * rstd
    e_xh = xh.abs() + (X.abs() + X.abs().mean(1, keepdim=True)) * rstd        # xh's error scale (chains over |x|)
    kC = 2 * (Cc + 8) * U
    G4 = Ga[None, :, None, None]
    y = ops.layernorm_c(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps)
    within("layernorm_c", y, xh * G4 + Be[None, :, None, None], kC * (e_xh * G4.abs() + Be.abs()[None, :, None, None]), "forward")
    Xr = X.clone().requires_grad_(True)
    yr = ((Xr - Xr.mean(1, keepdim=True)) / torch.sqrt(Xr.var(1, unbiased=False, keepdim=True) + eps)) * G4
    yr.backward(DY)
    dx, part = K().layernorm_c_bwd(x.to(DEV), dy.to(DEV), gamma.to(DEV), eps)
    d = (DY * G4).abs()
    per = d + d.mean(1, keepdim=True) + e_xh * (d * e_xh).mean(1, keepdim=True)
    within("layernorm_c_bwd dx", dx, Xr.grad, kC * rstd * per, "dx")
    tot = torch.empty(2 * Cc, device=DEV)
    K().sum_rows(part, tot, False)
    blocks = part.shape[0]
    for j, (ref, t1, t2) in enumerate((((DY * xh).sum((0, 2, 3)), (DY.abs() * e_xh).sum((0, 2, 3)), (DY * xh).abs().sum((0, 2, 3))),
                                       (DY.sum((0, 2, 3)), 0, DY.abs().sum((0, 2, 3))))):
        within("layernorm_c_bwd dgamma/dbeta", tot[j * Cc:(j + 1) * Cc], ref, kC * t1 + (10 + blocks) * U * t2, "dgamma" if j == 0 else "dbeta")
    dx2, part2 = K().layernorm_c_bwd(x.to(DEV), dy.to(DEV), gamma.to(DEV), eps)
    assert torch.equal(dx2, dx) and torch.equal(part2, part)


# ------------------------------------------------------------------------------------------------ column softmax backward
@pytest.mark.parametrize("N,Cc,Pn", [(1, 1, 1), (3, 4, 255), (1, 200, 256), (3, 200, 257), (1, 4, 4096), (3, 1, 257)])
def test_softmax_c_bwd(N, Cc, Pn):
    """dS = scale P (dP - sum_c P dP): the dot is an fp32 chain over C, then three roundings.
    Bound: 2^-24 |scale P| ((C + 2) sum_c |P dP| + 3 |dP - dot|)."""
    scale = 0.125
    P = torch.softmax(rnd(N, Cc, Pn, seed=Cc, scale=3.0), dim=1)
    dP = rnd(N, Cc, Pn, seed=Pn)
    Pd, dPd = P.double(), dP.double()
    dot = (Pd * dPd).sum(1, keepdim=True)
    ref = scale * Pd * (dPd - dot)
    bound = U * (scale * Pd).abs() * ((Cc + 2) * (Pd * dPd).abs().sum(1, keepdim=True) + 3 * (dPd - dot).abs())
    out = K().softmax_c_bwd(P.to(DEV), dP.to(DEV), scale)
    within("softmax_c_bwd", out, ref, bound, f"N={N} C={Cc} Pn={Pn}")


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("n", [1, 255, 257, 262144, 262145, 1572864])
def test_reduce_loss(n):
    """Four kinds, fp64 partials per workgroup (grid-stride above 1024 x 256 elements), fp64 final sum, one rounding: bound
    2 * 2^-24 |ref| + n * 2^-52 sum|terms|; BCE's per-element term is computed in fp32 (log1pf / expf): + 4 * 2^-24 * sum|term|."""
    a, b = rnd(n, seed=n), rnd(n, seed=n + 1)
    A, B = a.double(), b.double()
    ad, bd = a.to(DEV), b.to(DEV)
    sc = 1.0 / n
    for kind, terms in ((0, (A - B) ** 2), (2, A * A), (3, A)):
        out = K().reduce_loss(kind, ad, bd if kind == 0 else None, sc)
        ref = sc * terms.sum()
        within("reduce_loss", out.reshape(()), ref, 2 * U * ref.abs() + n * 2.0 ** -52 * sc * terms.abs().sum(), f"kind {kind}")
    # BCE-with-logits with |x| up to 80, both targets
    x = (urnd(n, seed=n + 2, lo=-80, hi=80) if n > 16 else torch.tensor([-80.0] * n))
    X = x.double()
    for t in (0, 1):
        out = K().reduce_loss(1, x.to(DEV), None, sc, target=t)
        terms = torch.clamp(X, min=0) - X * t + torch.log1p(torch.exp(-X.abs()))
        ref = sc * terms.sum()
        within("reduce_loss", out.reshape(()), ref, 2 * U * ref.abs() + 4 * U * sc * (X.abs() + 1).sum(), f"BCE t={t}")
    again = K().reduce_loss(0, ad, bd, sc)
    assert torch.equal(again, K().reduce_loss(0, ad, bd, sc))


@pytest.mark.parametrize("Cc,HW", [(2, 300), (256, 257), (1024, 100)])
def test_cross_entropy(Cc, HW):
    """Per pixel: max, an fp32 chain of C exponentials, logf; nll bound (C + 8) * 2^-24 * (|logsumexp| + |max| + |x_t| + 1);
    dlogits = w (softmax - onehot) with a relative softmax error of (C + 8) * 2^-24 (1 + |x - max|)."""
    N = 2
    x = rnd(N, Cc, 1, HW, seed=Cc, scale=20.0).clamp(-80, 80)
    x[0, :, 0, 0] = 80.0; x[0, 0, 0, 1] = -80.0; x[1, 1, 0, 2] = 80.0             # saturated logits, and channel 0 the only
    x[1, :, 0, 3] = -80.0; x[1, 0, 0, 3] = 80.0                                     # maximum 160 above the rest
    t = torch.randint(0, Cc, (N, 1, HW), generator=torch.Generator().manual_seed(1))
    w = 1.0 / (N * HW)
    X = x.double()
    lse = torch.logsumexp(X, 1)
    xt = X.gather(1, t[:, None]).squeeze(1)
    nll_ref = lse - xt
    mx = X.amax(1)
    k = (Cc + 8) * U
    for want in (False, True):
        nll, dl = K().cross_entropy(x.to(DEV), t.to(DEV), w, want_grad=want)
        within("cross_entropy", nll, nll_ref, k * (lse.abs() + mx.abs() + xt.abs() + 1), f"nll want_grad={want}")
        assert (dl is not None) == want
    sm = torch.softmax(X, 1)
    ref = w * (sm - F.one_hot(t, Cc).permute(0, 3, 1, 2).double())
    within("cross_entropy", dl, ref, k * w * sm * (1 + (X - mx[:, None]).abs()) + 2 * U * ref.abs(), "dlogits")


# ------------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("steps,clip", [(1, None), (2, 0.05), (1000, 1e9)])
def test_adam_and_clip_against_torch(steps, clip):
    """The kernel's Adam against torch.optim.Adam in fp64 (clip_grad_norm_ giving the gradient scale when `clip`), 1000 + 77
    elements, one of them with a zero gradient throughout.  Each step costs a few fp32 roundings of m, v and the update relative
    to their own magnitudes; the bound grows with the step count: 16 (steps + 1) * 2^-24 * (|p| + lr * steps)."""
    n = 1077
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p0 = rnd(n, seed=1)
    grads = [rnd(n, seed=100 + s % 37, scale=0.1 + (s % 5)) for s in range(steps)]
    for gr in grads:
        gr[17] = 0.0
    pd, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pr = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=lr, betas=(b1, b2), eps=eps)
    for s, gr in enumerate(grads, 1):
        gd = gr.to(DEV)
        gscale = None
        if clip is not None:
            sumsq = K().reduce_loss(2, gd, None, 1.0)
            gscale = K().clip_scale(sumsq, clip)
        K().adam_step(pd, gd, m, v, lr, b1, b2, eps, s, gscale)
        pr.grad = gr.double().clone()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([pr], clip)
        opt.step()
    # p is rounded once per step (relative to |p_t| <= |p| + lr t); the update carries a few roundings, and the fp32 bias
    # corrections 1 - b^t lose 2^-24 / (1 - b^t) of their value (500x at step 1 for b2 = 0.999)
    upd = sum(16 + 1 / (1 - b1 ** t) + 1 / (1 - b2 ** t) for t in range(1, steps + 1))
    bound = U * (4 * (steps + 1) * (pr.detach().abs() + lr * steps) + lr * upd)
    within("adam_step", pd, pr.detach(), bound, f"steps={steps} clip={clip}")
    assert torch.equal(pd.cpu()[17:18], p0[17:18]), "a zero gradient moved its parameter"


def test_clip_scale_edges():
    """min(1, max_norm / (sqrt(sumsq) + 1e-6)) in fp32: below, at and above the threshold, and a zero sum (scale 1)."""
    for ss, mx in ((0.25, 1.0), (1.0, 1.0), (4.0, 1.0), (0.0, 1.0), (1e6, 0.5)):
        out = K().clip_scale(torch.tensor([ss], device=DEV), mx)
        ref = min(1.0, mx / (math.sqrt(ss) + 1e-6))
        within("clip_scale", out, torch.tensor([ref]), torch.tensor([4 * U * ref]), f"sumsq={ss}")
        if ss == 0.0 or ss == 0.25:
            assert out.item() == 1.0


# ------------------------------------------------------------------------------------------------ resampling and LPIPS pieces
def test_resample2_exact():
    """Nearest x2 up is a copy; its adjoint sums each 2x2 block as (a + b) + (c + d): equal to that restatement in fp32."""
    x = rnd(3, 5, 7, 9, seed=1)                          # 15 planes, 63 low-res pixels each
    up = K().resample2(x.to(DEV), down=False)
    assert torch.equal(up.cpu(), x.repeat_interleave(2, 2).repeat_interleave(2, 3))
    y = rnd(3, 5, 14, 18, seed=2)
    dn = K().resample2(y.to(DEV), down=True)
    ref = (y[:, :, 0::2, 0::2] + y[:, :, 0::2, 1::2]) + (y[:, :, 1::2, 0::2] + y[:, :, 1::2, 1::2])
    assert torch.equal(dn.cpu(), ref)


def _s2d_ref(x, r, pad, Ho, Wo):
    P, H, W = x.shape
    xp = torch.zeros(P, max(H, Ho * r) + 2 * pad + r, max(W, Wo * r) + 2 * pad + r)
    xp[:, pad:pad + H, pad:pad + W] = x
    xp = xp[:, :Ho * r, :Wo * r]
    return xp.reshape(P, Ho, r, Wo, r).permute(0, 2, 4, 1, 3).reshape(P, r * r, Ho, Wo)


@pytest.mark.parametrize("r,pad,H,W,k", [(1, 0, 5, 7, 1), (2, 0, 9, 7, 2), (2, 2, 6, 11, 3), (4, 2, 64, 96, 11), (4, 0, 13, 15, 4),
                                         (4, 2, 37, 23, 11)])
def test_s2d_exact(r, pad, H, W, k):
    """Space-to-depth with zero padding and its adjoint (depth-to-space + crop) are permutations: exact.  Ho / Wo by the LPIPS
    stem's formula (blocks a k-tap / stride-r / pad conv reads)."""
    from dc_vic_amd._lib import check
    from dc_vic_amd.ops import _p
    P = 7                                                # odd plane count
    Ho, Wo = (H + 2 * pad - k) // r + 1 + (k - 1) // r, (W + 2 * pad - k) // r + 1 + (k - 1) // r
    x = rnd(P, H, W, seed=H)
    y = torch.empty(P, r * r, Ho, Wo, device=DEV)
    xd = x.to(DEV)
    check(L().dcvic_s2d_f32(_p(xd), _p(y), C.c_longlong(P), H, W, r, pad, Ho, Wo, 0, None), "s2d")
    assert torch.equal(y.cpu(), _s2d_ref(x, r, pad, Ho, Wo))
    g = rnd(P, r * r, Ho, Wo, seed=W)
    dx = torch.empty(P, H, W, device=DEV)
    gd = g.to(DEV)
    check(L().dcvic_s2d_f32(_p(gd), _p(dx), C.c_longlong(P), H, W, r, pad, Ho, Wo, 1, None), "s2d inverse")
    idx = _s2d_ref(torch.arange(P * H * W, dtype=torch.float64).reshape(P, H, W) + 1, r, pad, Ho, Wo).long() - 1
    ref = torch.zeros(P * H * W, dtype=torch.float32)
    m = idx >= 0
    ref[idx[m]] = g[m]                                  # every image pixel is read by exactly one depth slot (or none)
    assert torch.equal(dx.cpu(), ref.reshape(P, H, W))


@pytest.mark.parametrize("H,W", [(3, 3), (4, 7), (7, 4), (55, 55)])
def test_maxpool3s2_exact(H, W):
    """MaxPool2d(3, 2) forward, argmax (first maximum in the window wins, as in torch) and the gather backward vs fp64
    autograd, on inputs rounded to a few values so that windows hold exact ties."""
    from dc_vic_amd._lib import check
    from dc_vic_amd.ops import _p
    P = 5
    x = torch.round(rnd(P, H, W, seed=H * W) * 2) / 2
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    y = torch.empty(P, Ho, Wo, device=DEV)
    am = torch.empty(P, Ho, Wo, dtype=torch.uint8, device=DEV)
    xd = x.to(DEV)
    check(L().dcvic_maxpool3s2_f32(_p(xd), _p(y), _p(am), None, None, C.c_longlong(P), H, W, None), "maxpool")
    ry, ri = F.max_pool2d(x[:, None], 3, 2, return_indices=True)
    assert torch.equal(y.cpu(), ry[:, 0])
    oy, ox = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    ridx = ri[:, 0]
    k_ref = (ridx // W - 2 * oy) * 3 + (ridx % W - 2 * ox)
    assert torch.equal(am.cpu().long(), k_ref), "argmax is not the first maximum"
    dy = rnd(P, Ho, Wo, seed=3)
    dx = torch.empty(P, H, W, device=DEV)
    dyd = dy.to(DEV)
    check(L().dcvic_maxpool3s2_f32(None, None, _p(am), _p(dyd), _p(dx), C.c_longlong(P), H, W, None), "maxpool bwd")
    xr = x.double()[:, None].clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2).backward(dy.double()[:, None])
    # at most 4 windows share an input: sums of <= 4 terms in a fixed order
    xa = x.double()[:, None].clone().requires_grad_(True)
    F.max_pool2d(xa, 3, 2).backward(dy.double().abs()[:, None])                # sum |terms| per input pixel
    within("maxpool3s2 bwd", dx, xr.grad[:, 0], 3 * U * xa.grad[:, 0], f"{H}x{W}")


@pytest.mark.parametrize("Cc,H,W", [(64, 15, 15), (192, 7, 7), (256, 13, 21)])
def test_lpips_tap(Cc, H, W):
    """One tap: unit-normalise over C, weighted squared difference (value per pixel) and the gradient w.r.t. f1 vs fp64 autograd
    of the same formula; fp32 chains over C: bound 2 (C + 8) * 2^-24 * magnitudes.  Some pixels of f1 are all zero (the r1 > 0
    guard: the gradient there is g / n1 * dval/du1, as autograd of f / (||f|| + 1e-10) gives)."""
    from dc_vic_amd._lib import check
    from dc_vic_amd.ops import _p
    N, HW = 2, H * W
    f0, f1 = rnd(N, Cc, HW, seed=Cc).relu(), rnd(N, Cc, HW, seed=Cc + 1).relu()
    f1[0, :, 3] = 0.0; f1[1, :, HW - 1] = 0.0
    f0[1, :, 5] = 0.0
    w = rnd(Cc, seed=5).abs() / Cc
    gscale = 0.7
    pix = torch.empty(N, HW, device=DEV)
    df1 = torch.empty(N, Cc, HW, device=DEV)
    f0d, f1d, wd = f0.to(DEV), f1.to(DEV), w.to(DEV)          # (held: the launch must not see freed temporaries)
    check(L().dcvic_lpips_tap_f32(_p(f0d), _p(f1d), _p(wd), _p(pix), _p(df1), N, Cc, HW, C.c_float(gscale), None),
          "lpips_tap")
    A, Bm, Wd = f0.double(), f1.double().clone().requires_grad_(True), w.double()[None, :, None]
    u0 = A / (A.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = Bm.pow(2).sum(1, keepdim=True).clamp_min(1e-300).sqrt() + 1e-10      # (clamped: the norm's gradient at f1 = 0 is 0)
    u1 = Bm / n1
    val = (Wd * (u0 - u1) ** 2).sum(1)
    (val.sum() * gscale / HW).backward()
    k = 2 * (Cc + 8) * U
    dmag = (Wd * (u0.abs() + u1.abs()) ** 2).sum(1)
    within("lpips_tap", pix, val.detach(), k * dmag, "value")
    gmag = gscale / HW * Wd * (u0.abs() + u1.abs()) / n1.detach() * 2
    gmag = gmag + gscale / HW * u1.detach().abs() / n1.detach() * (2 * Wd * (u0.abs() + u1.detach().abs()) * u1.detach().abs()).sum(1, keepdim=True)
    within("lpips_tap", df1, Bm.grad, k * gmag, "df1")


# ------------------------------------------------------------------------------------------------ Swin window attention
def swin_ref(qkv, dout, table, heads, ws, shift):
    """fp64 autograd of the forward (swin.hip): shifted windows, scaled q k^T + relative bias (+ -100 mask), softmax, @ v;
    returns dqkv, dtable, and the score gradient / probabilities per (n, window, head) for the bounds."""
    N, C3, H, W = qkv.shape
    Cc, hd, T = C3 // 3, C3 // 3 // heads, ws * ws
    Q = qkv.double().clone().requires_grad_(True)
    Tb = table.double().clone().requires_grad_(True)
    xs = torch.roll(Q, (-shift, -shift), (2, 3))
    nWy, nWx = H // ws, W // ws
    win = xs.reshape(N, 3, heads, hd, nWy, ws, nWx, ws).permute(1, 0, 4, 6, 2, 5, 7, 3).reshape(3, N * nWy * nWx, heads, T, hd)
    q, k, v = win[0], win[1], win[2]
    ty, tx = torch.arange(T) // ws, torch.arange(T) % ws
    rel = (ty[:, None] - ty[None, :] + ws - 1) * (2 * ws - 1) + (tx[:, None] - tx[None, :] + ws - 1)
    S = (q * hd ** -0.5) @ k.transpose(-1, -2) + Tb[rel].permute(2, 0, 1)[None]
    if shift > 0:
        lab = torch.zeros(H, W, dtype=torch.long)
        for i, ys in enumerate((slice(0, H - ws), slice(H - ws, H - shift), slice(H - shift, H))):
            for j, xsl in enumerate((slice(0, W - ws), slice(W - ws, W - shift), slice(W - shift, W))):
                lab[ys, xsl] = i * 3 + j
        lw = lab.reshape(nWy, ws, nWx, ws).permute(0, 2, 1, 3).reshape(nWy * nWx, T)
        mask = (lw[:, :, None] != lw[:, None, :]).double() * -100.0
        S = S + mask.repeat(N, 1, 1)[:, None]
    S.retain_grad()
    Pm = torch.softmax(S, -1)
    o = Pm @ v
    out = o.reshape(N, nWy, nWx, heads, ws, ws, hd).permute(0, 3, 6, 1, 4, 2, 5).reshape(N, Cc, H, W)
    out = torch.roll(out, (shift, shift), (2, 3))
    (out * dout.double()).sum().backward()
    return Q.grad, Tb.grad, S.grad.detach(), Pm.detach(), rel, (q.detach(), k.detach(), v.detach())


@pytest.mark.parametrize("N,Cc,heads,H,W,shift", [(1, 96, 6, 16, 24, 0), (3, 96, 6, 24, 16, 4), (1, 32, 4, 16, 16, 4)])
def test_swin_attn_bwd(N, Cc, heads, H, W, shift):
    """Per (n, window, head): fp32 fma chains over the head dim (scores, dP), over the 64 tokens (softmax sum, the dP dot, dq /
    dk / dv), and the table gradient as a 64-lane chain over windows and pairs plus a shuffle tree.  k = 2 (64 + hd + 16), times
    the magnitude of each result's terms (with the score error, up to |S| + 100 for masked pairs, carried through P).
    Head dims 16 (the model's) and 8; shift 4 with the -100 mask; dtable with accumulate False and True onto a non-zero start."""
    ws = 8
    hd = Cc // heads
    qkv, dout = rnd(N, 3 * Cc, H, W, seed=1, scale=1.5), rnd(N, Cc, H, W, seed=2)
    R = (2 * ws - 1) ** 2
    table = rnd(R, heads, seed=3, scale=0.5)
    t0 = rnd(R, heads, seed=4)
    dq_ref, dt_ref, dS, Pm, rel, (q, k, v) = swin_ref(qkv, dout, table, heads, ws, shift)
    kk = 2 * (64 + hd + 16) * U
    # magnitudes: |S| error scale E (hd-chain of |q k| scale + |bias| + mask); P's relative error ~ kk (1 + E + E_max)
    E = ((q.abs() * hd ** -0.5) @ k.abs().transpose(-1, -2)) + table.double().abs()[rel].permute(2, 0, 1)[None] + (100.0 if shift else 0)
    relP = 1 + E + E.amax(-1, keepdim=True)
    dOw = torch.roll(dout.double(), (-shift, -shift), (2, 3)).reshape(N, heads, hd, H // ws, ws, W // ws, ws) \
        .permute(0, 3, 5, 1, 4, 6, 2).reshape(-1, heads, 64, hd)
    MdP = dOw.abs() @ v.abs().transpose(-1, -2)
    dot = (Pm * MdP).sum(-1, keepdim=True)
    MdS = Pm * (MdP + dot + relP * (MdP + dot))
    for acc in (False, True):
        dtable = (t0 if acc else torch.full_like(t0, float("nan"))).to(DEV)
        dq = K().swin_attn_bwd(qkv.to(DEV), dout.to(DEV), table.to(DEV), dtable, heads, ws, shift, accumulate=acc)
        # table: sum |dS| per (rel, head) over all windows and pairs
        mag = torch.zeros(R, heads, dtype=torch.float64)
        mag.index_add_(0, rel.flatten(), MdS.permute(2, 3, 0, 1).reshape(64 * 64, -1, heads).sum(1))
        base = t0.double() if acc else 0.0
        nwin = dS.shape[0]
        chain = 64 * -(-nwin // 64) + 8                # per lane: its windows' 64 pairs each, then the shuffle tree
        within("swin_attn_bwd dtable", dtable, dt_ref + base, kk * mag + chain * U * (mag + (t0.double().abs() if acc else 0)),
               f"acc={acc}")
    # dq / dk / dv: map the window-layout magnitudes back to the [N, 3C, H, W] layout the same way the reference did
    sc = hd ** -0.5
    Mq = sc * MdS @ k.abs()
    Mk = sc * MdS.transpose(-1, -2) @ q.abs()
    Mv = (Pm * relP).transpose(-1, -2) @ dOw.abs()
    M = torch.stack([Mq, Mk, Mv])                                    # [3, nw_total, heads, T, hd]
    nWy, nWx = H // ws, W // ws
    Mm = M.reshape(3, N, nWy, nWx, heads, ws, ws, hd).permute(1, 0, 4, 7, 2, 5, 3, 6).reshape(N, 3 * Cc, H, W)
    Mm = torch.roll(Mm, (shift, shift), (2, 3))
    within("swin_attn_bwd dqkv", dq, dq_ref, kk * Mm, f"shift={shift}")
