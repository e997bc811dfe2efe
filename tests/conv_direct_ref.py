"""The direct convolution family (csrc/conv.hip, conv3x3.hip, conv1x1.hip, conv_async.hip, conv_async16.hip, thin.hip) restated on the
CPU, and the cases tests/test_gpu_conv_direct.py and tests/test_conv_direct_host.py share.

  conv_chain32 / layer_chain32   the kernel's own fp32 chain: acc = fp32(fp64(acc) + fp64(x) fp64(w)) per step (the product of two fp32
                                 values is exact in fp64, so a step is an fma but for a second rounding), in the order dcvic_conv2d_f32
                                 derives: 8-channel chunks ascending, inside a chunk (tap, channel), or (4-channel half, tap, channel)
                                 under the `halves` predicate; geometry from the descriptor builders restated below, never F.conv2d
  epilogue32                     bias -> activation -> + res -> v (1 + s) + t in fp32, in the kernel's order
  conv_ref64 / terms64           the same layer in fp64 through torch's own operators; sum |x| |w| over the same taps + |init|
  select_class / variant_of / launch_plan   the host-side variant choice and the dispatch order of dcvic_conv2d_f32 at a given CU count
  CASES / DGRAD_CASES            the case tables, what each case reaches (reached, REQUIRED) and its reference (case_reference)

A plain module: no fixtures, nothing that needs a GPU at import."""
import torch
import torch.nn.functional as F

from infer_kernels_ref import (ACT_GELU, ACT_HALF_TANH, ACT_LRELU02, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, FLOOR, MARGIN,  # noqa: F401
                               act as act_fn)
from kernel_bounds import U, regime

KC = 8
ALL_ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_SWISH, ACT_GELU, ACT_SIGMOID, ACT_HALF_TANH)
ORDER_K = 2                       # comparison (a): 2 U sum|terms|
ADJOINT_K = 32                    # the adjoint identity: 32 U sum|terms|
K_MAX = 64                        # the restatement's own k against fp64 stays below this on every case (host test)


# ------------------------------------------------------------------------------------------------ descriptors (conv.hip)
def desc_conv(KH, KW, stride=1, pad_t=0, pad_l=0, upsample=False):
    """dcvic_conv_desc_init: tap t = ky KW + kx reads input offset (ky - pad_t, kx - pad_l)."""
    taps = [(ky, kx, ky - pad_t, kx - pad_l) for ky in range(KH) for kx in range(KW)]
    return dict(taps=taps, stride=stride, upsample=bool(upsample), transposed=False)


def desc_convT(k, py=0, px=0):
    """dcvic_convT_phase_desc.  k3 (s1, p1): oy = iy - 1 + ky, so dy = 1 - ky.  k5 (s2, p2, op1): oy = 2 iy - 2 + ky; for oy = 2 m + py the
    taps are ky = py (mod 2) and iy = m + (py + 2 - ky) / 2."""
    if k == 3:
        assert (py, px) == (0, 0)
        taps = [(ky, kx, 1 - ky, 1 - kx) for ky in range(3) for kx in range(3)]
    elif k == 5:
        taps = [(ky, kx, (py + 2 - ky) // 2, (px + 2 - kx) // 2) for ky in range(py, 5, 2) for kx in range(px, 5, 2)]
    else:
        raise ValueError(k)
    return dict(taps=taps, stride=1, upsample=False, transposed=True)


def tap_grid(d):
    """(TX, dy0, dx0, dstep) as dcvic_conv2d_f32 derives them; asserts its `regular grid` checks."""
    taps = d["taps"]
    T = len(taps)
    TX = 1
    while TX < T and taps[TX][2] == taps[0][2]:
        TX += 1
    assert T % TX == 0
    step = ((taps[1][3] - taps[0][3]) if TX > 1 else (taps[1][2] - taps[0][2])) if T > 1 else 1
    assert step in (1, -1)
    for t, (_, _, dy, dx) in enumerate(taps):
        assert dy == taps[0][2] + (t // TX) * step and dx == taps[0][3] + (t % TX) * step
    return TX, taps[0][2], taps[0][3], step


def halves_of(d, src_channels):
    """ConvKArgs::halves: 2 for the Conv2d(k3, s1, p1) family whose sources are all multiples of 8 channels, else 1."""
    TX, dy0, dx0, dstep = tap_grid(d)
    fam = len(d["taps"]) == 9 and TX == 3 and dstep == 1 and dy0 == -1 and dx0 == -1 and d["stride"] == 1 and not d["upsample"] \
        and sum(src_channels) % KC == 0 and all(c % KC == 0 for c in src_channels)
    return 2 if fam else 1


def chain_order(Cin, T, halves):
    """The (tap, channel) pairs of one output element's chain, in order."""
    for c0 in range(0, Cin, KC):
        if halves == 2:
            for h in (0, 4):
                for t in range(T):
                    for c in range(c0 + h, c0 + h + 4):
                        yield t, c
        else:
            for t in range(T):
                for c in range(c0, min(c0 + KC, Cin)):
                    yield t, c


# ------------------------------------------------------------------------------------------------ layers -> phases (ops.ConvPlan)
def layer(kind, k=3, stride=1, pad=0, out_hw=None, ups_phases=True):
    """kind: "conv" Conv2d(k, stride, pad) (out_hw: the ldm Downsample, F.pad (0, 1, 0, 1) then pad 0), "ups" nearest x2 + Conv2d(k3, s1, p1)
    (as four 2x2 phases, or through the UPS kernel template when ups_phases is False), "phases2" ConvPlan.from_phases2 (weights
    [4, Cout, Cin, 2, 2]), "convT" ConvTranspose2d(k5, s2, p2, op1) / (k3, s1, p1)."""
    return dict(kind=kind, k=k, stride=stride, pad=pad, out_hw=out_hw, ups_phases=ups_phases)


def out_size(L, H, W):
    if L["kind"] == "conv":
        if L["out_hw"] is not None:
            return tuple(L["out_hw"])
        return (H + 2 * L["pad"] - L["k"]) // L["stride"] + 1, (W + 2 * L["pad"] - L["k"]) // L["stride"] + 1
    if L["kind"] == "convT" and L["k"] == 3:
        return H, W
    return 2 * H, 2 * W


def ups_phase_weights(w):
    """ConvPlan.__init__: nearest x2 + conv3x3 as four 2x2 convolutions; the taps that land on the same low-resolution row / column are
    pre-added in fp32, in the plan's order."""
    weffs = []
    for py in (0, 1):
        rows = [w[:, :, 0], w[:, :, 1] + w[:, :, 2]] if py == 0 else [w[:, :, 0] + w[:, :, 1], w[:, :, 2]]
        for px in (0, 1):
            cols = [torch.stack([r[:, :, 0], r[:, :, 1] + r[:, :, 2]] if px == 0 else [r[:, :, 0] + r[:, :, 1], r[:, :, 2]], dim=-1) for r in rows]
            weffs.append(torch.stack(cols, dim=2))
    return weffs


def phases_of(L, w, H, W):
    """The launches of one ConvPlan call: [dict(desc, w, Hout, Wout, osy, osx, ooy, oox)] and the full output size."""
    Hf, Wf = out_size(L, H, W)
    one = dict(Hout=Hf, Wout=Wf, osy=1, osx=1, ooy=0, oox=0)
    kind, k = L["kind"], L["k"]
    if kind == "conv":
        pad = 0 if L["out_hw"] is not None else L["pad"]
        return [dict(one, desc=desc_conv(k, k, L["stride"], pad, pad), w=w)], (Hf, Wf)
    if kind == "ups" and not L["ups_phases"]:
        return [dict(one, desc=desc_conv(3, 3, 1, 1, 1, upsample=True), w=w)], (Hf, Wf)
    if kind == "convT" and k == 3:
        return [dict(one, desc=desc_convT(3), w=w)], (Hf, Wf)
    out = []
    if w is None:                 # the geometry alone
        wph = [None] * 4
    else:
        wph = ups_phase_weights(w) if kind == "ups" else (list(w) if kind == "phases2" else [w] * 4)
    for i, (py, px) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        d = desc_convT(5, py, px) if kind == "convT" else desc_conv(2, 2, 1, 1 - py, 1 - px)
        out.append(dict(desc=d, w=wph[i], Hout=H, Wout=W, osy=2, osx=2, ooy=py, oox=px))
    return out, (Hf, Wf)


# ------------------------------------------------------------------------------------------------ the chain
def pm(t):
    """[N, C, H, W] -> pixel-major [N H W, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_chain32(srcs, w, g, init=None, idx=None):
    """One launch's accumulators, pixel-major [pixels, Cout] fp32: for the pixels `idx` (flat indices into N x Hout x Wout; None: all).
    g: a phase of phases_of.  init: [N, Cout, Hout, Wout] or None."""
    d = g["desc"]
    x = torch.cat(list(srcs), 1)
    N, Cin, H, W = x.shape
    Hout, Wout = g["Hout"], g["Wout"]
    tap_grid(d)
    if idx is None:
        idx = torch.arange(N * Hout * Wout)
    n, oy, ox = idx // (Hout * Wout), (idx // Wout) % Hout, idx % Wout
    xp = x.permute(0, 2, 3, 1)
    cols, wts = [], []
    for ky, kx, dy, dx in d["taps"]:
        if d["upsample"]:
            iy, ix = (oy + dy) >> 1, (ox + dx) >> 1
        else:
            iy, ix = oy * d["stride"] + dy, ox * d["stride"] + dx
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        v = xp[n, iy.clamp(0, H - 1), ix.clamp(0, W - 1)]
        cols.append(torch.where(ok[:, None], v, torch.zeros(())).t().double().contiguous())          # [Cin, pixels]
        wk = w[:, :, ky, kx]
        wts.append((wk if d["transposed"] else wk.t()).double().contiguous())                         # [Cin, Cout]
    Cout = wts[0].shape[1]
    acc = torch.zeros(idx.numel(), Cout) if init is None else pm(init)[idx].clone()
    for t, c in chain_order(Cin, len(d["taps"]), halves_of(d, [s.shape[1] for s in srcs])):
        acc = torch.addcmul(acc.double(), cols[t][c][:, None], wts[t][c][None, :]).float()
    return acc


def _phase_pixels(g, idx, Hf, Wf):
    """Which of the full-output pixels idx (flat into N x Hf x Wf) a phase writes, and their flat indices in the phase's own grid."""
    n, oy, ox = idx // (Hf * Wf), (idx // Wf) % Hf, idx % Wf
    sel = ((oy % g["osy"]) == g["ooy"]) & ((ox % g["osx"]) == g["oox"])
    py, px = (oy - g["ooy"]) // g["osy"], (ox - g["oox"]) // g["osx"]
    sel &= (py < g["Hout"]) & (px < g["Wout"])
    return sel, ((n * g["Hout"] + py) * g["Wout"] + px)[sel]


def layer_chain32(L, srcs, w, init=None, idx=None):
    """conv_chain32 over every phase of the layer, scattered as the launches scatter: pixel-major [len(idx), Cout] for the full-output
    pixels idx (None: all)."""
    H, W = srcs[0].shape[2:]
    N = srcs[0].shape[0]
    phases, (Hf, Wf) = phases_of(L, w, H, W)
    if idx is None:
        idx = torch.arange(N * Hf * Wf)
    out = None
    for g in phases:
        sel, pidx = _phase_pixels(g, idx, Hf, Wf)
        ini = None
        if init is not None:
            ini = init[:, :, g["ooy"]::g["osy"], g["oox"]::g["osx"]][:, :, :g["Hout"], :g["Wout"]]
        a = conv_chain32(srcs, g["w"], g, ini, pidx)
        if out is None:
            out = torch.full((idx.numel(), a.shape[1]), float("nan"))
        out[sel] = a
    return out


# ------------------------------------------------------------------------------------------------ epilogue
ACT_SLOPE = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_LRELU02: 1.0, ACT_SWISH: 1.1, ACT_GELU: 1.13, ACT_SIGMOID: 0.25, ACT_HALF_TANH: 0.5}
ACT_ROUNDINGS = 8                 # a transcendental activation's own roundings, see epilogue_terms


def epilogue32(acc, bias=None, act=ACT_NONE, res=None, affine=None):
    """dcvic_conv_epilogue in fp32 on pixel-major values: + bias (skipped without one: "+ 0" would turn -0 into +0), activation, + res,
    v (1 + s) + t.  res / affine are pixel-major too."""
    v = acc if bias is None else acc + bias[None, :]
    v = act_fn(act, v)
    if res is not None:
        v = v + res
    if affine is not None:
        v = v * (1.0 + affine[0]) + affine[1]
    return v


def epilogue64(v, bias=None, act=ACT_NONE, res=None, affine=None):
    v = v.double()
    if bias is not None:
        v = v + bias.double()[None, :]
    v = act_fn(act, v)
    if res is not None:
        v = v + res.double()
    if affine is not None:
        v = v * (1.0 + affine[0].double()) + affine[1].double()
    return v


def epilogue_terms(terms, v64, bias=None, act=ACT_NONE, res=None, affine=None):
    """sum|terms| carried through the epilogue.  An error e of the pre-activation value becomes at most slope x e (the activation's slope
    bound, as in test_groupnorm_forward).  A transcendental activation adds roundings of its own: expf / erff / tanhf of the device and
    of the host are each within about an ulp, then an add, a multiply or a divide -- ACT_ROUNDINGS = 8 U relative to |act(v)|, and for
    GELU relative to |v| (1 + erf cancels for negative v, so erff's absolute error counts, times |v| / 2).  The residual and the affine
    map add their own magnitudes.  v64: the fp64 pre-activation value with bias."""
    t = terms if bias is None else terms + bias.double().abs()[None, :]
    y = act_fn(act, v64)
    if act in (ACT_SWISH, ACT_SIGMOID, ACT_HALF_TANH):
        t = ACT_SLOPE[act] * t + ACT_ROUNDINGS / ORDER_K * y.abs()
    elif act == ACT_GELU:
        t = ACT_SLOPE[act] * t + ACT_ROUNDINGS / ORDER_K * v64.abs()
    if res is not None:
        t = t + res.double().abs()
    if affine is not None:
        t = t * (1.0 + affine[0].double()).abs() + affine[1].double().abs()
    return t


# ------------------------------------------------------------------------------------------------ fp64 through torch's operators
def conv_ref64(L, srcs, w, init=None):
    """The layer's linear part in fp64, [N, Cout, Hf, Wf]: F.conv2d / F.conv_transpose2d / F.interpolate / F.pad."""
    x = torch.cat([s.double() for s in srcs], 1)
    kind, k = L["kind"], L["k"]
    if kind == "conv":
        if L["out_hw"] is not None:
            y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w.double(), stride=L["stride"])
            assert tuple(y.shape[2:]) == tuple(L["out_hw"])
        else:
            y = F.conv2d(x, w.double(), stride=L["stride"], padding=L["pad"])
    elif kind == "ups":
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w.double(), padding=1)
    elif kind == "convT":
        y = F.conv_transpose2d(x, w.double(), stride=2, padding=2, output_padding=1) if k == 5 else F.conv_transpose2d(x, w.double(), padding=1)
    elif kind == "phases2":
        N, _, H, W = x.shape
        y = torch.zeros(N, w[0].shape[0], 2 * H, 2 * W, dtype=torch.float64)
        for wp, (py, px) in zip(w, ((0, 0), (0, 1), (1, 0), (1, 1))):
            y[:, :, py::2, px::2] = F.conv2d(F.pad(x, (1 - px, px, 1 - py, py)), wp.double())
    else:
        raise ValueError(kind)
    return y if init is None else y + init.double()


def terms64(L, srcs, w, init=None):
    """sum |x| |w| over the same taps, + |init|."""
    wa = [p.abs() for p in w] if L["kind"] == "phases2" else w.abs()
    return conv_ref64(L, [s.abs() for s in srcs], wa, None if init is None else init.abs())


# ------------------------------------------------------------------------------------------------ variant choice and dispatch (conv.hip)
CLASS_TC = (128, 64, 32, 96)
CLASS_P = ((256, 128, 64), (256, 128, 64), (256, 128, 64, 32), (256, 128))
TUNING_DEFAULT = (1, 1, 2)        # dcvic_conv_set_tuning(use_dma, use_async, async_fill); use_async 2: the 32x32x2 twin only
A_MAXSLOT, NTHREADS = 16, 256
ASYNC16_TILES = ((0, 64), (1, 128), (1, 64), (2, 256), (2, 128), (2, 64), (2, 32))
GENERIC_TILES = ((0, 256), (0, 128), (0, 64), (1, 256), (1, 128), (1, 64), (2, 256), (2, 128), (3, 256), (3, 128))


def tile_width_log(Wout):
    TWlog = 5
    while TWlog > 2 and (1 << TWlog) > Wout and (1 << (TWlog - 1)) >= Wout:
        TWlog -= 1
    return TWlog


def choose_class(Cout):
    if Cout <= 32:
        return 2
    if Cout <= 64:
        return 1
    if Cout in (96, 192):
        return 3
    if Cout % 128 == 0 or Cout > 192:
        return 0
    return 1


def variant_score(cls, P, Cout, N, Hout, Wout, ups, num_cu=256, use_async=1):
    if P <= 0:
        return -1.0
    if cls == 2 and P < 128 and (ups or use_async != 1):
        return -1.0
    TC = CLASS_TC[cls]
    TW = 1 << tile_width_log(Wout)
    TH = P // TW
    if TH < 1 or (ups and (TH & 1)):
        return -1.0
    cot = -(-Cout // TC)
    ty, tx = -(-Hout // TH), -(-Wout // TW)
    wg = float(N) * ty * tx * cot
    useful = Cout / (cot * TC) * (float(Hout) * Wout) / (float(ty) * TH * tx * TW)
    fill = 1.0 if wg >= 1.5 * num_cu else wg / (1.5 * num_cu)
    effP = {256: 1.0, 128: 0.93, 64: 0.85}.get(P, 0.75)
    effC = {128: 1.0, 96: 0.97, 64: 0.93}.get(TC, 0.80)
    return useful * fill * effP * effC


def select_class(Cout, N, Hout, Wout, ups, num_cu=256, use_async=1):
    """dcvic_conv_select_class: the TC class (it fixes the weight pack) with the best-scoring tile."""
    best_cls, best = choose_class(Cout), -1.0
    for cls in range(4):
        for P in CLASS_P[cls]:
            sc = variant_score(cls, P, Cout, N, Hout, Wout, ups, num_cu, use_async)
            if sc > best + 1e-9:
                best, best_cls = sc, cls
    return best_cls


def variant_of(cls, Cout, N, Hout, Wout, ups, num_cu=256, use_async=1):
    """The pixel-tile size P dcvic_conv2d_f32 picks inside class cls."""
    P, best = 0, -1.0
    for p in CLASS_P[cls]:
        sc = variant_score(cls, p, Cout, N, Hout, Wout, ups, num_cu, use_async)
        if sc > best:
            best, P = sc, p
    return P


def launch_plan(d, src_channels, Cout, N, H, W, Hout, Wout, num_cu=256, tuning=TUNING_DEFAULT, init=False, scatter=False, hw_vec=True):
    """dcvic_conv2d_f32's host side for one launch: dict(variant, cls, P, TWlog, TG, CPS, n_chunks, nslots, halves, blocks).
    variant as dcvic_conv_last_variant reports it.  hw_vec: every source is a 16-byte view (conv1x1.hip's test)."""
    use_dma, use_async, fill = tuning
    fill = fill if fill > 0 else TUNING_DEFAULT[2]
    ups = d["upsample"]
    taps = d["taps"]
    T = len(taps)
    Cin = sum(src_channels)
    TX, dy0, dx0, dstep = tap_grid(d)
    halves = halves_of(d, src_channels)
    cls = select_class(Cout, N, Hout, Wout, ups, num_cu, use_async)
    P = variant_of(cls, Cout, N, Hout, Wout, ups, num_cu, use_async)
    assert P > 0
    TC = CLASS_TC[cls]
    TWlog = tile_width_log(Wout)
    TW = 1 << TWlog
    TH = P // TW
    n_chunks, n_cot = -(-Cin // KC), -(-Cout // TC)
    blocks = N * (-(-Hout // TH)) * (-(-Wout // TW)) * n_cot
    dys, dxs = [t[2] for t in taps], [t[3] for t in taps]
    if ups:
        PH, PW = TH // 2 + ((max(dys) - min(dys) + 1) >> 1) + 1, TW // 2 + ((max(dxs) - min(dxs) + 1) >> 1) + 1
    else:
        PH, PW = (TH - 1) * d["stride"] + max(dys) - min(dys) + 1, (TW - 1) * d["stride"] + max(dxs) - min(dxs) + 1
    plane = PH * PW
    TG = max(1, min(T, (40 * 1024) // (KC * TC * 4)))
    CPS = 1
    if TG == T:
        per_chunk = (KC * plane + T * KC * TC) * 4
        mfma = T * (KC // 2) * ((TC // 32) * (P // 32)) // 4
        while CPS < 8 and (CPS + 1) * per_chunk <= 48 * 1024 and CPS * mfma < 256:
            CPS += 1
        CPS = min(CPS, n_chunks)
    r = dict(cls=cls, P=P, TWlog=TWlog, TG=TG, CPS=CPS, n_chunks=n_chunks, nslots=-(-plane // NTHREADS), halves=halves, blocks=blocks, T=T)

    def async_fits():
        tg = max(1, (40 * 1024) // (KC * TC * 4))
        if halves == 2 and tg < T:
            tg = T
        tg = min(tg, T)
        cps = 1
        if tg == T:
            per_chunk = (KC * plane + T * KC * TC) * 4
            while cps < 8 and (cps + 1) * per_chunk <= 48 * 1024 and (cps + 1) * KC * plane <= A_MAXSLOT * NTHREADS:
                cps += 1
            cps = min(cps, n_chunks)
        xslots = -(-(cps * KC * plane) // NTHREADS)
        if xslots > A_MAXSLOT:
            return False
        xs = xslots * NTHREADS + 2 * (PW + 2)
        ws = ((cps * T if tg >= T else tg) + 2) * KC * TC
        return 2 * (xs + ws) * 4 <= 156 * 1024

    if P == 256 and use_dma and not ups and cls in (0, 3) and TWlog == 5 and not init and d["stride"] == 1 and dstep == 1:
        fam3 = halves == 2
        ph2 = not fam3 and T == 4 and TX == 2 and Cin % KC == 0 and all(c % KC == 0 for c in src_channels)
        if (fam3 or ph2) and not (cls == 3 and not fam3):
            tiles = N * (-(-Hout // 8)) * (-(-Wout // 32)) * n_cot
            return dict(r, variant=9003 if cls == 3 else (9000 if fam3 else 9001), blocks=tiles)
    if cls == 2 and P < 128:
        assert async_fits()
        return dict(r, variant=8500 + cls * 100 + P // 32)
    if use_dma and T == 1 and d["stride"] == 1 and not ups and not init and dy0 == 0 and dx0 == 0 and not scatter \
            and (Hout, Wout) == (H, W) and (H * W) % 4 == 0 and hw_vec and cls in (0, 1, 3):
        b1 = N * (-(-(H * W) // 256)) * n_cot
        if b1 >= num_cu:
            return dict(r, variant=7000 + cls, blocks=b1)
    if not ups and use_async and blocks <= (1 if P == 256 else fill) * num_cu and async_fits():
        if use_async == 1 and (cls, P) in ASYNC16_TILES:
            return dict(r, variant=8500 + cls * 100 + P // 32)
        return dict(r, variant=8000 + cls * 100 + P // 32)
    assert (cls, P) in GENERIC_TILES
    return dict(r, variant=cls * 1000 + P + (1 if ups else 0))


# ------------------------------------------------------------------------------------------------ the cases
# tunings: dcvic_conv_set_tuning(use_dma, use_async, async_fill)
GENERIC, DMA, ASYNC32, ASYNC16 = (0, 0, -1), (1, 0, -1), (0, 2, 1 << 20), (0, 1, 1 << 20)
C1, C3, C5 = layer("conv", 1), layer("conv", 3, 1, 1), layer("conv", 5, 1, 2)
C1S2, C3S2, C5S2 = layer("conv", 1, 2, 0), layer("conv", 3, 2, 1), layer("conv", 5, 2, 2)
UPS, UPS_TEMPLATE, PH2 = layer("ups"), layer("ups", ups_phases=False), layer("phases2")
CT5, CT3 = layer("convT", 5), layer("convT", 3)
OFF_REGIMES = ("offset", "outlier", "swish")
ALL_REGIMES = ("normal",) + OFF_REGIMES + ("offset_zero_sum",)


def case(id, fam, L, cins, cout, N, H, W, expect, tuning=GENERIC, act=ACT_NONE, bias=True, res=False, aff=0, init=False, out_slice=False,
         views=False, subset=False, thin=False, regimes=None):
    """aff: 0 none, 1 batch-1 vectors, "N" per image.  views: the sources are channel-slice-like views (batch stride, odd storage offset).
    subset: comparison (a) on the partial-tile / border pixels of the first and last image plus seeded others (large grids).
    expect: the variant dcvic_conv_last_variant reports (thin: 9200 + Cout / 9210 + Cin, the plan's own record)."""
    return dict(id=id, fam=fam, L=L, cins=list(cins), cout=cout, N=N, H=H, W=W, expect=expect, tuning=tuning, act=act, bias=bias, res=res,
                aff=aff, init=init, out_slice=out_slice, views=views, subset=subset, thin=thin, regimes=regimes)


# A tile other than the smallest of the best class is picked only once the grid nearly fills 1.5 x 256 CUs (variant_score: 358 workgroups
# make P = 256 beat P = 128), so those cases are many tiny images -- one or two tiles each -- with few input channels.
CASES = [
    # ---- generic conv_mfma_kernel, one case per (TC class, P); 8 x 17 = one ragged 8 x 32 tile per image, 4 x 33 = two 4 x 32 tiles
    case("g0_256_cin11_cout127", "generic", C3, [11], 127, 360, 8, 17, 256, subset=True, regimes=ALL_REGIMES),   # Cin 11: (tap, channel) order, last chunk masked; Cout TC - 1; plane 10 x 34 -> two staging slots
    case("g0_128_cout255", "generic", C3, [8], 255, 90, 4, 33, 128, subset=True),                  # two co-tiles, the second one channel short
    case("g0_64_k5_tapgroups", "generic", C5, [16], 128, 360, 1, 17, 64, subset=True),             # 5x5 on 128-channel tiles: 10 of 25 taps per weight stage (TG < T), H = 1
    case("g1_256_cin12_cout63", "generic", C3, [12], 63, 360, 8, 17, 1256, subset=True, act=ACT_RELU),   # Cin 8 m + 4
    case("g1_128_cout33", "generic", C3, [8], 33, 180, 4, 33, 1128, subset=True),
    case("g2_256_cin1_cout3", "generic", C3, [1], 3, 360, 8, 17, 2256, subset=True),               # Cin 1, Cout 3: one chunk of one channel, 3 of 32 rows
    case("g2_128_cout31", "generic", C3, [8], 31, 180, 9, 9, 2128, subset=True),                   # 16-wide tiles, 9 x 9 maps: partial in both directions
    case("g3_256_cout95", "generic", C3, [8], 95, 360, 8, 17, 3256, subset=True),
    case("g3_128_cout96", "generic", C3, [8], 96, 90, 9, 33, 3128, subset=True, res=True),
    # ---- the smallest tile (class 1, P = 64): every small launch.  Shapes: odd sides, smaller than a tile, more than one tile
    case("s_cin1_cout1_5x3", "generic", C3, [1], 1, 2, 5, 3, 1064, regimes=ALL_REGIMES),          # TWlog 2, Wout 3 < 4, Cin 1, Cout 1
    case("s_cin3_cout3_9x7", "generic", C3, [3], 3, 2, 9, 7, 1064),                                # TWlog 3, Wout 7 < 8
    case("s_cin11_cout65_9x9", "generic", C3, [11], 65, 2, 9, 9, 1064),                            # TWlog 4; Cout TC + 1: a second co-tile of one channel
    case("s_k3_cps2_ragged", "generic", C3, [24], 64, 2, 9, 9, 1064),                              # 3 chunks, 2 per stage: the last stage has one
    case("s_k1_cps8_ragged", "generic", C1, [84], 63, 3, 7, 9, 1064),                              # 1x1: 11 chunks, 8 per stage, 84 = 8 m + 4
    case("s_linear_1x1map", "generic", C1, [20], 12, 5, 1, 1, 1064),                               # Linear on a [B, in, 1, 1] map
    case("s_k5_cin20", "generic", C5, [20], 64, 2, 13, 11, 1064, act=ACT_LRELU02),                 # 5x5 s1 on odd sides, 8 m + 4 channels
    case("s_k5s2_even", "generic", C5S2, [16], 40, 2, 12, 10, 1064),
    case("s_k5s2_odd", "generic", C5S2, [3], 40, 2, 13, 11, 1064),
    case("s_k3s2_even", "generic", C3S2, [16], 24, 2, 12, 10, 1064),
    case("s_k3s2_odd", "generic", C3S2, [16], 24, 2, 13, 11, 1064),
    case("s_k1s2_odd", "generic", C1S2, [16], 24, 2, 13, 11, 1064),
    case("s_k1s2_even", "generic", C1S2, [16], 24, 2, 12, 10, 1064),
    case("s_k1_odd", "generic", C1, [16], 24, 2, 13, 11, 1064),
    case("s_k1_even", "generic", C1, [16], 24, 2, 12, 10, 1064),
    case("s_downsample_asym", "generic", layer("conv", 3, 2, 0, out_hw=(8, 6)), [16], 24, 2, 17, 12, 1064),   # F.pad (0, 1, 0, 1): the last row / column of taps falls outside on the even side only
    case("s_src2_inside_chunk", "generic", C3, [5, 7], 16, 2, 9, 9, 1064, views=True),             # boundaries inside a chunk: halves = 1
    case("s_src3_inside_chunk", "generic", C3, [3, 10, 7], 16, 2, 9, 9, 1064, views=True),
    case("s_src2_on_chunks", "generic", C3, [8, 16], 16, 2, 9, 9, 1064, views=True),               # on chunk boundaries: halves = 2
    case("s_src3_on_chunks", "generic", C3, [8, 8, 16], 16, 2, 9, 9, 1064, views=True),
    # ---- phase algebra
    case("p_convT5_odd", "phases", CT5, [16], 24, 2, 9, 7, 1064, regimes=ALL_REGIMES),
    case("p_convT3", "phases", CT3, [24], 16, 2, 7, 9, 1064),
    case("p_ups_phases", "phases", UPS, [16], 32, 2, 5, 7, 1064, act=ACT_SWISH),
    case("p_from_phases2", "phases", PH2, [12], 20, 2, 5, 7, 1064, bias=False),
    case("u_ups_template", "ups_template", UPS_TEMPLATE, [16], 32, 2, 5, 7, 1065, regimes=ALL_REGIMES),   # DCVIC_UPS_PHASES=0: conv_mfma_kernel<.., UPS = true>
    case("u_ups_template_cin12", "ups_template", UPS_TEMPLATE, [12], 20, 2, 6, 9, 1065, res=True),
    # ---- epilogue, on one tiny layer
    case("e_relu", "generic", C3, [8], 16, 2, 6, 6, 1064, act=ACT_RELU),
    case("e_lrelu", "generic", C3, [8], 16, 2, 6, 6, 1064, act=ACT_LRELU02, res=True),
    case("e_swish", "generic", C3, [8], 16, 2, 6, 6, 1064, act=ACT_SWISH, res=True, aff="N"),
    case("e_gelu", "generic", C3, [8], 16, 2, 6, 6, 1064, act=ACT_GELU),
    case("e_sigmoid", "generic", C3, [8], 16, 2, 6, 6, 1064, act=ACT_SIGMOID, aff=1),
    case("e_half_tanh", "generic", C3, [8], 16, 2, 6, 6, 1064, act=ACT_HALF_TANH),
    case("e_nobias_res", "generic", C3, [8], 16, 2, 6, 6, 1064, bias=False, res=True),
    case("e_init_nobias", "generic", C5, [8], 16, 2, 6, 6, 1064, bias=False, init=True),           # CHARM: a chain continued from another launch
    case("e_out_slice", "generic", C3, [8], 16, 2, 6, 6, 1064, out_slice=True, aff="N"),
    # ---- DMA tap kernels: P = 256 of class 0 / 3.  15 x 33: 2 x 2 tiles of 8 x 32 per image, three of them partial (taller ragged maps
    # go to the 2-row tiles); 7 x 17: one partial tile; three buffers in flight (conv3x3.hip,
    # DCVIC_CONV_STAGGER), so 3 and 5 chunks = 6 and 10 four-channel stages (5 eight-channel ones for the 2x2 phases): prologue, steady state, drain
    case("d_9000_src2_15x33", "dma3x3", C3, [8, 16], 128, 90, 15, 33, 9000, tuning=DMA, subset=True, act=ACT_RELU, res=True, regimes=ALL_REGIMES),
    case("d_9000_cin40_7x17", "dma3x3", C3, [40], 127, 360, 7, 17, 9000, tuning=DMA, subset=True),
    case("d_9003_cout96", "dma3x3", C3, [40], 96, 90, 15, 34, 9003, tuning=DMA, subset=True),
    case("d_9001_ups_phases", "dma3x3", UPS, [40], 97, 360, 7, 17, 9001, tuning=DMA, subset=True, regimes=("offset",)),
    # ---- conv1x1_dma_kernel: 13 x 20 = 260 pixels, a second 256-pixel tile of four; 3 chunks over 16-channel stages
    case("q_128_cin24", "dma1x1", C1, [24], 128, 128, 13, 20, 7000, tuning=DMA, subset=True, regimes=ALL_REGIMES),
    case("q_64_src3", "dma1x1", C1, [8, 12, 4], 64, 128, 13, 20, 7001, tuning=DMA, subset=True, act=ACT_GELU, res=True),
    case("q_96_cin40", "dma1x1", C1, [40], 96, 128, 13, 20, 7003, tuning=DMA, subset=True),
    case("q_fallback_hw273", "generic", C1, [24], 128, 128, 13, 21, 64, tuning=DMA, subset=True),  # H W % 4 != 0: not eligible
    # ---- async twins on the five geometries
    case("a32_k5", "async", C5, [20], 64, 2, 13, 11, 8102, tuning=ASYNC32, regimes=ALL_REGIMES),
    case("a32_k3", "async", C3, [24], 64, 2, 9, 9, 8102, tuning=ASYNC32, res=True),
    case("a32_k1", "async", C1, [84], 63, 3, 7, 9, 8102, tuning=ASYNC32),
    case("a32_k5s2", "async", C5S2, [16], 40, 2, 13, 11, 8102, tuning=ASYNC32),
    case("a32_convT5", "async", CT5, [16], 24, 2, 9, 7, 8102, tuning=ASYNC32),
    case("a16_k5", "async16", C5, [20], 64, 2, 13, 11, 8701, tuning=ASYNC16, regimes=ALL_REGIMES),  # class 2, P = 32
    case("a16_k3", "async16", C3, [24], 64, 2, 9, 9, 8701, tuning=ASYNC16, res=True),
    case("a16_k1", "async16", C1, [84], 63, 3, 7, 9, 8701, tuning=ASYNC16),
    case("a16_k5s2", "async16", C5S2, [16], 40, 2, 13, 11, 8701, tuning=ASYNC16),
    case("a16_convT5", "async16", CT5, [16], 24, 2, 9, 7, 8701, tuning=ASYNC16),
    case("a16_2_64", "async16", C3, [8], 1, 360, 4, 9, 8702, tuning=ASYNC16, subset=True),         # class 2, P = 64
    # ---- thin kernels (ops.THIN_MIN_PIXELS = 0): 17 x 70 = 2 x 2 tiles of 16 x 64, both partial
    case("t_cout1", "thin", C3, [8], 1, 2, 17, 70, 9201, thin=True, regimes=ALL_REGIMES),
    case("t_cout4", "thin", C3, [16], 4, 2, 17, 70, 9204, thin=True, act=ACT_RELU, res=True),
    case("t_cin1", "thin", C3, [1], 5, 2, 17, 70, 9211, thin=True),
    case("t_cin4", "thin", C3, [4], 40, 2, 17, 70, 9214, thin=True, act=ACT_SWISH),
]
for _i, _c in enumerate(CASES):
    if _c["regimes"] is None:
        _c["regimes"] = ("normal", OFF_REGIMES[_i % 3])
CASE_IDS = [c["id"] for c in CASES]
FAST_FAMILIES = ("dma3x3", "dma1x1", "async", "async16", "thin")      # re-asserted bit-equal to the generic kernel in every regime


def case_inputs(c, name, seed=11):
    """srcs, w, bias, res, affine (s, t, each [1 or N, Cout]), init of one case under a regime; `offset_zero_sum`: the offset input with
    weights that sum to zero over Cin at every tap."""
    L, N, H, W, cout = c["L"], c["N"], c["H"], c["W"], c["cout"]
    rname = "offset" if name == "offset_zero_sum" else name
    cin = sum(c["cins"])
    x = regime(rname, (N, cin, H, W), seed)
    srcs = [t.contiguous() for t in torch.split(x, c["cins"], 1)]
    kind, k = L["kind"], L["k"]
    if kind == "phases2":
        w = regime("normal", (4, cout, cin, 2, 2), seed + 1) * (cin * 4) ** -0.5
        cdim = 2
    elif kind == "convT":
        w = regime("normal", (cin, cout, k, k), seed + 1) * (cin * k * k / (4 if k == 5 else 1)) ** -0.5
        cdim = 0
    else:
        w = regime("normal", (cout, cin, k, k), seed + 1) * (cin * k * k) ** -0.5
        cdim = 1
    if name == "offset_zero_sum" and cin > 1:
        w = w - w.mean(cdim, keepdim=True)
    Hf, Wf = out_size(L, H, W)
    bias = regime("normal", (cout,), seed + 2) * 0.1 if c["bias"] else None
    res = regime(rname, (N, cout, Hf, Wf), seed + 3) if c["res"] else None
    aff = None
    if c["aff"]:
        nb = N if c["aff"] == "N" else 1
        aff = (regime("normal", (nb, cout), seed + 4) * 0.3, regime("normal", (nb, cout), seed + 5) * 0.3)
    init = regime(rname, (N, cout, Hf, Wf), seed + 6) if c["init"] else None
    return srcs, w, bias, res, aff, init


def case_plan(c, num_cu=256):
    """launch_plan of the case's (last) phase, or the thin route's record."""
    if c["thin"]:
        cin = sum(c["cins"])
        return dict(variant=9200 + c["cout"] if c["cout"] <= 4 and cin >= 8 else 9210 + cin)
    phases, _ = phases_of(c["L"], None, c["H"], c["W"])
    g = phases[-1]
    return launch_plan(g["desc"], c["cins"], c["cout"], c["N"], c["H"], c["W"], g["Hout"], g["Wout"], num_cu, c["tuning"], c["init"],
                       scatter=g["osy"] != 1, hw_vec=not c["views"])


def subset_pixels(c, seed=5):
    """The pixels of comparison (a) on a large grid: in the first and the last image every pixel on the map's border or in a partial
    tile (the tile of the launch, in full-output coordinates), plus max(1024, 4096 / Cout) seeded others."""
    p = case_plan(c)
    phases, (Hf, Wf) = phases_of(c["L"], None, c["H"], c["W"])
    s = phases[-1]["osy"]
    TW = (1 << p["TWlog"]) * s
    TH = (8 if p["variant"] in (9000, 9001, 9003) else p["P"] >> p["TWlog"]) * s
    if 7000 <= p["variant"] < 8000:
        flat = torch.arange(Hf * Wf)
        edge = (flat >= (Hf * Wf) // 256 * 256).reshape(Hf, Wf)
    else:
        edge = torch.zeros(Hf, Wf, dtype=torch.bool)
    oy, ox = torch.arange(Hf)[:, None], torch.arange(Wf)[None, :]
    edge = edge | (oy == 0) | (oy == Hf - 1) | (ox == 0) | (ox == Wf - 1) | (oy >= Hf // TH * TH) | (ox >= Wf // TW * TW)
    e = torch.nonzero(edge.reshape(-1))[:, 0]
    n_other = max(1024, 4096 // c["cout"] + 1)
    others = torch.randint(0, c["N"] * Hf * Wf, (n_other,), generator=torch.Generator().manual_seed(seed))
    return torch.unique(torch.cat([e, (c["N"] - 1) * Hf * Wf + e, others]))


def case_reference(c, name):
    """Everything the comparisons of one case and regime need, pixel-major: the inputs, idx (the pixels of comparison (a): all of them
    unless the case is a subset one), chain (conv_chain32 + epilogue32 at idx), ref and terms (conv_ref64 / terms64 through the fp64
    epilogue, every pixel) and k, the worst err / (U terms) of chain against ref."""
    srcs, w, bias, res, aff, init = case_inputs(c, name)
    L = c["L"]
    Hf, Wf = out_size(L, c["H"], c["W"])
    npx = c["N"] * Hf * Wf
    idx = subset_pixels(c) if c["subset"] else torch.arange(npx)
    n_all = torch.arange(npx) // (Hf * Wf)
    affp = None if aff is None else tuple(a[n_all] if a.shape[0] > 1 else a.expand(npx, -1) for a in aff)
    resp = None if res is None else pm(res)
    acc = layer_chain32(L, srcs, w, init, idx)
    assert not torch.isnan(acc).any(), "a pixel that no phase writes"
    chain = epilogue32(acc, bias, c["act"], None if resp is None else resp[idx], None if affp is None else tuple(a[idx] for a in affp))
    pre = pm(conv_ref64(L, srcs, w, init))
    ref = epilogue64(pre, bias, c["act"], resp, affp)
    terms = epilogue_terms(pm(terms64(L, srcs, w, init)), pre if bias is None else pre + bias.double()[None, :], bias, c["act"], resp, affp)
    k = float(((chain.double() - ref[idx]).abs() / (U * terms[idx] + 2.0 ** -126)).max())
    return dict(srcs=srcs, w=w, bias=bias, res=res, aff=aff, init=init, idx=idx, chain=chain, ref=ref, terms=terms, k=k)


def reached(c):
    """What a case reaches, derived from the case and its launch plan: the tags of REQUIRED."""
    L, cin, cout, p = c["L"], sum(c["cins"]), c["cout"], case_plan(c)
    v = p["variant"]
    Hf, Wf = out_size(L, c["H"], c["W"])
    tags = {f"act/{c['act']}"}
    geo = {"conv": f"k{L['k']}s{L['stride']}", "ups": "ups", "phases2": "from_phases2", "convT": f"convT{L['k']}"}[L["kind"]]
    if L["kind"] == "conv" and L["out_hw"] is not None:
        geo = "downsample_asym"
    if L["kind"] == "ups":
        geo = "ups_phases" if L["ups_phases"] else "ups_template"
    odd = "odd" if (c["H"] % 2 and c["W"] % 2) else ("even" if not (c["H"] % 2 or c["W"] % 2) else "mixed")
    tags |= {f"geo/{geo}", f"geo/{geo}/{odd}"}
    if c["thin"]:
        tags.add(f"thin/{'cout' if v < 9210 else 'cin'}/{v % 10}")
        return tags
    if v < 7000:
        tags.add(f"generic/{v // 1000}/{v % 1000 & ~1}")
        if v & 1:
            tags.add("generic/ups_template")
        if p["TG"] < p["T"] and CLASS_TC[p["cls"]] == 128:
            tags.add("generic/TG<T")
        if p["CPS"] > 1 and p["n_chunks"] % p["CPS"]:
            tags.add("generic/CPS_ragged")
        if p["nslots"] > 1:
            tags.add("generic/nslots>1")
        tags.add(f"generic/TWlog{p['TWlog']}")
        if phases_of(L, None, c["H"], c["W"])[0][-1]["Wout"] < (1 << p["TWlog"]):
            tags.add("generic/Wout<TW")
        if (Hf, Wf) == (1, 1):
            tags.add("generic/1x1map")
    elif v < 8000:
        tags.add(f"dma1x1/{CLASS_TC[v - 7000]}")
        if p["n_chunks"] % 2:
            tags.add("dma1x1/odd_chunks")
        if (c["H"] * c["W"]) % 256:
            tags.add("dma1x1/ragged_tile")
        if len(c["cins"]) == 3:
            tags.add("dma1x1/src3")
    elif v < 9000:
        tw = "async16" if v >= 8500 else "async32"
        tags |= {f"{tw}/{geo}", f"{tw}/{(v % 500) // 100}/{v % 100 * 32}"}
    else:
        tags.add(f"dma3x3/{v}")
    if c["L"] is C1 and c["tuning"] == DMA and v < 7000:
        tags.add("dma1x1/fallback")
    if cin in (1, 3, 11):
        tags.add(f"cin/{cin}")
    if cin % 8 == 4:
        tags.add("cin/8m+4")
    if len(c["cins"]) > 1:
        tags.add(f"src{len(c['cins'])}/halves{p['halves']}")
    if c["views"]:
        tags.add("src/views")
    TC = CLASS_TC[p["cls"]]
    for name, val in (("1", 1), ("3", 3)):
        if cout == val:
            tags.add(f"cout/{name}")
    if cout % TC == TC - 1:
        tags.add("cout/TC-1")
    if cout % TC == 1 and cout > TC:
        tags.add("cout/TC+1")
    if not c["bias"]:
        tags.add("epi/nobias")
    if c["res"]:
        tags.add("epi/res")
    if c["aff"]:
        tags.add(f"epi/aff{c['aff']}")
    if c["init"] and not c["bias"]:
        tags.add("epi/init_nobias")
    if c["out_slice"]:
        tags.add("epi/out_slice")
    return tags


REQUIRED = (
    [f"generic/{cls}/{P}" for cls, P in GENERIC_TILES] +
    ["generic/ups_template", "generic/TG<T", "generic/CPS_ragged", "generic/nslots>1", "generic/TWlog2", "generic/TWlog3", "generic/TWlog4",
     "generic/TWlog5", "generic/Wout<TW", "generic/1x1map",
     "cin/1", "cin/3", "cin/11", "cin/8m+4", "src2/halves1", "src3/halves1", "src2/halves2", "src3/halves2", "src/views",
     "cout/1", "cout/3", "cout/TC-1", "cout/TC+1",
     "geo/k1s1/odd", "geo/k1s2/odd", "geo/k1s2/even", "geo/k3s1/odd", "geo/k3s1/even", "geo/k3s2/odd", "geo/k3s2/even", "geo/k5s1/odd", "geo/k5s2/odd",
     "geo/k5s2/even", "geo/k1s1/even", "geo/k5s1/even", "geo/downsample_asym", "geo/convT5/odd", "geo/convT3", "geo/ups_phases", "geo/from_phases2"] +
    [f"act/{a}" for a in ALL_ACTS] +
    ["epi/nobias", "epi/res", "epi/aff1", "epi/affN", "epi/init_nobias", "epi/out_slice",
     "dma3x3/9000", "dma3x3/9001", "dma3x3/9003", "dma1x1/128", "dma1x1/64", "dma1x1/96", "dma1x1/odd_chunks", "dma1x1/ragged_tile", "dma1x1/src3",
     "dma1x1/fallback"] +
    [f"{tw}/{g}" for tw in ("async32", "async16") for g in ("k5s1", "k3s1", "k1s1", "k5s2", "convT5")] +
    ["async16/2/64", "async16/2/32", "thin/cout/1", "thin/cout/4", "thin/cin/1", "thin/cin/4"])


# ------------------------------------------------------------------------------------------------ data gradients (train/autograd._dgrad_plan)
def dcase(id, mod, cin, cout, k, s, p, H, W, N=2):
    """mod "conv" / "convT" / "linear" as dc_vic_amd.layers builds them; H x W: the FORWARD layer's input."""
    return dict(id=id, mod=mod, cin=cin, cout=cout, k=k, s=s, p=p, H=H, W=W, N=N)


DGRAD_CASES = [
    dcase("k1", "conv", 12, 20, 1, 1, 0, 7, 9),
    dcase("k3s1p1", "conv", 12, 20, 3, 1, 1, 7, 9),                # flipped, transposed weight
    dcase("k3s1p1_c16_24", "conv", 16, 24, 3, 1, 1, 7, 9),         # the adjoint is in the 3x3 order family (halves = 2)
    dcase("k4s1p1", "conv", 12, 20, 4, 1, 1, 8, 10),               # adjoint pad 2: g is 7 x 9
    dcase("k5s1p2", "conv", 12, 20, 5, 1, 2, 7, 9),
    dcase("k4s2p1_odd", "conv", 12, 20, 4, 2, 1, 10, 14),          # g is 5 x 7: four hand-indexed 2x2 phases
    dcase("k4s2p1_even", "conv", 12, 20, 4, 2, 1, 12, 16),         # g is 6 x 8
    dcase("k5s2p2_even", "conv", 12, 20, 5, 2, 2, 12, 16),         # the tape accepts even input sides only: adjoint = convT k5
    dcase("convT5", "convT", 12, 20, 5, 2, 2, 5, 7),               # adjoint = Conv2d(k5, s2, p2) on the 10 x 14 gradient
    dcase("convT3", "convT", 12, 20, 3, 1, 1, 7, 9),
    dcase("linear", "linear", 12, 20, 1, 1, 0, 3, 5),
]


def dgrad_forward_layer(d):
    return layer("convT", d["k"]) if d["mod"] == "convT" else layer("conv", d["k"], d["s"], d["p"])


def dgrad_weight(d, seed=21):
    cin, cout, k = d["cin"], d["cout"], d["k"]
    if d["mod"] == "convT":
        return regime("normal", (cin, cout, k, k), seed) * (cin * k * k / (4 if k == 5 else 1)) ** -0.5
    if d["mod"] == "linear":
        return regime("normal", (cout, cin), seed) * cin ** -0.5
    return regime("normal", (cout, cin, k, k), seed) * (cin * k * k) ** -0.5


def dgrad_layer(d, w):
    """The adjoint as _dgrad_plan builds it: (layer, weights) of the plan that maps the output's gradient to the input's.  Used for the
    yardstick k and sum|terms| only; the reference is fp64 autograd through conv_ref64 of the forward layer."""
    k, s, p = d["k"], d["s"], d["p"]
    if d["mod"] == "linear":
        return C1, w.t().contiguous()[:, :, None, None]
    if d["mod"] == "convT":
        return (C3 if k == 3 else C5S2), w
    if s == 1:
        return layer("conv", k, 1, k - 1 - p), w.flip(2, 3).transpose(0, 1).contiguous()
    if (k, s, p) == (4, 2, 1):
        ks = ((3, 1), (2, 0))
        wt = w.transpose(0, 1)
        return PH2, torch.stack([wt[:, :, list(ks[py])][:, :, :, list(ks[px])].contiguous() for py in (0, 1) for px in (0, 1)])
    assert (k, s, p) == (5, 2, 2)
    return CT5, w


def dgrad_ref64(d, w, g, x=None):
    """fp64 autograd of conv_ref64 of the forward layer at the output gradient g: -> (dx, y) with y = conv(x) (x: zeros unless given)."""
    L = dgrad_forward_layer(d)
    xx = (torch.zeros(d["N"], d["cin"], d["H"], d["W"]) if x is None else x).double().requires_grad_(True)
    w4 = w[:, :, None, None] if d["mod"] == "linear" else w
    y = conv_ref64(L, [xx], w4)
    assert y.shape == g.shape, (y.shape, g.shape)
    (dx,) = torch.autograd.grad(y, xx, g.double())
    return dx, y.detach()
