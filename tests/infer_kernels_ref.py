"""Plain torch restatements of the inference kernels (csrc/norm.hip, ew.hip, gemm.hip, attn.hip, swin.hip) on the CPU, at a chosen
precision: at float64 they are the references of tests/test_gpu_infer_kernels.py, at float32 its yardsticks -- the same sums in the
order class of the kernel (one sequential chain over k, online softmax over 64-key tiles, one max / sum pass), whose own error against
fp64 sets the measured bounds.  Also the kernels' loop and grid arithmetic restated in Python, and the shapes both test files use.

No GPU is needed here: tests/test_infer_kernels_host.py checks every restatement and every shape on the CPU."""
import math

import torch
import torch.nn.functional as F

from kernel_bounds import PEAK, U, regime

MARGIN = 4                        # measured bound = MARGIN x the fp32 restatement's worst error (tests/test_gpu_rate_train.py's convention)
FLOOR = 16                        # ... and never below FLOOR * U * max|ref|


def measured_bound(restated, ref):
    """The scalar bound of a measured check: 4 x the fp32 restatement's worst error against fp64 on this input, at least 16 U max|ref|."""
    ref = ref.double()
    own = float((restated.double() - ref).abs().max())
    return max(MARGIN * own, FLOOR * U * float(ref.abs().max())), own


# ------------------------------------------------------------------------------------------------ activations (common.h dcvic_act)
ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_SWISH, ACT_GELU, ACT_SIGMOID, ACT_HALF_TANH = range(7)


def act(a, v):
    """dcvic_act in the precision of v, written as the kernel writes it."""
    if a == ACT_RELU:
        return torch.clamp_min(v, 0)
    if a == ACT_LRELU02:
        return torch.where(v > 0, v, v * torch.tensor(0.2, dtype=torch.float32).to(v.dtype))
    if a == ACT_SWISH:
        return v / (1 + torch.exp(-v))
    if a == ACT_GELU:
        return 0.5 * v * (1 + torch.erf(v * 0.70710678118654752440))
    if a == ACT_SIGMOID:
        return 1 / (1 + torch.exp(-v))
    if a == ACT_HALF_TANH:
        return 0.5 * torch.tanh(v)
    return v


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_forward64(x, gamma, beta, groups, eps, swish):
    """fp64 GroupNorm (+ swish) of an fp32 map and the magnitudes of its derived bound: h = xh gamma + beta with xh = (x - mean) rstd;
    e_xh = |xh| + (|x| + |mean|) rstd is xh's error scale, as in tests/test_gpu_train_kernels.py gn_ref.  Returns y, e_xh, xh, the
    per-group E[x^2] / var (the factor of the fused statistics' error) and sum|terms| of the derived bound:
    (e_xh |gamma| + |beta|) [x 1.1 = max |swish'|, + |y| for the roundings of swish itself]."""
    N, Cc, H, W = x.shape
    X, Ga, Be = x.double(), gamma.double()[:, None, None], beta.double()[:, None, None]
    xg = X.reshape(N, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    var = xg.var(-1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    xh = ((xg - mean) * rstd).reshape(N, Cc, H, W)
    e_xh = xh.abs() + ((xg.abs() + mean.abs()) * rstd).reshape(N, Cc, H, W)
    h = xh * Ga + Be
    y = h * torch.sigmoid(h) if swish else h
    terms = e_xh * Ga.abs() + Be.abs()
    if swish:
        terms = 1.1 * terms + y.abs()
    ex2_var = ((xg * xg).mean(-1, keepdim=True) / (var + eps)).expand_as(xg).reshape(N, Cc, H, W)
    return y, e_xh, xh, ex2_var, terms


def gn_forward32(x, gamma, beta, groups, eps, swish, stats=None):
    """The kernel's apply pass in fp32 from fp64 statistics (or from `stats` = per-group (S, Q) fp64 sums): mean and var rounded to
    fp32, rstd = 1 / sqrtf(var + eps), ((x - mean) rstd gamma + beta), swish as v / (1 + expf(-v))."""
    N, Cc, H, W = x.shape
    xg = x.reshape(N, groups, -1)
    L = xg.shape[-1]
    if stats is None:
        S, Q = xg.double().sum(-1, keepdim=True), (xg.double() ** 2).sum(-1, keepdim=True)
    else:
        S, Q = stats
    mean_d = S / L
    mean = mean_d.float()
    var = torch.clamp_min(Q / L - mean_d * mean_d, 0.0).float()
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    xh = ((xg - mean) * rstd).reshape(N, Cc, H, W)
    h = xh * gamma[:, None, None] + beta[:, None, None]
    return act(ACT_SWISH, h) if swish else h


def gn_loop_counts(C, HW, groups, B=512):
    """groupnorm_kernel's vector apply loop walked thread by thread: per thread the 4-way-unrolled iterations, the tail iterations and
    how often step() wraps (j >= hw4); asserts that the incrementally advanced channel equals i // hw4 at every element the thread
    touches.  -> dict of min / max over the threads, n4 and sc."""
    cg = C // groups
    assert HW % 4 == 0
    hw4, n4 = HW // 4, cg * HW // 4
    sc, sj = B // hw4, B - (B // hw4) * hw4
    un, tail, wraps = [], [], []
    for tid in range(B):
        c, j = tid // hw4, tid - (tid // hw4) * hw4
        u = t = w = 0

        def step():
            nonlocal c, j, w
            c += sc
            j += sj
            if j >= hw4:
                j -= hw4
                c += 1
                w += 1
        i = tid
        while i + 3 * B < n4:
            for q in range(4):
                assert c == (i + q * B) // hw4 and c < cg, (tid, i, q, c)
                step()
            u += 1
            i += 4 * B
        while i < n4:
            assert c == i // hw4 and c < cg, (tid, i, c)
            step()
            t += 1
            i += B
        un.append(u); tail.append(t); wraps.append(w)
    return dict(n4=n4, sc=sc, unrolled_min=min(un), unrolled_max=max(un), tail_min=min(tail), tail_max=max(tail), wraps_max=max(wraps),
                wraps_min=min(wraps))


# N, C, H, W, groups and the path of groupnorm_kernel the case is listed for; every case runs dense, through a 16-byte-aligned
# batch-strided view (vector path) and through a misaligned one (scalar path)
GN_CASES = [
    dict(N=2, C=64, H=64, W=64, groups=32, path="unrolled_sc0"),          # group 8192 floats, HW/4 = 1024 > 512: sc == 0, every thread unrolled once
    dict(N=2, C=512, H=12, W=20, groups=8, path="unrolled_twice_wraps"),  # n4 = 3840: threads 0..255 run the unrolled loop twice (c, j carried over),
                                                                          # the others once and then the tail; HW/4 = 60, sc = 8, sj = 32: step() wraps about every other call
    dict(N=1, C=76, H=16, W=24, groups=4, path="unrolled_beside_tail_only"),   # n4 = 1824: threads 0..287 unrolled once, threads 288..511 ONLY the tail, three iterations
    dict(N=2, C=66, H=9, W=7, groups=6, path="scalar"),                   # HW % 4 != 0
    dict(N=3, C=40, H=4, W=8, groups=5, path="short"),                    # n4 = 64 < 512: most threads idle, no unrolled iteration
]
GN_VIEWS = (None, (8, 4), (8, 1))


# ------------------------------------------------------------------------------------------------ fused GroupNorm statistics
def fused_stats(y):
    """The F(4x4) epilogue's GroupNorm partials of an fp32 map [N, C, H, W] (csrc/wino44.hip), emulated: per channel and 16 x 32 tile,
    lane e of 16 adds the 32 values of its two 4 x 4 blocks (block t = blk * 16 + e at rows 4 (t >> 3), columns 4 (t & 7); rows then
    columns) in one fp32 chain -- sum and fused-multiply-add sum of squares --, four xor-shuffle levels add the lanes, and the tiles
    are added in fp64 (groupnorm_kernel).  Pixels outside the map add nothing.  -> per-channel (S, Q) in fp64."""
    N, C, H, W = y.shape
    Hp, Wp = -(-H // 16) * 16, -(-W // 32) * 32
    yp = F.pad(y, (0, Wp - W, 0, Hp - H))
    # [N, C, ty, blkrow(4), i(4), tx, blkcol(8), j(4)] -> lanes e = (blkrow & 1) * 8 + blkcol, blk = blkrow >> 1
    t = yp.reshape(N, C, Hp // 16, 2, 2, 4, Wp // 32, 8, 4).permute(0, 1, 2, 6, 4, 7, 3, 5, 8)   # N C ty tx (blkrow&1) blkcol blk i j
    t = t.reshape(N, C, Hp // 16, Wp // 32, 16, 32)
    s = torch.zeros(t.shape[:-1], dtype=torch.float32)
    q = torch.zeros_like(s)
    for k in range(32):
        v = t[..., k]
        s = s + v
        q = (v.double() * v.double() + q.double()).float()             # fmaf: one rounding
    for o in (1, 2, 4, 8):
        idx = torch.arange(16) ^ o
        s = s + s[..., idx]
        q = q + q[..., idx]
    return s[..., 0].double().sum((2, 3)), q[..., 0].double().sum((2, 3))


def group_stats(S, Q, groups):
    """Per-channel fp64 sums -> per-group sums shaped [N, groups, 1]."""
    N, C = S.shape
    return S.reshape(N, groups, -1).sum(-1, keepdim=True), Q.reshape(N, groups, -1).sum(-1, keepdim=True)


FUSED_RATIOS = (0, 3, 10, 30, 100)
FUSED_HOLDS_TO = 10               # up to this |mean| / std the fused statistics keep 2e-6 of the output's maximum
FUSED_TOL = 2e-6


def fused_stats_error(ratio, C, H, W, groups, seed=0):
    """Emulated: GroupNorm + swish of a unit-variance map shifted to |mean| / std = ratio, from the fused statistics against the same
    apply pass from fp64 statistics; the difference relative to the output's maximum."""
    x = regime("normal", (1, C, H, W), seed) + float(ratio)
    gamma, beta = torch.ones(C), torch.zeros(C)
    a = gn_forward32(x, gamma, beta, groups, 1e-6, True)
    b = gn_forward32(x, gamma, beta, groups, 1e-6, True, stats=group_stats(*fused_stats(x), groups))
    return float((a - b).abs().max() / a.abs().max())


# ------------------------------------------------------------------------------------------------ launch grids of ew.hip
def ew_passes(CHW):
    """Grid-stride passes of ew_kernel's busiest thread: grid.x = min(2048, ceil(CHW / 256))."""
    grid = min(2048, -(-CHW // 256))
    return -(-CHW // (grid * 256))


def plane_passes(pixels):
    """... of chan_affine / copy_planes / copy_window: grid.x = min(64, ceil(pixels / 256)) per plane."""
    grid = min(64, -(-pixels // 256))
    return -(-pixels // (grid * 256))


def crop_passes(total):
    """... of crop_clamp: grid.x = min(1024, ceil(C outH outW / 256))."""
    grid = min(1024, -(-total // 256))
    return -(-total // (grid * 256))


# shapes [N, C, H, W]: once above each grid-stride threshold, once ragged below it
EW_BIG = (2, 3, 419, 419)         # C*HW = 526683 > 2048 * 256: a second, partial pass
EW_SMALL = (3, 5, 7, 11)          # 385 elements: one ragged block and a half
PLANE_BIG = (2, 3, 129, 131)      # 16899 pixels per plane > 64 * 256
PLANE_SMALL = (3, 5, 7, 11)
CROP_BIG = (2, 3, 300, 301)       # crop to 297 x 299: 266409 > 1024 * 256
CROP_BIG_OUT = (297, 299)
CROP_SMALL = (3, 3, 9, 13)
CROP_SMALL_OUT = (7, 10)


# ------------------------------------------------------------------------------------------------ bgemm
def gemm_chain(A, B, alpha, dtype=torch.float32):
    """alpha * sum_k A[b][m][k] B[b][k][n] as ONE chain over k ascending in `dtype` (the kernel: one fma per term), alpha last."""
    A, B = A.to(dtype), B.to(dtype)
    acc = torch.zeros(A.shape[0], A.shape[1], B.shape[2], dtype=dtype)
    for k in range(A.shape[2]):
        acc = acc + A[:, :, k:k + 1] * B[:, k:k + 1, :]
    return torch.tensor(alpha, dtype=torch.float32).to(dtype) * acc


def gemm_ref64(A, B, alpha):
    """fp64 product, and |alpha| sum_k |a b| for the derived bound of the epilogue."""
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    acc = A.double() @ B.double()
    return a32 * acc, acc


# The stride patterns of the product, by call site.  Per batch item the logical A [M, K] lies in memory either row-major
# (a_ms = K, a_ks = 1: "a_kfast") or as [K][M] (a_ms = 1, a_ks = M); B [K, N] row-major (b_ks = N, b_ns = 1) or as [N][K] (b_ks = 1,
# b_ns = K: "b_kfast").  An operand "in the map" is one third of a [batch, 3, plane] buffer (q | k | v of one [N, 3C, HW] map: batch
# stride 3 x its plane), else dense.  name: (a transposed, b transposed, a in map, b in map, c in map)
GEMM_PATTERNS = {
    "vqgan_scores": (True, False, True, True, False),      # vqgan.py:85       St = c^-0.5 k^T q
    "vqgan_values": (False, False, True, False, False),    # vqgan.py:89       h = v St
    "tape_scores": (True, False, True, True, False),       # autograd.py:505   the same product recomputed by the backward
    "tape_dV": (False, True, False, False, True),          # autograd.py:510   dV = dO St^T
    "tape_dSt": (True, False, True, False, False),         # autograd.py:513   dSt = v^T dO
    "tape_dQ": (False, False, True, False, True),          # autograd.py:516   dQ = k dS
    "tape_dK": (False, True, True, False, True),           # autograd.py:517   dK = q dS^T
    "a_strided_b_kfast": (True, True, False, False, False),  # the fourth staging layout (no call site)
}
GEMM_SIZES = (1, 63, 64, 65, 150)
GEMM_KS = (1, 15, 16, 17, 150)


# ------------------------------------------------------------------------------------------------ softmax over C of [N, C, P]
def softmax_c_onepass(x, dtype=torch.float32):
    """One max pass, one sum of exp(x - M), exp(x - M) * (1 / S), in `dtype`."""
    x = x.to(dtype)
    M = x.amax(1, keepdim=True)
    e = torch.exp(x - M)
    return e * (1 / e.sum(1, keepdim=True))


SOFTMAX_CS = (1, 3, 5, 200)
SOFTMAX_PS = (1, 63, 64, 65, 257)
SOFTMAX_REGIMES = ("normal", "flat", "wide", "peak_first")


def softmax_input(name, N, C, P, seed):
    """[N, C, P] scores whose rows (the softmax runs over C) follow a score regime."""
    return regime(name, (N, P, C), seed).transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ fused attention
def attn_inputs(name, N, C, HW, seed):
    """A [N, 3C, HW] q | k | v map whose scaled scores C^-0.5 q.k follow a score regime: `normal` unit-variance q, k (scores of unit
    variance); `flat` q = 0; `wide` q x 20; `peak_*`: channel 0 of k is zero except at one key per image (first / last 64-key tile),
    where it is C^0.5, and channel 0 of q is 60 + its randn value: that key's score stands 60 above the others for every query."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((N, 3 * C, HW), generator=g)
    if name == "flat":
        qkv[:, :C] = 0.0
    elif name == "wide":
        qkv[:, :C] *= 20.0
    elif name in ("peak_first", "peak_last"):
        lo = 0 if name == "peak_first" else HW - 64
        j = torch.randint(lo, lo + 64, (N,), generator=g)
        qkv[:, C] = 0.0
        qkv[torch.arange(N), C, j] = float(C) ** 0.5
        qkv[:, 0] += PEAK
    elif name != "normal":
        raise ValueError(name)
    return qkv


def attn_queries(HW):
    """The queries a case is checked at: all of them up to 128 tokens, else the first and last 16-query wave, the last wave of the
    first 64-query block and one in the middle (the restatement's chains cost queries x keys x C)."""
    if HW <= 128:
        return torch.arange(HW)
    starts = (0, 48, HW // 2 + 16, HW - 16)
    return torch.cat([torch.arange(s, s + 16) for s in starts])


def attn_ref64(qkv, C, queries):
    """fp64: softmax_j(C^-0.5 q_i . k_j) v_j for the chosen queries -> [N, C, len(queries)]."""
    scale = float(torch.tensor(float(int(C) ** -0.5), dtype=torch.float32))
    q, k, v = qkv[:, :C].double(), qkv[:, C:2 * C].double(), qkv[:, 2 * C:].double()
    S = scale * (q[:, :, queries].transpose(1, 2) @ k)                  # [N, Q, HW]
    return v @ torch.softmax(S, -1).transpose(1, 2)


def attn_online(qkv, C, queries, dtype=torch.float32):
    """attn_fused_kernel's arithmetic in `dtype`: per 64-key tile the scores as one chain over the channels, then scale, the running
    maximum, alpha = exp(m_old - m_new), p = exp(s - m_new), l = l alpha + sum p, O = O alpha, then every key of the tile added
    onto the running O: ONE chain over all HW keys, as in the kernel.  (Summing each tile's value product from zero and adding the
    tile sums is a two-level sum, more accurate than the kernel's chain: with equal weights over 1024 / 6144 keys the kernel stood at
    1.08 / 1.94 of the bound measured against that form on MI355X.)  out = O / l."""
    scale = torch.tensor(float(int(C) ** -0.5), dtype=torch.float32).to(dtype)
    q, k, v = qkv[:, :C].to(dtype), qkv[:, C:2 * C].to(dtype), qkv[:, 2 * C:].to(dtype)
    N, _, HW = q.shape
    qs = q[:, :, queries]                                               # [N, C, Q]
    Q = qs.shape[-1]
    m = torch.full((N, Q), -math.inf, dtype=dtype)
    l = torch.zeros((N, Q), dtype=dtype)
    O = torch.zeros((N, C, Q), dtype=dtype)
    Sall = torch.zeros((N, HW, Q), dtype=dtype)                         # S^T[key][query], every tile's chain at once
    for c in range(C):
        Sall = Sall + k[:, c, :, None] * qs[:, c, None, :]
    Sall = Sall * scale
    for j0 in range(0, HW, 64):
        S = Sall[:, j0:j0 + 64]
        m_new = torch.maximum(m, S.amax(1))
        alpha = torch.exp(m - m_new)
        p = torch.exp(S - m_new[:, None, :])
        l = l * alpha + p.sum(1)
        m = m_new
        O = O * alpha[:, None, :]
        for j in range(64):
            O = O + v[:, :, j0 + j, None] * p[:, j, None, :]
    return O / l[:, None, :]


# C, HW (H, W), N: block counts N * HW / 64 divisible by 8 and not; the 64 x 96 map once, at C = 512
ATTN_CASES = [(C, hw, N) for C in (128, 256, 512) for hw, N in (((8, 8), 3), ((8, 16), 4), ((32, 32), 1))] + [(512, (64, 96), 1)]
ATTN_REGIMES = ("normal", "flat", "wide", "peak_first", "peak_last")


# ------------------------------------------------------------------------------------------------ Swin window attention
def swin_forward(qkv, table, heads, shift, dtype=torch.float32):
    """swin_attn_kernel in `dtype` (window 8, head dim 16): q * 0.25, the score as one chain over the head dim, + relative bias, - 100
    across the regions of a shifted window, one max / sum pass, p = e * (1 / sum), the output as one chain over the 64 tokens."""
    ws, hd = 8, 16
    N, C3, H, W = qkv.shape
    Cc, T = C3 // 3, 64
    xs = torch.roll(qkv.to(dtype), (-shift, -shift), (2, 3))
    nWy, nWx = H // ws, W // ws
    win = xs.reshape(N, 3, heads, hd, nWy, ws, nWx, ws).permute(1, 0, 4, 6, 2, 5, 7, 3).reshape(3, N * nWy * nWx, heads, T, hd)
    q, k, v = win[0] * 0.25, win[1], win[2]
    ty, tx = torch.arange(T) // ws, torch.arange(T) % ws
    rel = (ty[:, None] - ty[None, :] + ws - 1) * (2 * ws - 1) + (tx[:, None] - tx[None, :] + ws - 1)
    S = torch.zeros(q.shape[:-1] + (T,), dtype=dtype)
    for d in range(hd):
        S = S + q[..., :, None, d] * k[..., None, :, d]
    S = S + table.to(dtype)[rel].permute(2, 0, 1)[None]
    if shift > 0:
        lab = torch.zeros(H, W, dtype=torch.long)
        for i, ys in enumerate((slice(0, H - ws), slice(H - ws, H - shift), slice(H - shift, H))):
            for j, xsl in enumerate((slice(0, W - ws), slice(W - ws, W - shift), slice(W - shift, W))):
                lab[ys, xsl] = i * 3 + j
        lw = lab.reshape(nWy, ws, nWx, ws).permute(0, 2, 1, 3).reshape(nWy * nWx, T)
        mask = (lw[:, :, None] != lw[:, None, :]).to(dtype) * -100.0
        S = S + mask.repeat(N, 1, 1)[:, None]
    e = torch.exp(S - S.amax(-1, keepdim=True))
    p = e * (1 / e.sum(-1, keepdim=True))
    o = torch.zeros(q.shape, dtype=dtype)
    for j in range(T):
        o = o + p[..., :, j, None] * v[..., None, j, :]
    out = o.reshape(N, nWy, nWx, heads, ws, ws, hd).permute(0, 3, 6, 1, 4, 2, 5).reshape(N, Cc, H, W)
    return torch.roll(out, (shift, shift), (2, 3))


SWIN_CS = (32, 96, 128)           # heads 2, 6, 8
SWIN_MAPS = ((8, 8), (8, 24), (24, 16))
SWIN_REGIMES = {"normal": 1.0, "wide": 4.5}   # scale of q and k: 0.25 q.k over 16 channels has std 1 / std 20


def swin_inputs(name, N, Cc, H, W, seed):
    """A [N, 3C, H, W] qkv map whose scores 0.25 q.k (16 channels per head) have unit variance (`normal`) or std about 20 (`wide`)."""
    x = regime("normal", (N, 3 * Cc, H, W), seed)
    x[:, :2 * Cc] *= SWIN_REGIMES[name]
    return x


# ------------------------------------------------------------------------------------------------ Winograd routes
# route: (Cin, Cout, H, W of the input, N, upsample, residual); ragged: partial 8 x 32 / 16 x 32 tiles, Cout not a multiple of 64
WINO_ROUTE_CASES = {
    "wino": (64, 96, 19, 36, 2, False, True),
    "wino_ups": (64, 96, 9, 20, 2, True, True),
    "wino44": (64, 96, 19, 36, 2, False, True),
    "wino44_ups": (64, 96, 9, 20, 2, True, True),
}
WINO_BOUND = {"wino": 2e-6, "wino_ups": 2e-6, "wino44": 1.2e-5, "wino44_ups": 1.2e-5}   # the bounds tests/test_gpu_kernels.py and test_gpu_wino44_ups.py state
WINO_REGIMES = ("offset", "outlier", "swish", "offset_zero_sum")


def wino_inputs(name, route, seed):
    """x, w, b, r of one route's case under a regime; `offset_zero_sum`: the offset input with weights that sum to zero over Cin at
    every tap (the offsets then cancel in the exact result and only their roundings remain)."""
    Cin, Cout, H, W, N, ups, res = WINO_ROUTE_CASES[route]
    x = regime("offset" if name == "offset_zero_sum" else name, (N, Cin, H, W), seed)
    w = regime("normal", (Cout, Cin, 3, 3), seed + 1) * (Cin * 9) ** -0.5
    if name == "offset_zero_sum":
        w = w - w.mean(1, keepdim=True)
    b = regime("normal", (Cout,), seed + 2) * 0.1
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    r = regime("offset" if name == "offset_zero_sum" else name, (N, Cout, Ho, Wo), seed + 3) if res else None
    return x, w, b, r


def conv_ref64(x, w, b, r, ups):
    xd = x.double()
    if ups:
        xd = F.interpolate(xd, scale_factor=2, mode="nearest")
    y = F.conv2d(xd, w.double(), b.double(), padding=1)
    return y + r.double() if r is not None else y
