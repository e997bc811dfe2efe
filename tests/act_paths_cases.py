"""The cases tests/test_gpu_act_paths.py replays and tools/record_act_golden.py records: every kernel path that applies dcvic_act
(csrc/common.h) -- the GroupNorm apply pass, the convolution epilogues of every family ConvPlan can route to, the thin kernels and the
elementwise kernel -- under every activation, with and without bias, residual and affine where the family takes them.

A case is pinned by the SHA-256 of its output bytes (tests/golden/act_paths.json, recorded on the build BEFORE the activation switch
was hoisted out of the per-value code): the hoist must leave every output bit where it was.  The inputs are seeded and carry the
values at which an activation's expression can change: +0 and -0, subnormals, |v| on both sides of 88 (where expf overflows) and
ordinary values, placed so that they reach the activation itself (GroupNorm: through gamma / beta; convolutions: through zero weight
rows and the bias).

A plain module: nothing that needs a GPU at import.  The shapes are the smallest that route to each family with N = 2, a channel
count that is no multiple of the co-tile and a map that is no multiple of the pixel tile; the DMA kernels only run once their grid
fills the 256 CUs, which is what makes their maps large."""
import hashlib
import json
import os

import torch

import conv_direct_ref as R
from infer_kernels_ref import act as act_fn

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "act_paths.json")
ACTS = tuple(R.ALL_ACTS)
ACT_NAMES = ("none", "relu", "lrelu02", "swish", "gelu", "sigmoid", "half_tanh")
EDGE = (88.6, -0.0, 1e-40, -88.73, -103.5, 0.0, -1e-40, 87.3)     # expf(88.73) overflows fp32, expf(88.6) does not; 1e-40 is subnormal


def sprinkle(t, step=97):
    """+0, -0 and the two subnormals at every `step`-th element of t (in place)."""
    f = t.view(-1)
    for k, v in enumerate((0.0, -0.0, 1e-40, -1e-40)):
        f[k::step] = v
    return t


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ GroupNorm
EPS = 1e-6
GN_SHAPES = {
    # float4 path: len = 2 * 64 * 66 = 8448, n4 = 2112 > 3 * 512 (the 4x-unrolled loop AND the tail loop run); hw4 = 1056 is no multiple
    # of 512, so a channel boundary falls inside a thread's stride
    "vec": dict(N=2, C=4, groups=2, H=64, W=66, part=False),
    "scalar": dict(N=2, C=6, groups=3, H=5, W=7, part=False),
    "part": dict(N=2, C=4, groups=2, H=64, W=66, part=True),
}
N_PT = 3


def gn_inputs(name):
    s = GN_SHAPES[name]
    g = torch.Generator().manual_seed(4100 + len(name))
    x = sprinkle(torch.randn((s["N"], s["C"], s["H"], s["W"]), generator=g) * 1.5 + 0.3)
    # channel 0 ordinary; 1: the normalised values (about +-3) times 40 cross +-88 and -103; 2: gamma 0 and beta -0 (the products are
    # +-0); 3: a subnormal gamma; 4, 5 (scalar case): gamma 0 and beta on either side of the expf overflow edge
    gamma = torch.tensor([1.1, 40.0, 0.0, 1e-39, 0.0, 0.0][:s["C"]])
    beta = torch.tensor([0.1, -3.0, -0.0, 0.0, 88.6, -88.73][:s["C"]])
    part = None
    if s["part"]:
        part = torch.stack([torch.randn((s["N"], s["C"], N_PT), generator=g) * 300.0,
                            torch.rand((s["N"], s["C"], N_PT), generator=g) * 4000.0 + 3000.0], dim=-1).contiguous()
    return x, gamma, beta, part


def gn_ids():
    return [f"gn/{name}/{ACT_NAMES[a]}/{'inplace' if inplace else 'out'}" for name in GN_SHAPES for a in ACTS for inplace in (False, True)]


def gn_run(name, a, inplace, dev_inputs):
    from dc_vic_amd import ops
    s = GN_SHAPES[name]
    x, gamma, beta, part = dev_inputs
    xin = x.clone()
    y = ops.groupnorm(xin, gamma, beta, groups=s["groups"], eps=EPS, act=a, out=xin if inplace else None,
                      part=None if part is None else (part, N_PT))
    torch.cuda.synchronize()
    return y


def gn_ref64(name, a):
    s = GN_SHAPES[name]
    x, gamma, beta, part = gn_inputs(name)
    N, C, G = s["N"], s["C"], s["groups"]
    xg = x.double().reshape(N, G, -1)
    if part is None:
        mean, ex2 = xg.mean(-1), (xg * xg).mean(-1)
    else:
        p = part.double().reshape(N, G, -1, 2)
        mean, ex2 = p[..., 0].sum(-1) / xg.shape[-1], p[..., 1].sum(-1) / xg.shape[-1]
    var = (ex2 - mean * mean).clamp_min(0).float().double()
    mean = mean.float().double()
    rstd = (1.0 / torch.sqrt((var + EPS).float())).double()
    h = ((xg - mean[..., None]) * rstd[..., None]).reshape(N, C, s["H"], s["W"])
    return act_fn(a, h * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None])


# ------------------------------------------------------------------------------------------------ convolutions
def _case(fam, L, cins, cout, H, W, expect, tuning=R.GENERIC, aff=True, thin=False, wino=False):
    """aff: whether the family takes the affine epilogue.  expect: the variant dcvic_conv_last_variant reports (thin / wino: the
    plan's own record, ops.conv_kernel_name)."""
    c = R.case(fam, fam, L, cins, cout, 2, H, W, expect, tuning=tuning, thin=thin)
    c.update(aff_ok=aff, wino=wino)
    return c


CONV_CASES = [
    _case("direct", R.C3, [8], 17, 9, 9, 1064),                                        # conv_mfma_kernel, class 1, P = 64
    _case("async", R.C3, [24], 63, 9, 9, 8102, tuning=R.ASYNC32),                      # conv_mfma_async_kernel
    _case("async16", R.C3, [24], 63, 9, 9, 8701, tuning=R.ASYNC16),                    # conv_mfma_async16_kernel, class 2, P = 32
    # conv1x1_dma_kernel needs a workgroup per CU: 130 x 254 = 33020 pixels = 128.98 tiles of 256
    _case("dma1x1_128", R.C1, [24], 127, 130, 254, 7000, tuning=R.DMA),
    _case("dma1x1_64", R.C1, [24], 63, 130, 254, 7001, tuning=R.DMA),
    _case("dma1x1_96", R.C1, [24], 95, 130, 254, 7003, tuning=R.DMA),
    # conv3x3_dma_kernel: the 256-pixel tile wins from about 358 workgroups on: 13 x 17 tiles of 8 x 32 per image, the last row and
    # column of tiles partial
    _case("dma3x3", R.C3, [8], 127, 103, 513, 9000, tuning=R.DMA),
    _case("wino", R.C3, [8], 50, 9, 36, 9100, aff=False, wino=True),                   # F(2x2): 8 x 32-pixel tiles, 64-channel co-tiles
    _case("thin_cout", R.C3, [16], 4, 17, 70, 9204, aff=False, thin=True),
    _case("thin_cin", R.C3, [4], 40, 17, 70, 9214, aff=False, thin=True),
]
CONV_BY_ID = {c["id"]: c for c in CONV_CASES}


def conv_combos(c):
    """(bias, res, aff) of one family."""
    return [(b, r, f) for b in (True, False) for r in (False, True) for f in ((False, True) if c["aff_ok"] else (False,))]


def conv_id(c, a, combo):
    b, r, f = combo
    return f"conv/{c['id']}/{ACT_NAMES[a]}/{'bias' if b else 'nobias'}{'+res' if r else ''}{'+aff' if f else ''}"


def conv_ids():
    return [conv_id(c, a, cb) for c in CONV_CASES for a in ACTS for cb in conv_combos(c)]


def conv_inputs(c):
    """x, w, bias, res, (s, t) on the CPU.  Output channels with a zero weight row see exactly their bias (EDGE) at the activation; one
    row times 60 spreads its channel across +-88."""
    cin, cout, N, H, W = sum(c["cins"]), c["cout"], c["N"], c["H"], c["W"]
    k = c["L"]["k"]
    g = torch.Generator().manual_seed(5200 + cout + 7 * cin)
    x = sprinkle(torch.randn((N, cin, H, W), generator=g))
    w = torch.randn((cout, cin, k, k), generator=g) * (cin * k * k) ** -0.5
    bias = torch.randn((cout,), generator=g) * 0.1
    n_edge = len(EDGE) if cout >= 12 else 1
    w[:n_edge] = 0.0
    bias[:n_edge] = torch.tensor(EDGE[:n_edge])
    w[n_edge] *= 60.0
    res = sprinkle(torch.randn((N, cout, H, W), generator=g), 89)
    aff = (torch.randn((N, cout), generator=g) * 0.3, torch.randn((N, cout), generator=g) * 0.3)
    return x, w, bias, res, aff


class ConvRunner:
    """One family's plan and inputs on the device; run(act, combo) -> (output, kernel names of the launch)."""

    def __init__(self, c):
        from dc_vic_amd import ops
        self.c = c
        x, w, bias, res, aff = conv_inputs(c)
        self.srcs = [t.contiguous().to(DEV) for t in torch.split(x, c["cins"], 1)]
        self.res = res.to(DEV)
        self.aff = tuple(t.to(DEV).contiguous() for t in aff)
        k = c["L"]["k"]
        self.plan = ops.ConvPlan(w.to(DEV), bias.to(DEV), "conv", stride=1, pad=(k // 2, k // 2))
        if c["wino"]:
            self.plan.wino = "force"

    def run(self, a, combo):
        from dc_vic_amd import ops
        from dc_vic_amd._lib import lib
        c = self.c
        b, r, f = combo
        keep = ops.THIN_ENABLED, ops.THIN_MIN_PIXELS
        ops.THIN_ENABLED, ops.THIN_MIN_PIXELS = bool(c["thin"]), 0
        lib().dcvic_conv_set_tuning(*c["tuning"])
        ops.kernel_events_start()
        try:
            y = self.plan(self.srcs, act=a, res=self.res if r else None, affine=self.aff if f else None, use_bias=b)
            torch.cuda.synchronize()
        finally:
            names = list(ops.kernel_events_stop())
            lib().dcvic_conv_set_tuning(*R.TUNING_DEFAULT)
            ops.THIN_ENABLED, ops.THIN_MIN_PIXELS = keep
        return y, names


def conv_expected_kernel(c):
    from dc_vic_amd import ops
    return ops.conv_kernel_name(c["expect"])


def conv_ref64(c, a, combo):
    b, r, f = combo
    x, w, bias, res, aff = conv_inputs(c)
    pre = R.conv_ref64(c["L"], [x], w)
    N, Co, H, W = pre.shape
    n_all = torch.arange(N * H * W) // (H * W)
    y = R.epilogue64(R.pm(pre), bias if b else None, a, R.pm(res) if r else None, tuple(t[n_all] for t in aff) if f else None)
    return y.reshape(N, H, W, Co).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ elementwise
EW_DEFAULT_OPS = (4,)             # dcvic_ew_f32 accepts op 0, 1, 2 and 4; 4 (activation) is the one that reaches the default arm
EW_SHAPE = (2, 3, 33, 35)         # 3465 values per image: 14 workgroups of 256, the last one partial


def ew_inputs():
    g = torch.Generator().manual_seed(6300)
    x = sprinkle(torch.randn(EW_SHAPE, generator=g) * 30.0)          # N(0, 30^2): values on both sides of +-88
    x.view(-1)[5:5 + len(EDGE)] = torch.tensor(EDGE)
    return x


def ew_ids():
    return [f"ew/op{op}/{ACT_NAMES[a]}" for op in EW_DEFAULT_OPS for a in ACTS]


def ew_run(op, a, x_dev):
    from dc_vic_amd import ops
    y = ops._ew(op, x_dev, None, None, act=a)
    torch.cuda.synchronize()
    return y


def all_ids():
    return gn_ids() + conv_ids() + ew_ids()


def record():
    """Every case on the current build -> {id: sha256 of the output bytes}; asserts that each convolution reached its family's kernel."""
    out = {}
    for name in GN_SHAPES:
        dev = tuple(None if t is None else t.to(DEV) for t in gn_inputs(name))
        for a in ACTS:
            for inplace in (False, True):
                out[f"gn/{name}/{ACT_NAMES[a]}/{'inplace' if inplace else 'out'}"] = sha(gn_run(name, a, inplace, dev))
    for c in CONV_CASES:
        rn = ConvRunner(c)
        want = conv_expected_kernel(c)
        for a in ACTS:
            for cb in conv_combos(c):
                y, names = rn.run(a, cb)
                assert names == [want], (c["id"], names, want)
                out[conv_id(c, a, cb)] = sha(y)
    x = ew_inputs().to(DEV)
    for op in EW_DEFAULT_OPS:
        for a in ACTS:
            out[f"ew/op{op}/{ACT_NAMES[a]}"] = sha(ew_run(op, a, x))
    assert list(out) == all_ids()
    return out


def write_golden(hashes, compiler, commit):
    """commit: the commit whose build produced the hashes (the parent of the change under test)."""
    doc = {"header": {"what": "SHA-256 of the output bytes of every case of tests/act_paths_cases.py",
                      "recorded_on_commit": commit,
                      "recorded_by": "tools/record_act_golden.py on the build before the activation switch was hoisted (csrc/common.h dcvic_act_c)",
                      "note": "the hashes pin bits produced by this ROCm's compiler and its expf / erff / tanhf; a new compiler may "
                              "legitimately move them -- re-record on the parent of the change under test, never on the change itself",
                      "compiler": compiler, "device": "AMD Instinct MI355X (gfx950)"},
           "hashes": hashes}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=False)
        f.write("\n")
