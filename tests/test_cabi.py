"""The C-ABI library loads and exports every symbol include/dcvic.h declares (no compute calls: CPU box)."""
import os
import re

from dc_vic_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "dcvic.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dcvic_[a-zA-Z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 28
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/dcvic.h but not exported"
    assert sorted(_lib.SYMBOLS) == names


def declared_prototypes():
    """{name: (restype, [argtypes])} of every function include/dcvic.h declares, in ctypes terms: the mapping the binding uses
    (every pointer parameter a c_void_p, a const char* return a c_char_p, any other pointer return an opaque c_void_p)."""
    import ctypes as C
    scalars = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
    txt = open(os.path.join(ROOT, "include", "dcvic.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^(\w[\w \t]*?\**)\s*\b(dcvic_\w+)\s*\(([^()]*)\)\s*;", txt, flags=re.M):
        ret = " ".join(ret.split())
        if ret == "const char*":
            restype = C.c_char_p
        elif "*" in ret:
            restype = C.c_void_p
        else:
            restype = None if ret == "void" else scalars[ret]
        argtypes = []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            if "*" in prm:
                argtypes.append(C.c_void_p)
                continue
            words = prm.split()                      # a scalar type, then an optional parameter name
            ty = " ".join(words)
            argtypes.append(scalars[ty] if ty in scalars else scalars[" ".join(words[:-1])])
        assert name not in protos, f"{name} declared twice"
        protos[name] = (restype, argtypes)
    return protos


def signature_mismatches(table, protos):
    """Every disagreement between a "return:parameters" table (_lib.SIGNATURES) and the header's prototypes, as messages."""
    bad = [f"{n}: declared in include/dcvic.h but absent from the table" for n in protos if n not in table]
    bad += [f"{n}: in the table but not declared in include/dcvic.h" for n in table if n not in protos]
    for n in table:
        if n in protos:
            ret, params = table[n].split(":")
            have = (_lib._CTYPE[ret], [_lib._CTYPE[c] for c in params])
            if have != protos[n]:
                bad.append(f"{n}: the table says {have}, the header {protos[n]}")
    return bad


def test_signature_table_matches_header_prototypes():
    """_lib.SIGNATURES states every prototype of include/dcvic.h type for type, and the loaded library's functions carry exactly those
    restype / argtypes.  The comparison itself is shown to catch a long long declared as int, a missing parameter and a function
    missing from the table."""
    import ctypes as C
    protos = declared_prototypes()
    assert len(protos) == 89 and sorted(protos) == declared_symbols()
    # the parser, on prototypes read by eye: optional parameter names, every scalar type, each kind of return
    assert protos["dcvic_tables_destroy_host"] == (None, [C.c_void_p])
    assert protos["dcvic_last_error"] == (C.c_char_p, [])
    assert protos["dcvic_conv_packed_bytes"] == (C.c_size_t, [C.c_void_p])
    assert protos["dcvic_rans_decoder_create_host"] == (C.c_void_p, [C.c_void_p, C.c_longlong])
    assert protos["dcvic_pair_moments_workspace_doubles"] == (C.c_longlong, [C.c_longlong, C.c_longlong])
    assert protos["dcvic_reduce_loss_f32"] == (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_double,
                                                         C.c_void_p, C.c_void_p, C.c_void_p])
    assert protos["dcvic_clip_scale_f32"] == (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p])

    assert signature_mismatches(_lib.SIGNATURES, protos) == []
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name

    def broken(name, sig):
        t = dict(_lib.SIGNATURES)
        if sig is None:
            del t[name]
        else:
            t[name] = sig
        return signature_mismatches(t, protos)
    assert _lib.SIGNATURES["dcvic_neglog2_sum_f32"] == "i:pqppiqp"
    for sig in ("i:pippiqp", "i:pqppiip",      # a long long declared as int
                "i:pqppiq", "i:qppiqp",         # a parameter missing
                "i:pqppiqpp", "q:pqppiqp", None):
        bad = broken("dcvic_neglog2_sum_f32", sig)
        assert len(bad) == 1 and bad[0].startswith("dcvic_neglog2_sum_f32:"), (sig, bad)


def test_error_reporting_without_gpu():
    L = _lib.lib()
    assert L.dcvic_version() >= 100
    # argument validation happens before any HIP call
    rc = L.dcvic_pmf_to_quantized_cdf_host(None, 0, None)
    assert rc == -1 and b"pmf_to_quantized_cdf" in L.dcvic_last_error()
    d = _lib.ConvDesc()
    import ctypes as C
    assert L.dcvic_conv_desc_init(C.byref(d), 8, 8, 7, 7, 1, 0, 0, 0) == -1     # 49 taps > 25
    assert L.dcvic_conv_desc_init(C.byref(d), 128, 128, 3, 3, 1, 1, 1, 0) == 0
    assert d.T == 9 and d.tap_dy[0] == -1 and d.tap_dx[8] == 1
    assert L.dcvic_conv_packed_bytes(C.byref(d)) == 128 * 128 * 9 * 4
    assert L.dcvic_convT_phase_desc(C.byref(d), 192, 192, 5, 0, 0) == 0 and d.T == 9
    assert L.dcvic_convT_phase_desc(C.byref(d), 192, 192, 5, 1, 1) == 0 and d.T == 4
    assert L.dcvic_convT_phase_desc(C.byref(d), 192, 192, 5, 0, 1) == 0 and d.T == 6


def test_wino_packed_bytes_host_formula():
    """dcvic_wino_packed_bytes is a host-side size query (no GPU): one 32 KiB slab (16 positions x 8 channels x 64 output
    channels, fp32) per (64-channel tile, 8-channel chunk), both rounded up."""
    from dc_vic_amd import _lib
    L = _lib.lib()
    for cin, cout in ((128, 128), (704, 512), (8, 64), (20, 96), (256, 3)):
        assert L.dcvic_wino_packed_bytes(cin, cout) == ((cout + 63) // 64) * ((cin + 7) // 8) * 16 * 8 * 64 * 4
    assert L.dcvic_wino_packed_bytes(0, 64) == 0
    # F(4x4, 3x3): one 72 KiB slab (2 k-steps x 36 positions x 4 channels x 64 output channels) per (64-channel tile, 8-channel chunk)
    for cin, cout in ((256, 256), (704, 512), (8, 64), (128, 200)):
        assert L.dcvic_wino44_packed_bytes(cin, cout) == ((cout + 63) // 64) * ((cin + 7) // 8) * 2 * 36 * 4 * 64 * 4
    assert L.dcvic_wino44_packed_bytes(64, 0) == 0


# Runs in a child process with every GPU hidden (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES set before the library loads), and only
# after the child has confirmed that HIP sees no device.  The buffers are dummy non-null addresses: the checks must reject the
# arguments before any launch, and if a check ever stopped doing so the launch would fail for want of a device instead of touching
# memory that does not exist.
_NO_GPU_PRELUDE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from dc_vic_amd import _lib
L = _lib.lib()
with open("/proc/self/maps") as f:                # the HIP runtime the library is bound to
    hip = C.CDLL(next(l.split()[-1] for l in f if "libamdhip64" in l))
n = C.c_int(0)
if hip.hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0:
    sys.exit(3)                                   # a device is still visible: run nothing
P = C.c_void_p(64)
LL = C.c_longlong

def err(rc, *words):
    assert rc == -1, rc
    msg = L.dcvic_last_error().decode()
    for w in words:
        assert w in msg, msg
"""


def _run_without_gpu(script: str) -> None:
    """Runs _NO_GPU_PRELUDE + script in a child process with every GPU hidden; the script prints CHECKS_OK at its end."""
    import subprocess
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_GPU_PRELUDE + script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 3, "HIP still sees a device with every device hidden: the checks were not run"
    assert r.returncode == 0 and "CHECKS_OK" in r.stdout, r.stdout + r.stderr


_ARG_CHECKS = r"""
# copy_planes(dst, dst_bs, dstH, dstW, src, src_bs, srcH, srcW, N, C, copyH, copyW, reflect, stream): src 6x5, dst 12x10
cp = lambda copyH, copyW, reflect: L.dcvic_copy_planes_f32(P, LL(3 * 120), 12, 10, P, LL(3 * 30), 6, 5, 2, 3, copyH, copyW, reflect, None)
err(cp(12, 5, 1), "copy_planes", "reflect")        # a reflection by H (torch 'reflect' needs pad < H)
err(cp(6, 10, 1), "copy_planes", "reflect")        # ... by W
err(cp(7, 5, 0), "copy_planes", "exceeds source")  # crop larger than its source
err(cp(6, 6, 0), "copy_planes", "exceeds source")
err(cp(13, 5, 1), "copy_planes", "exceeds destination")
# copy_window: a row stride narrower than the window
err(L.dcvic_copy_window_f32(P, LL(600), LL(60), LL(5), P, LL(600), LL(60), LL(10), 2, 3, 4, 6, None), "copy_window")
# crop_clamp: crop larger than the image
err(L.dcvic_crop_clamp_f32(P, LL(3 * 30), 6, 5, P, None, 2, 3, 6, 6, None), "crop_clamp")

# gaussian_rate(y, y_bs, sym_in, mu, sigma, ms_bs, table, n_scales, y_hat, yh_bs, sym, idx, si_bs, lik, bits, ws, N, C, HW, stream)
def gr(N, ms_bs=LL(4), si_bs=LL(4), bits=P, ws=P, y=P, sym_in=None):
    return L.dcvic_gaussian_rate_f32(y, LL(4), sym_in, P, P, ms_bs, P, 64, P, LL(4), None, None, si_bs, None, bits, ws, N, 1, 4, None)
err(gr(1025), "gaussian_rate", "1024")                        # bits_out for more than 1024 images
err(gr(2, ms_bs=LL(3)), "gaussian_rate", "batch stride")      # a batch stride below C*HW
err(gr(2, si_bs=LL(2)), "gaussian_rate", "batch stride")
err(gr(2, ws=None), "gaussian_rate", "workspace")             # bits_out without the partial-sum workspace
err(gr(2, y=None), "gaussian_rate", "exactly one")            # neither y nor sym_in
err(gr(2, sym_in=P), "gaussian_rate", "exactly one")          # both
# neglog2_sum(x, x_bs, bits, ws, N, CHW, stream)
err(L.dcvic_neglog2_sum_f32(P, LL(10), P, P, 1025, LL(10), None), "neglog2_sum")
err(L.dcvic_neglog2_sum_f32(P, LL(9), P, P, 2, LL(10), None), "neglog2_sum")
assert L.dcvic_rate_blocks(LL(1)) == 1 and L.dcvic_rate_blocks(LL(2048)) == 1 and L.dcvic_rate_blocks(LL(2049)) == 2
assert L.dcvic_rate_blocks(LL(64 * 2048)) == 64 and L.dcvic_rate_blocks(LL(10 ** 9)) == 64
print("CHECKS_OK")
"""


def test_rate_and_copy_argument_checks_without_gpu():
    """The rate and copy entry points reject bad arguments in their host-side checks, before any launch (see _ARG_CHECKS)."""
    _run_without_gpu(_ARG_CHECKS)



# Every case breaks one rule of one training-step entry point (csrc/train.hip) and keeps the others valid.  A divisor of zero
# must be rejected before the host divides by it (a SIGFPE would end the child); a zero size must not reach a launch.
_TRAIN_ARG_CHECKS = r"""
F = C.c_float
# conv_wgrad(G, g_bs, M, Hg, Wg, X, x_bs, Cx, Hx, Wx, N, KH, KW, stride, pt, pl, dW, accumulate, workspace, stream); baseline:
# N = 2, 16 -> 8 channels, 3x3 / stride 1 / pad 1 on 8 x 8 maps
def wg(M=8, Hg=8, Wg=8, Cx=16, Hx=8, Wx=8, N=2, KH=3, KW=3, stride=1):
    return L.dcvic_conv_wgrad_f32(P, LL(M * Hg * Wg), M, Hg, Wg, P, LL(Cx * Hx * Wx), Cx, Hx, Wx, N, KH, KW, stride, 1, 1, P, 0, P, None)
for kw in (dict(N=0), dict(M=0), dict(Cx=0), dict(Hg=0), dict(Wg=0), dict(Hx=0), dict(Wx=0)):
    err(wg(**kw), "conv_wgrad", "empty map")
for kw in (dict(KW=0), dict(KW=6), dict(KH=0), dict(KH=6), dict(stride=0), dict(stride=5)):
    err(wg(**kw), "conv_wgrad", "unsupported")
slabs = C.c_int(-1)
for args in ((0, 8, 16, 3, 3, 8), (2, 0, 16, 3, 3, 8), (2, 8, 0, 3, 3, 8), (2, 8, 16, 0, 3, 8), (2, 8, 16, 3, 0, 8), (2, 8, 16, 3, 3, 0)):
    assert L.dcvic_conv_wgrad_workspace_floats(*args, C.byref(slabs)) == 0 and slabs.value == 0, args
assert L.dcvic_conv_wgrad_workspace_floats(2, 8, 16, 3, 3, 8, C.byref(slabs)) == slabs.value * 8 * 16 * 9 and slabs.value >= 2

# chan_reduce(a, a_bs, b, b_bs, out, N, C, HW, stream) / sum_rows(in, out, rows, len, accumulate, stream)
for n, c, hw in ((0, 4, 16), (2, 0, 16), (2, 4, 0)):
    err(L.dcvic_chan_reduce_f32(P, LL(64), None, LL(0), P, n, c, hw, None), "chan_reduce")
err(L.dcvic_sum_rows_f32(P, P, 0, LL(16), 0, None), "sum_rows")
err(L.dcvic_sum_rows_f32(P, P, 2, LL(0), 0, None), "sum_rows")

# ew_bwd(op, d, g, a, b, len, w, act, C, HW, vec_bs, stream)
for op in (-1, 12):
    err(L.dcvic_ew_bwd_f32(op, P, P, P, P, LL(64), F(1), 0, 4, 16, LL(0), None), "ew_bwd")
err(L.dcvic_ew_bwd_f32(1, P, P, P, P, LL(0), F(1), 0, 4, 16, LL(0), None), "ew_bwd")
err(L.dcvic_ew_bwd_f32(7, P, P, P, P, LL(64), F(1), 0, 0, 16, LL(0), None), "ew_bwd", "op 7")
err(L.dcvic_ew_bwd_f32(7, P, P, P, P, LL(64), F(1), 0, 4, 0, LL(0), None), "ew_bwd", "op 7")

# groupnorm_bwd(x, x_bs, dy, dy_bs, dx, dx_bs, gamma, beta, dgamma_part, dbeta_part, N, C, HW, groups, eps, act, stream)
def gnb(N=2, Cc=64, HW=16, groups=32, act=3):
    bs = LL(Cc * HW)
    return L.dcvic_groupnorm_bwd_f32(P, bs, P, bs, P, bs, P, P, P, P, N, Cc, HW, groups, F(1e-6), act, None)
for kw in (dict(groups=0), dict(N=0), dict(Cc=0), dict(HW=0)):
    err(gnb(**kw), "groupnorm_bwd")
err(gnb(groups=7), "groupnorm_bwd", "groups=7")                       # C % groups
err(gnb(Cc=130, groups=2), "groupnorm_bwd", "65 channels per group")  # at most 64
err(gnb(act=1), "groupnorm_bwd", "act=1")                            # only none / swish

# layernorm_c_bwd(x, dy, dx, gamma, part, N, C, HW, eps, stream)
for n, c, hw in ((0, 8, 16), (2, 0, 16), (2, 8, 0), (2, 1025, 16)):
    err(L.dcvic_layernorm_c_bwd_f32(P, P, P, P, P, n, c, hw, F(1e-6), None), "layernorm_c_bwd")
# softmax_c_bwd(P, dP, dS, N, C, Pn, scale, stream)
for n, c, pn in ((0, 4, 16), (65536, 4, 16), (2, 0, 16), (2, 4, 0)):
    err(L.dcvic_softmax_c_bwd_f32(P, P, P, n, c, pn, F(1), None), "softmax_c_bwd")

# swin_attn_bwd(qkv, dout, dqkv, table, dtable, dS_ws, N, C, H, W, heads, ws, shift, accumulate, stream)
def swb(N=1, Cc=32, H=16, W=16, heads=2, ws=8, shift=0):
    return L.dcvic_swin_attn_bwd_f32(P, P, P, P, P, P, N, Cc, H, W, heads, ws, shift, 0, None)
for kw in (dict(heads=0), dict(N=0), dict(Cc=0), dict(H=0), dict(W=0)):
    err(swb(**kw), "swin_attn_bwd")
err(swb(ws=4), "swin_attn_bwd", "ws=4")
err(swb(heads=1), "swin_attn_bwd", "heads=1")          # head dim 32 > 16
err(swb(heads=3), "swin_attn_bwd", "heads=3")          # C % heads
err(swb(H=12), "swin_attn_bwd", "H=12")                # H % ws
err(swb(shift=8), "swin_attn_bwd", "shift=8")
err(swb(shift=-4), "swin_attn_bwd", "shift=-4")

# reduce_loss(kind, a, b, len, target, scale, out, workspace, stream) / cross_entropy(logits, target, nll, dlogits, N, C, HW, w, stream)
D = C.c_double
for kind, b, ln in ((-1, P, 16), (4, P, 16), (0, P, 0), (0, None, 16)):
    err(L.dcvic_reduce_loss_f32(kind, P, b, LL(ln), 0, D(1), P, P, None), "reduce_loss")
for n, c, hw in ((0, 4, 16), (2, 0, 16), (2, 4, 0)):
    err(L.dcvic_cross_entropy_f32(P, P, P, P, n, c, hw, F(1), None), "cross_entropy")

# adam_step(p, g, m, v, len, lr, b1, b2, eps, step, gscale, stream) / clip_scale(sumsq, max_norm, out, stream)
err(L.dcvic_adam_step_f32(P, P, P, P, LL(16), F(1e-3), F(0.9), F(0.999), F(1e-8), 0, None, None), "adam")
err(L.dcvic_adam_step_f32(P, P, P, P, LL(0), F(1e-3), F(0.9), F(0.999), F(1e-8), 1, None, None), "adam")
err(L.dcvic_clip_scale_f32(None, F(1), P, None), "clip_scale")

# resample2(down, in, out, planes, Hlow, Wlow, stream) / s2d(in, out, planes, H, W, r, pad, Ho, Wo, inverse, stream) /
# maxpool3s2(x, y, argmax, dy, dx, planes, H, W, stream) / lpips_tap(f0, f1, w, pix, df1, N, C, HW, gscale, stream)
for pl, h, w in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
    err(L.dcvic_resample2_f32(1, P, P, LL(pl), h, w, None), "resample2")
for a in ((0, 8, 8, 2, 0, 4, 4), (2, 0, 8, 2, 0, 4, 4), (2, 8, 0, 2, 0, 4, 4), (2, 8, 8, 0, 0, 4, 4), (2, 8, 8, 2, -1, 4, 4),
          (2, 8, 8, 2, 0, 0, 4)):
    err(L.dcvic_s2d_f32(P, P, LL(a[0]), *a[1:], 0, None), "s2d")
for pl, h, w in ((0, 8, 8), (2, 2, 8), (2, 8, 2)):
    err(L.dcvic_maxpool3s2_f32(P, P, P, None, None, LL(pl), h, w, None), "maxpool")
for n, c, hw in ((0, 64, 16), (65536, 64, 16), (2, 0, 16), (2, 64, 0)):
    err(L.dcvic_lpips_tap_f32(P, P, P, P, None, n, c, hw, F(1), None), "lpips_tap")
print("CHECKS_OK")
"""


def test_train_argument_checks_without_gpu():
    """The training-step entry points reject zero sizes and divisors, out-of-range kernels / ops / steps and unsupported
    layer shapes in their host-side checks, before any launch and without dividing by zero (see _TRAIN_ARG_CHECKS)."""
    _run_without_gpu(_TRAIN_ARG_CHECKS)

# Every case breaks exactly one rule of one convolution entry point and keeps every other argument valid, so the order in which an
# entry point runs its checks does not matter.  Baseline layer: N = 2, one 16-channel 8 x 8 source, 16 output channels (3 for thin).
_CONV_ARG_CHECKS = r"""
N, CIN, H, W = 2, 16, 8, 8

def make_io(cout=16, up=False, srcs=(CIN,), h=H, w=W):
    io = _lib.ConvIO()
    io.N, io.H, io.W = N, h, w
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    io.Hout, io.Wout, io.Hfull, io.Wfull = ho, wo, ho, wo
    io.osy = io.osx = 1
    io.n_src = len(srcs)
    for i, c in enumerate(srcs):
        io.src[i].ptr = 64; io.src[i].C = c; io.src[i].batch_stride = c * h * w
    io.out = 64; io.out_batch_stride = cout * ho * wo
    io.act = 0
    return io

def variant(io, **kw):
    io = type(io).from_buffer_copy(io)
    for k, v in kw.items():
        if k.startswith("src0_"):
            setattr(io.src[0], k[5:], v)
        else:
            setattr(io, k, v)
    return io

def with_res(io, cout, **kw):
    return variant(io, **{"res": 64, "res_batch_stride": cout * io.Hfull * io.Wfull, **kw})

d = _lib.ConvDesc()
assert L.dcvic_conv_desc_init(C.byref(d), CIN, 16, 3, 3, 1, 1, 1, 0) == 0
def conv2d(io, packed=P, desc=d):
    return L.dcvic_conv2d_f32(C.byref(desc), packed, None if io is None else C.byref(io), None)
def wino(io, packed=P, cin=CIN):
    return L.dcvic_conv3x3_wino_f32(cin, 16, packed, None if io is None else C.byref(io), None)
def wino_ups(io, packed=P, cin=CIN):
    return L.dcvic_conv3x3_wino_ups_f32(cin, 16, packed, None if io is None else C.byref(io), None)
def wino44(io, packed=P, cin=CIN):
    return L.dcvic_conv3x3_wino44_f32(cin, 16, packed, None if io is None else C.byref(io), None)
def wino44_stats(io, packed=P, cin=CIN, part=P):
    return L.dcvic_conv3x3_wino44_stats_f32(cin, 16, packed, None if io is None else C.byref(io), part, None)
def bf16(io, packed=P, cin=CIN, up=0):
    return L.dcvic_conv3x3_bf16_f32(cin, 16, up, packed, None if io is None else C.byref(io), None)
def thin(io, packed=P, cin=CIN, cout=3):
    return L.dcvic_conv3x3_thin_f32(packed, cin, cout, None if io is None else C.byref(io), None)

# (entry point, error prefixes its messages may start with, the call, its output channels, whether it maps H x W to 2H x 2W)
ENTRIES = [
    ("conv2d", ("conv2d",), conv2d, 16, False),
    ("wino", ("conv3x3_wino",), wino, 16, False),
    ("wino_ups", ("conv3x3_wino_ups",), wino_ups, 16, True),
    ("wino44", ("conv3x3_wino44",), wino44, 16, False),
    ("wino44_stats", ("conv3x3_wino44", "conv3x3_wino44_stats"), wino44_stats, 16, False),
    ("bf16", ("conv3x3_bf16",), bf16, 16, False),
    ("thin", ("conv3x3_thin",), thin, 3, False),
]
n_cases = 0

def rejects(prefixes, rc, what):
    global n_cases
    assert rc == -1, (what, rc)
    msg = L.dcvic_last_error().decode()
    assert msg.split(":")[0] in prefixes, (what, msg)
    n_cases += 1

for name, prefixes, call, cout, up in ENTRIES:
    io = make_io(cout, up)
    hw = io.Hfull * io.Wfull
    def rej(rc, what):
        rejects(prefixes, rc, f"{name}: {what}")
    rej(call(None), "null io")
    rej(call(variant(io, out=None)), "null out")
    rej(call(io, packed=None), "null packed weights")
    rej(call(variant(io, n_src=0)), "n_src 0")
    rej(call(variant(io, n_src=4)), "n_src 4")
    rej(call(variant(io, src0_C=8)), "channel sum below Cin")
    rej(call(make_io(cout, up, srcs=(8, 16))), "channel sum above Cin")
    rej(call(variant(io, src0_batch_stride=CIN * H * W - 4)), "source batch stride")
    rej(call(variant(io, out_batch_stride=cout * hw - 4)), "output batch stride")
    rej(call(with_res(io, cout, res_batch_stride=cout * hw - 4)), "residual batch stride")

# Winograd x3 and bf16: 8-channel sources
rejects(("conv3x3_wino",), wino(make_io(srcs=(12,)), cin=12), "wino: 12 channels")
rejects(("conv3x3_wino_ups",), wino_ups(make_io(up=True, srcs=(12,)), cin=12), "wino_ups: 12 channels")
rejects(("conv3x3_wino44",), wino44(make_io(srcs=(12,)), cin=12), "wino44: 12 channels")
rejects(("conv3x3_wino44", "conv3x3_wino44_stats"), wino44_stats(make_io(srcs=(12,)), cin=12), "wino44_stats: 12 channels")
rejects(("conv3x3_bf16",), bf16(make_io(srcs=(12,)), cin=12), "bf16: 12 channels")

# Winograd x3: 16-byte views, W % 4, no affine / init, geometry
for name, prefixes, call, cout, up in ENTRIES[1:5]:
    io = make_io(16, up)
    hw = io.Hfull * io.Wfull
    def rej(rc, what):
        rejects(prefixes, rc, f"{name}: {what}")
    rej(call(variant(io, src0_ptr=68)), "misaligned source")
    rej(call(variant(io, out=68)), "misaligned output")
    rej(call(with_res(io, 16, res=68)), "misaligned residual")
    rej(call(variant(io, src0_batch_stride=CIN * H * W + 2)), "source batch stride % 4")
    rej(call(variant(io, out_batch_stride=16 * hw + 2)), "output batch stride % 4")
    rej(call(with_res(io, 16, res_batch_stride=16 * hw + 2)), "residual batch stride % 4")
    rej(call(make_io(16, up, w=6)), "W % 4")
    rej(call(variant(io, aff_scale=64, aff_shift=64)), "affine")
    rej(call(variant(io, aff_scale=64)), "affine scale only")
    rej(call(variant(io, init=64, init_batch_stride=16 * hw)), "init")
    other = make_io(16, not up)
    rej(call(variant(other, out_batch_stride=16 * 4 * H * W)), "output geometry")
    rej(call(variant(io, Hout=io.Hout - 1)), "Hout")
    rej(call(variant(io, Wfull=io.Wfull + 4, out_batch_stride=16 * io.Hfull * (io.Wfull + 4))), "Wfull")
    rej(call(variant(io, osy=2)), "scatter")
    rej(call(variant(io, oox=1)), "offset")

# wino44: activation set, statistics buffer
io = make_io()
rejects(("conv3x3_wino44",), wino44(variant(io, act=3)), "wino44: ACT_SWISH")
rejects(("conv3x3_wino44", "conv3x3_wino44_stats"), wino44_stats(variant(io, act=3)), "wino44_stats: ACT_SWISH")
rejects(("conv3x3_wino44", "conv3x3_wino44_stats"), wino44_stats(io, part=None), "wino44_stats: null gn_part")

# bf16: no init, two-sided affine, output H x W (2H x 2W when upsampling)
pb = ("conv3x3_bf16",)
rejects(pb, bf16(variant(io, init=64, init_batch_stride=16 * H * W)), "bf16: init")
rejects(pb, bf16(variant(io, aff_scale=64)), "bf16: affine scale only")
rejects(pb, bf16(variant(io, aff_shift=64)), "bf16: affine shift only")
rejects(pb, bf16(variant(io, Hout=12, Hfull=12, out_batch_stride=16 * 12 * W)), "bf16: output 12 x 8")
rejects(pb, bf16(variant(make_io(up=True), Wout=W, Wfull=W, out_batch_stride=16 * 2 * H * W)), "bf16: output 16 x 8")
rejects(pb, bf16(io, up=1), "bf16: upsample onto an H x W output")
rejects(pb, bf16(make_io(up=True), up=0), "bf16: 2H x 2W output without upsample")
rejects(pb, bf16(variant(io, osx=2)), "bf16: scatter")

# thin: one source, a thin layer, no affine / init
pt = ("conv3x3_thin",)
io = make_io(3)
rejects(pt, thin(make_io(3, srcs=(8, 8))), "thin: two sources")
rejects(pt, thin(make_io(16), cout=16), "thin: 16 -> 16")
rejects(pt, thin(make_io(3, srcs=(12,)), cin=12), "thin: 12 -> 3")
rejects(pt, thin(variant(io, aff_scale=64, aff_shift=64)), "thin: affine")
rejects(pt, thin(variant(io, init=64, init_batch_stride=3 * H * W)), "thin: init")
rejects(pt, thin(variant(io, Wout=W - 1)), "thin: geometry")

# conv2d: scatter inside Hfull x Wfull, cfg 0..3, two-sided affine, planes below 2^30
p2 = ("conv2d",)
io = make_io()
rejects(p2, conv2d(variant(io, ooy=1)), "conv2d: scatter past Hfull")
rejects(p2, conv2d(variant(io, osx=2, Wout=5)), "conv2d: scatter past Wfull")
rejects(p2, conv2d(variant(io, init=64, init_batch_stride=16 * H * W - 4)), "conv2d: init batch stride")
for cfg in (-1, 4):
    dc = _lib.ConvDesc.from_buffer_copy(d); dc.cfg = cfg
    rejects(p2, conv2d(io, desc=dc), f"conv2d: cfg {cfg}")
rejects(p2, conv2d(variant(io, aff_scale=64)), "conv2d: affine scale only")
rejects(p2, conv2d(variant(io, aff_shift=64)), "conv2d: affine shift only")
big = make_io(h=1 << 15, w=1 << 15)
rejects(p2, conv2d(big), "conv2d: input plane 2^30")
rejects(p2, conv2d(variant(io, Hfull=1 << 15, Wfull=1 << 15, out_batch_stride=16 << 30)), "conv2d: output plane 2^30")
assert n_cases == 7 * 10 + 5 + 4 * 15 + 3 + 8 + 6 + 9, n_cases
print("CHECKS_OK")
"""


def test_conv_argument_checks_without_gpu():
    """The seven convolution entry points reject what their contracts exclude, before any launch (see _CONV_ARG_CHECKS)."""
    _run_without_gpu(_CONV_ARG_CHECKS)


def test_copy_window_shape_check_without_gpu():
    """ops.copy_window rejects unequal shapes before it touches the library."""
    import pytest
    import torch
    from dc_vic_amd import ops
    with pytest.raises(ValueError, match="copy_window"):
        ops.copy_window(torch.zeros(2, 3, 6, 4), torch.zeros(2, 3, 6, 5))
    with pytest.raises(ValueError, match="copy_window"):
        ops.copy_window(torch.zeros(2, 3, 6, 5), torch.zeros(2, 3, 5, 6).transpose(2, 3))
