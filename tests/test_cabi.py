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
    import ctypes as C
    from dc_vic_amd import _lib
    L = _lib.lib()
    L.dcvic_wino_packed_bytes.restype = C.c_size_t
    for cin, cout in ((128, 128), (704, 512), (8, 64), (20, 96), (256, 3)):
        assert L.dcvic_wino_packed_bytes(cin, cout) == ((cout + 63) // 64) * ((cin + 7) // 8) * 16 * 8 * 64 * 4
    assert L.dcvic_wino_packed_bytes(0, 64) == 0
    # F(4x4, 3x3): one 72 KiB slab (2 k-steps x 36 positions x 4 channels x 64 output channels) per (64-channel tile, 8-channel chunk)
    L.dcvic_wino44_packed_bytes.restype = C.c_size_t
    for cin, cout in ((256, 256), (704, 512), (8, 64), (128, 200)):
        assert L.dcvic_wino44_packed_bytes(cin, cout) == ((cout + 63) // 64) * ((cin + 7) // 8) * 2 * 36 * 4 * 64 * 4
    assert L.dcvic_wino44_packed_bytes(64, 0) == 0


# Runs in a child process with every GPU hidden (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES set before the library loads), and only
# after the child has confirmed that HIP sees no device.  The buffers are dummy non-null addresses: the checks must reject the
# arguments before any launch, and if a check ever stopped doing so the launch would fail for want of a device instead of touching
# memory that does not exist.
_ARG_CHECKS = r"""
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
print("ARG_CHECKS_OK")
"""


def test_rate_and_copy_argument_checks_without_gpu():
    """The rate and copy entry points reject bad arguments in their host-side checks, before any launch (see _ARG_CHECKS)."""
    import subprocess
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _ARG_CHECKS, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 3, "HIP still sees a device with every device hidden: the checks were not run"
    assert r.returncode == 0 and "ARG_CHECKS_OK" in r.stdout, r.stdout + r.stderr


def test_copy_window_shape_check_without_gpu():
    """ops.copy_window rejects unequal shapes before it touches the library."""
    import pytest
    import torch
    from dc_vic_amd import ops
    with pytest.raises(ValueError, match="copy_window"):
        ops.copy_window(torch.zeros(2, 3, 6, 4), torch.zeros(2, 3, 6, 5))
    with pytest.raises(ValueError, match="copy_window"):
        ops.copy_window(torch.zeros(2, 3, 6, 5), torch.zeros(2, 3, 5, 6).transpose(2, 3))
