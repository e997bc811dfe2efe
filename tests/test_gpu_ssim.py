"""MS-SSIM and PSNR on the MI355X (csrc/ssim.hip, dc_vic_amd.metrics.ms_ssim_psnr) against the fp64 restatement of
tests/test_ssim_host.py (parity with pytorch-msssim unpinned: the package is not in the reference tree)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ssim_host import _pair, ms_ssim_ref, psnr_ref, sse_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# worst |GPU - fp64| over every shape of test_ms_ssim_vs_fp64, N = 3, on one MI355X: 3.3e-8 (at 163x201; 8e-9 to 2.2e-8 elsewhere,
# values near 0.987); the bound is about 10x that
MS_SSIM_TOL = 3e-7


def _gpu(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def test_integer_planes_and_psnr_bit_exact():
    """The truncated planes equal torch's `.int()` bit for bit: values one fp32 ulp either side of k / 127.5 - 1 and random values
    next to them, per-image squared-error sums against an all-0 and an all-255 plane (both sums pin sum t and sum t^2 of each image)."""
    from dc_vic_amd.metrics import msssim_psnr_sse
    k = torch.arange(256, dtype=torch.float64)
    c = (k / 127.5 - 1.0).float()
    vals = torch.stack([c, torch.nextafter(c, torch.full_like(c, -2.0)), torch.nextafter(c, torch.full_like(c, 2.0)),
                        (c + torch.rand(256, generator=torch.Generator().manual_seed(0)) * (1.0 / 127.5)).clamp(-1, 1)], 1)
    x = vals.clamp(-1, 1).reshape(256, 1, 1, 4).repeat(1, 3, 1, 1).contiguous()       # image k: the values around k
    for fill in (-1.0, 1.0):
        y = torch.full_like(x, fill)
        ms, ps, sse = msssim_psnr_sse(*_gpu(x, y))
        assert torch.equal(sse.cpu(), sse_ref(x, y).double())
        assert (ms.cpu() == -1.0).all()
        r = psnr_ref(x, y)
        fin = torch.isfinite(r)
        assert torch.equal(torch.isinf(ps.cpu()), ~fin)
        assert (ps.cpu()[fin] - r[fin]).abs().max() <= 1e-12
    # random images at a validation size: exact integer sums, PSNR to 1e-12
    g = torch.Generator().manual_seed(1)
    x, y = torch.rand((3, 3, 512, 768), generator=g) * 2 - 1, torch.rand((3, 3, 512, 768), generator=g) * 2 - 1
    ms, ps, sse = msssim_psnr_sse(*_gpu(x, y))
    assert torch.equal(sse.cpu(), sse_ref(x, y).double())
    assert (ps.cpu() - psnr_ref(x, y)).abs().max() <= 1e-12


SHAPES = [(512, 768), (768, 512), (161, 161), (163, 201), (333, 257), (1365, 2048)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_ms_ssim_vs_fp64(H, W):
    from dc_vic_amd.metrics import ms_ssim_psnr
    x, y = _pair(3, H, W, seed=H * 7 + W, noise=0.08)
    ref = ms_ssim_ref(x, y)
    assert ((ref > 0.05) & (ref < 0.9999)).all(), ref
    xg, yg = _gpu(x, y)
    ms3, ps3 = ms_ssim_psnr(xg, yg)
    ms1, ps1 = ms_ssim_psnr(xg[1:2].contiguous(), yg[1:2].contiguous())
    err = (ms3.cpu() - ref).abs().max().item()
    assert err <= MS_SSIM_TOL, f"{H}x{W}: max |ms_ssim - fp64| = {err:.3e}"
    assert (ms1.cpu() - ref[1:2]).abs().max().item() <= MS_SSIM_TOL
    assert (ps3.cpu() - psnr_ref(x, y)).abs().max() <= 1e-12


def test_identical_inputs_and_batch_invariance():
    from dc_vic_amd.metrics import ms_ssim_psnr
    x, y = _gpu(*_pair(3, 333, 257, seed=9))
    ms, ps = ms_ssim_psnr(x, x)
    assert torch.equal(ms.cpu(), torch.ones(3, dtype=torch.float64)) and torch.isinf(ps).all()
    ms3, ps3 = ms_ssim_psnr(x, y)
    for k in range(3):
        ms1, ps1 = ms_ssim_psnr(x[k:k + 1].contiguous(), y[k:k + 1].contiguous())
        assert torch.equal(ms1.cpu(), ms3.cpu()[k:k + 1]) and torch.equal(ps1.cpu(), ps3.cpu()[k:k + 1])


def test_arguments_and_small_images():
    from dc_vic_amd import _lib
    from dc_vic_amd.metrics import ms_ssim_psnr
    from dc_vic_amd.ops import _p, _stream
    L = _lib.lib()
    x, y = _gpu(*_pair(1, 161, 200, seed=3))
    with pytest.raises(ValueError):
        ms_ssim_psnr(x, y[:, :, :160].contiguous())
    with pytest.raises(ValueError):
        ms_ssim_psnr(x[:, :2].contiguous(), y[:, :2].contiguous())
    with pytest.raises(ValueError):
        ms_ssim_psnr(x.double(), y.double())
    with pytest.raises(ValueError):
        ms_ssim_psnr(x.transpose(2, 3), y.transpose(2, 3))
    out = torch.empty(3, dtype=torch.float64, device=DEV)
    nb = L.dcvic_msssim_workspace_bytes(1, 3, 161, 200)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

    def call(xx, yy, H, W, ms_ptr, nbytes):
        return L.dcvic_msssim_psnr_f64(_p(xx), _p(yy), 1, 3, H, W, ms_ptr, _p(out[1:2]), _p(out[2:3]), _p(ws), C.c_longlong(nbytes), _stream())

    assert call(x, y, 161, 200, _p(out[0:1]), nb) == 0
    assert call(x, y, 161, 200, _p(out[0:1]), nb - 1) == -1 and b"workspace" in L.dcvic_last_error()
    xs, ys = x[:, :, :160].contiguous(), y[:, :, :160].contiguous()
    assert call(xs, ys, 160, 200, _p(out[0:1]), nb) == -1 and b"min(H, W) > 160" in L.dcvic_last_error()
    assert call(xs, ys, 160, 200, None, nb) == 0                        # PSNR only: any size
    assert L.dcvic_msssim_psnr_f64(None, _p(y), 1, 3, 161, 200, _p(out[0:1]), _p(out[1:2]), _p(out[2:3]), _p(ws), C.c_longlong(nb),
                                   _stream()) == -1 and b"msssim_psnr" in L.dcvic_last_error()
    # the Python path: -1 below the minimum, PSNR still computed
    for H, W in ((160, 200), (200, 160), (16, 16)):
        a, b = _pair(2, H, W, seed=H + W)
        ms, ps = ms_ssim_psnr(*_gpu(a, b))
        assert torch.equal(ms.cpu(), torch.full((2,), -1.0, dtype=torch.float64))
        assert (ps.cpu() - psnr_ref(a, b)).abs().max() <= 1e-12


def test_graph_capture_replays_the_same_bits():
    from dc_vic_amd.metrics import ms_ssim_psnr
    x, y = _gpu(*_pair(2, 512, 768, seed=12))
    ms0, ps0 = ms_ssim_psnr(x, y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ms, ps = ms_ssim_psnr(x, y)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ms, ms0) and torch.equal(ps, ps0)
    x2, y2 = _pair(2, 512, 768, seed=13)
    x.copy_(x2.to(DEV))
    y.copy_(y2.to(DEV))
    g.replay()
    torch.cuda.synchronize()
    ms2, ps2 = ms_ssim_psnr(x, y)
    assert torch.equal(ms, ms2) and torch.equal(ps, ps2) and not torch.equal(ms2, ms0)
    del g
