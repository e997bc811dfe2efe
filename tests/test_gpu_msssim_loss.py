"""dcvic_msssim_loss_f32 / dcvic_abs_err_f32 (csrc/msssim_loss.hip) on a real MI355X against tests/msssim_loss_ref.py, the torch
restatement of the reference's MSSSIMLoss / L1Loss in fp64 with torch autograd's gradient.

Shapes: (1,3,161,161) every pool pads and the last valid map is 1 x 1; (2,3,163,201); (1,3,162,331) ragged last tiles in both
directions (stats tiles 64 x 16, gradient tiles 32 x 16); (3,3,256,256) the trainer's crop.  Regimes: msssim_loss_ref.REGIMES.
Bounds (the README's rule for the rate term): value within max(1e-6 * loss_weight, 4 x the fp32 restatement's own error on the same
inputs) -- the floor is absolute because 1 - V cancels; gradient within max(1e-5 of the fp64 gradient's max, 4 x the fp32
restatement's error).  Every factor of near / far / unclamped is asserted to be at least 1e-3 away from 0 (the relu's kink).

Set DCVIC_MSSSIM_ERRLOG=<file> to have the measured errors appended there."""
import os

import pytest
import torch

import msssim_loss_ref as R
from test_msssim_loss_host import check_refusals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_WEIGHT = 50.0                                          # config/exp1_stage1_2.yaml's distortion weight
SHAPES = [(1, 3, 161, 161), (2, 3, 163, 201), (1, 3, 162, 331), (3, 3, 256, 256)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _log(line):
    print(line)
    path = os.environ.get("DCVIC_MSSSIM_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def run(real, fake, scale, want_grad=True, want_per_plane=True, fill=None):
    """The entry point on device copies of (real, fake) -> (loss, per_plane, dfake) as CPU tensors.  `fill`: a value every output and
    the workspace hold beforehand."""
    from dc_vic_amd import _lib
    L = _lib.lib()
    r, f = real.to(DEV).contiguous(), fake.to(DEV).contiguous()
    N, Cc, H, W = f.shape
    need = int(L.dcvic_msssim_loss_workspace_bytes(N, Cc, H, W))
    assert need > 0 and need % 256 == 0
    mk = (lambda *s, dtype: torch.full(s, fill, dtype=dtype, device=DEV)) if fill is not None else (lambda *s, dtype: torch.empty(s, dtype=dtype, device=DEV))
    ws = mk(need // 8, dtype=torch.float64)
    loss, per = mk(1, dtype=torch.float64), (mk(N, Cc, dtype=torch.float64) if want_per_plane else None)
    df = mk(N, Cc, H, W, dtype=torch.float32) if want_grad else None
    p = lambda t: t.data_ptr() if t is not None else None
    rc = L.dcvic_msssim_loss_f32(p(r), p(f), N, Cc, H, W, float(scale), p(loss), p(per), p(df), p(ws), need, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "msssim_loss")
    torch.cuda.synchronize()
    return loss.cpu(), per.cpu() if per is not None else None, df.cpu() if df is not None else None


@pytest.mark.parametrize("regime", ["near", "far", "unclamped"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_value_and_gradient_against_fp64(shape, regime):
    real, fake = R.pair(shape, regime)
    ref = R.reference(shape, regime, LOSS_WEIGHT)
    assert float(ref["factors"].abs().min()) >= 1e-3 and float(ref["factors"].min()) > 0, ref["factors"]
    N, Cc = shape[:2]
    loss, per, df = run(real, fake, LOSS_WEIGHT / (N * Cc))
    gmax = float(ref["grad64"].abs().max())
    v_err, v_ref = abs(float(loss) - float(ref["loss64"])), abs(float(ref["loss32"]) - float(ref["loss64"]))
    g_err, g_ref = float((df.double() - ref["grad64"]).abs().max()), float((ref["grad32"] - ref["grad64"]).abs().max())
    v_bound, g_bound = max(1e-6 * LOSS_WEIGHT, 4 * v_ref), max(1e-5 * gmax, 4 * g_ref)
    p_err = float((per - R.ms_ssim_planes(real, fake)).abs().max())
    _log(f"[msssim_loss {'x'.join(map(str, shape))} {regime}] loss {float(ref['loss64']):.6e} err {v_err:.3e} (fp32 torch {v_ref:.3e}, bound {v_bound:.3e}, "
         f"err/bound {v_err / v_bound:.3f}); grad max {gmax:.3e} err/max {g_err / gmax:.3e} (fp32 torch {g_ref / gmax:.3e}, err/bound {g_err / g_bound:.3f}); "
         f"per-plane MS-SSIM err {p_err:.3e}; smallest factor {float(ref['factors'].min()):.4f}")
    assert torch.isfinite(df).all()
    assert v_err <= v_bound, (v_err, v_bound)
    assert g_err <= g_bound, (g_err / gmax, g_bound / gmax)
    assert p_err <= 1e-6


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_anticorrelated_and_identical(shape):
    N, Cc = shape[:2]
    scale = LOSS_WEIGHT / (N * Cc)
    real, fake = R.pair(shape, "anticorrelated")
    assert float(R.reference(shape, "anticorrelated", LOSS_WEIGHT)["factors"].min(0).values.max()) < 0        # every plane has a negative factor
    loss, per, df = run(real, fake, scale, fill=float("nan"))
    assert abs(float(loss) - scale * N * Cc) <= 1e-12 * scale * N * Cc
    assert float(per.abs().max()) == 0.0 and float(df.abs().max()) == 0.0
    real, _ = R.pair(shape, "identical")
    loss, per, df = run(real, real, scale)
    near_max = float(R.reference(shape, "near", LOSS_WEIGHT)["grad64"].abs().max())
    _log(f"[msssim_loss {'x'.join(map(str, shape))} identical] loss {float(loss):.3e}, max|dfake| {float(df.abs().max()):.3e} ({float(df.abs().max()) / near_max:.3e} of near's max)")
    assert float(loss) == 0.0 and torch.equal(per, torch.ones_like(per))
    assert float(df.abs().max()) <= 1e-5 * near_max


def test_bits_do_not_depend_on_run_batch_prior_contents_or_gradient():
    shape = (3, 3, 256, 256)
    real, fake = R.pair(shape, "far")
    scale = LOSS_WEIGHT / 9
    a = run(real, fake, scale, fill=0.0)
    b = run(real, fake, scale, fill=float("nan"))           # NaN-filled outputs and workspace
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    fwd = run(real, fake, scale, want_grad=False, want_per_plane=False, fill=float("nan"))
    assert torch.equal(fwd[0], a[0]) and fwd[1] is None and fwd[2] is None
    one = run(real[:1], fake[:1], scale)                     # image 0 alone, the same scale
    assert torch.equal(one[1][0], a[1][0]) and torch.equal(one[2][0], a[2][0])
    assert not torch.equal(a[2][0], a[2][1])


def test_argument_refusals_name_the_entry_point():
    check_refusals()


# ---------------------------------------------------------------------------------------------------- L1
def run_abs(a, b, scale, want_grad=True, fill=None):
    from dc_vic_amd import _lib
    L = _lib.lib()
    ad, bd = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    N, M = ad.shape[0], ad[0].numel()
    need = int(L.dcvic_abs_err_workspace_bytes(N, M))
    mk = (lambda n, dtype: torch.full((n,), fill, dtype=dtype, device=DEV)) if fill is not None else (lambda n, dtype: torch.empty(n, dtype=dtype, device=DEV))
    ws, loss = mk(need // 8, torch.float64), mk(1, torch.float64)
    da = mk(ad.numel(), torch.float32) if want_grad else None
    rc = L.dcvic_abs_err_f32(ad.data_ptr(), bd.data_ptr(), M, N, float(scale), loss.data_ptr(), da.data_ptr() if want_grad else None, ws.data_ptr(), need,
                             torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "abs_err")
    torch.cuda.synchronize()
    return loss.cpu(), da.cpu().view(a.shape) if want_grad else None


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 64, 64), (3, 3, 256, 256)], ids=["1x3x5x7", "2x3x64x64", "3x3x256x256"])
def test_abs_err(shape):
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g) * 2 - 1
    b = a + 0.2 * torch.randn(shape, generator=g)
    ties = torch.rand(shape, generator=g) < 0.1
    ties.view(-1)[:3] = True                                 # planted exact ties
    b[ties] = a[ties]
    scale = LOSS_WEIGHT / a.numel()
    loss, da = run_abs(a, b, scale, fill=float("nan"))
    ref, gref = R.value_and_grad(R.l1_loss, b, a, LOSS_WEIGHT, torch.float64)
    assert abs(float(loss) - float(ref)) <= 1e-6 * float(ref)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    assert torch.equal(da, torch.sign(a - b) * s32) and float(da[ties].abs().max()) == 0.0
    assert set(da.unique().tolist()) == {-s32, 0.0, s32}
    assert float((da.double() - gref).abs().max()) <= 1e-7 * scale
    again, da2 = run_abs(a, b, scale, fill=0.0)
    assert torch.equal(again, loss) and torch.equal(da2, da)
    assert torch.equal(run_abs(a, b, scale, want_grad=False)[0], loss)
    _, one = run_abs(a[:1], b[:1], scale)                    # image 0 alone, the same scale
    assert torch.equal(one[0], da[0])


def test_tape_ops_seed_the_gradient():
    """A.ms_ssim_loss / A.l1_loss: the value and the seeded gradient are the entry points' (weight / (N C) and weight / numel)."""
    from dc_vic_amd.train import autograd as A
    shape = (2, 3, 163, 201)
    real, fake = R.pair(shape, "far")
    ref = R.reference(shape, "far", LOSS_WEIGHT)
    for op, want in ((A.ms_ssim_loss, run(real, fake, LOSS_WEIGHT / 6)), (A.l1_loss, run_abs(fake, real, LOSS_WEIGHT / fake.numel()))):
        v = A.Var(fake.to(DEV))
        val = op(A.Ctx([]), v, real.to(DEV), LOSS_WEIGHT)
        assert torch.equal(val.cpu(), want[0]) and torch.equal(v.grad.cpu(), want[-1])
    assert abs(float(want[0]) - float(R.l1_loss(real, fake, LOSS_WEIGHT))) <= 1e-6 * float(want[0]) and ref is not None
    with pytest.raises(ValueError, match="64 x 64"):
        A.ms_ssim_loss(A.Ctx([]), A.Var(torch.zeros((1, 3, 64, 64), device=DEV)), torch.zeros((1, 3, 64, 64), device=DEV), 1.0)
    with pytest.raises(ValueError, match="RGB"):
        A.ms_ssim_loss(A.Ctx([]), A.Var(torch.zeros((1, 1, 200, 200), device=DEV)), torch.zeros((1, 1, 200, 200), device=DEV), 1.0)
