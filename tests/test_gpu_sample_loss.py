"""Stage 1-2 training on a real MI355X: the two code-loss kernels with one weight per image (csrc/sample_loss.hip,
include/dcvic_sample_loss.h) against torch fp64 autograd of sum_n w[n] * S[n], their bits (against dcvic_focal_ce_f32, across batch
sizes, across runs, over poisoned buffers), a target outside the classes, the reference's own losses carried through
apply_loss_weight (tests/golden/sample_loss.npz) and the two tape ops.  Bounds: the floors test_gpu_focal.py holds the focal kernel
to, 1e-6 relative for values and 1e-5 of the tensor's max for gradients."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
VALUE_TOL, GRAD_TOL = 1e-6, 1e-5
WEIGHTS = (0.7, 0.0, 2.5)
CHANNELS = (2, 5, 256, 257, 272, 273, 300)          # the register path (C <= 272), its edge, the streaming path
POSITIONS = (1, 63, 64, 65, 1024)                   # around the 64-position workgroup, and the trainer's 32 x 32
GAMMAS = (0.0, 1.0, 2.0)
SQ_SIZES = (1, 252, 256, 4096 + 3, 64 * 2048 + 5)   # the last: more than 64 workgroups of 2048 elements per image, the grid stride


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def relerr(a, b):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def focal_inputs(N, Cc, HW, seed=0):
    """Logits [N, C, HW, 1] * 2 and targets that include 0 and C - 1; with more than one position, the middle one of the last image is
    made confidently right (target logit + 40: p_t -> 1)."""
    lg = rnd(N, Cc, HW, 1, seed=500 + Cc + HW + seed) * 2
    idx = torch.randint(0, Cc, (N, HW, 1), generator=torch.Generator().manual_seed(501 + seed))
    idx.view(-1)[0], idx.view(-1)[-1] = 0, Cc - 1
    if HW > 1:
        lg[N - 1, idx[N - 1, HW // 2, 0], HW // 2, 0] += 40.0
    return lg.contiguous(), idx


def focal_fp64(lg, idx, w, gamma):
    """(sum_n w[n] S[n], its gradient, S) in torch fp64 on the CPU, f as FocalCrossEntropyLoss.forward forms it."""
    x = lg.double().requires_grad_(True)
    ce = F.cross_entropy(x, idx, reduction="none")
    pt = F.softmax(x, dim=1).gather(1, idx.unsqueeze(1)).squeeze(1)
    S = (((1 - pt) ** gamma) * ce).reshape(x.shape[0], -1).sum(dim=1)
    loss = (torch.as_tensor(w, dtype=torch.float64) * S).sum()
    loss.backward()
    return loss.detach().reshape(1), x.grad, S.detach()


def wvec(values):
    return torch.tensor(values, dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------- focal, against fp64
@pytest.mark.parametrize("Cc", CHANNELS)
def test_focal_ce_sample_vs_fp64(Cc):
    """Every HW and gamma at this C; prints each measured error before it asserts."""
    from dc_vic_amd.train import kernels as K
    N, w = 3, wvec(WEIGHTS)
    for HW in POSITIONS:
        lg, idx = focal_inputs(N, Cc, HW)
        ld, td = lg.to(DEV), idx.to(DEV)
        for gamma in GAMMAS:
            ref_l, ref_g, ref_S = focal_fp64(lg, idx, w.cpu().double(), gamma)
            loss, dl, per = K.focal_ce_sample(ld, td, w, gamma, want_grad=True, want_per_sample=True)
            ev, eg, es = relerr(loss, ref_l), relerr(dl, ref_g), float(((per.cpu().double() - ref_S).abs() / ref_S.abs()).max())
            print(f"[focal_ce_sample] C {Cc} HW {HW} gamma {gamma:g}: value {float(loss):.9e} err {ev:.3e}, gradient err {eg:.3e}, per-sample err {es:.3e}")
            assert torch.isfinite(loss).all() and torch.isfinite(dl).all() and torch.isfinite(per).all()
            assert ev <= VALUE_TOL and eg <= GRAD_TOL and es <= VALUE_TOL, (Cc, HW, gamma, ev, eg, es)
            assert not dl[1].any(), "a zero weight gives an exactly zero gradient plane"
            assert dl[0].any() and dl[2].any()
            # value only: the same bits, and no gradient buffer
            l2, d2, p2 = K.focal_ce_sample(ld, td, w, gamma, want_grad=False)
            assert d2 is None and p2 is None and torch.equal(l2, loss)


@pytest.mark.parametrize("Cc,HW", [(256, 1024), (5, 65), (300, 63)], ids=["trainer", "ragged", "streaming"])
def test_focal_ce_sample_at_one_weight_is_focal_ce(Cc, HW):
    """With every w[n] = s the gradient has the bits of dcvic_focal_ce_f32 at scale s (one kernel core), for s = 1 and for the
    trainer's 0.05 / (N * HW); the values agree within 1e-6 (two orders of the same fp64 partial sums)."""
    from dc_vic_amd.train import kernels as K
    N = 3
    lg, idx = focal_inputs(N, Cc, HW, seed=1)
    ld, td = lg.to(DEV), idx.to(DEV)
    for gamma in GAMMAS:
        for s in (1.0, 0.05 / (N * HW)):
            fl, fg = K.focal_ce(ld, td, gamma, s, want_grad=True)
            sl, sg, _ = K.focal_ce_sample(ld, td, torch.full((N,), s, dtype=torch.float32, device=DEV), gamma, want_grad=True)
            assert torch.equal(sg, fg), (Cc, HW, gamma, s)
            assert relerr(sl, fl) <= VALUE_TOL, (Cc, HW, gamma, s, float(sl), float(fl))


# ---------------------------------------------------------------------------------------------------- squared error, against fp64
def sq_inputs(N, M, seed=0):
    """a as a slice [N, M] of a wider [N, M + 7] buffer (batch stride M + 7, image start off 16-byte alignment), b dense."""
    full = rnd(N, M + 7, seed=520 + seed)
    return full, full[:, 3:3 + M], rnd(N, M, seed=521 + seed)


def sq_fp64(a, b, w):
    x = a.double().clone().requires_grad_(True)
    S = ((x - b.double()) ** 2).sum(dim=1)
    loss = (torch.as_tensor(w, dtype=torch.float64) * S).sum()
    loss.backward()
    return loss.detach().reshape(1), x.grad, S.detach()


@pytest.mark.parametrize("M", SQ_SIZES)
def test_sq_err_sample_vs_fp64(M):
    from dc_vic_amd.train import kernels as K
    N, w = 3, wvec(WEIGHTS)
    full, a, b = sq_inputs(N, M)
    ref_l, ref_g, ref_S = sq_fp64(a, b, w.cpu().double())
    fd = full.to(DEV)
    ad, bd = fd[:, 3:3 + M], b.to(DEV)
    assert ad.stride(0) == M + 7 and not (ad.is_contiguous() and M > 1)
    loss, da, per = K.sq_err_sample(ad, bd, w, want_grad=True, want_per_sample=True)
    ev, eg, es = relerr(loss, ref_l), relerr(da, ref_g), float(((per.cpu().double() - ref_S).abs() / ref_S.abs()).max())
    print(f"[sq_err_sample] M {M}: value {float(loss):.9e} err {ev:.3e}, gradient err {eg:.3e}, per-sample err {es:.3e}")
    assert ev <= VALUE_TOL and eg <= GRAD_TOL and es <= VALUE_TOL, (M, ev, eg, es)
    assert da.is_contiguous() and tuple(da.shape) == (N, M) and not da[1].any() and da[0].any() and da[2].any()
    assert torch.equal(fd.cpu(), full), "the operand and the values around its slice are read only"
    l2, d2, p2 = K.sq_err_sample(ad, bd, w, want_grad=False)
    assert d2 is None and p2 is None and torch.equal(l2, loss)
    # the same values from a dense copy: the batch stride changes no bit
    l3, d3, p3 = K.sq_err_sample(ad.contiguous(), bd, w, want_grad=True, want_per_sample=True)
    assert torch.equal(l3, loss) and torch.equal(d3, da) and torch.equal(p3, per)


def test_sq_err_sample_on_a_channel_slice_view_vs_reduce_loss():
    """a = full[:, 2:6] of a [3, 8, 5, 7] map, as the trainer's code latents are channel slices; at one weight s the value agrees with
    reduce_loss(SUM_SQ_ERR) + ew(EW_MSE_GRAD), the composition mse_loss launches, within the floors."""
    from dc_vic_amd.train import kernels as K
    full, b = rnd(3, 8, 5, 7, seed=530).to(DEV), rnd(3, 4, 5, 7, seed=531).to(DEV)
    a = full[:, 2:6]
    assert not a.is_contiguous() and a[0].is_contiguous()
    s = 1.0 / a.numel()
    loss, da, per = K.sq_err_sample(a, b, torch.full((3,), s, dtype=torch.float32, device=DEV), want_per_sample=True)
    ac = a.contiguous()
    old_v, old_g = K.reduce_loss(K.SUM_SQ_ERR, ac, b, s), K.ew(K.EW_MSE_GRAD, None, ac, b, w=s)
    ref_l, ref_g, ref_S = sq_fp64(ac.cpu().reshape(3, -1), b.cpu().reshape(3, -1), [s] * 3)
    assert relerr(loss, ref_l) <= VALUE_TOL and relerr(da.reshape(3, -1), ref_g) <= GRAD_TOL and relerr(per, ref_S) <= VALUE_TOL
    assert relerr(loss, old_v.reshape(1)) <= VALUE_TOL and relerr(da, old_g) <= GRAD_TOL
    assert tuple(da.shape) == (3, 4, 5, 7)
    with pytest.raises(ValueError, match="dense within an image"):
        K.sq_err_sample(full[:, :, :, 1:5], full[:, :, :, 1:5].contiguous(), torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match="sample weights"):
        K.sq_err_sample(a, b, torch.ones(2, device=DEV))


# ---------------------------------------------------------------------------------------------------- bits
def test_image_0_does_not_depend_on_the_batch():
    """per_sample[0] and image 0's gradient plane: equal bits at N = 1 and at N = 3, for both kernels and both focal paths."""
    from dc_vic_amd.train import kernels as K
    w = wvec(WEIGHTS)
    for Cc, HW in ((256, 1024), (300, 65)):
        lg, idx = focal_inputs(3, Cc, HW, seed=2)
        ld, td = lg.to(DEV), idx.to(DEV)
        _, g3, p3 = K.focal_ce_sample(ld, td, w, 2.0, want_per_sample=True)
        _, g1, p1 = K.focal_ce_sample(ld[:1].contiguous(), td[:1].contiguous(), w[:1].contiguous(), 2.0, want_per_sample=True)
        assert torch.equal(p1[0], p3[0]) and torch.equal(g1[0], g3[0]), (Cc, HW)
    for M in (4096 + 3, 64 * 2048 + 5):
        full, a, b = sq_inputs(3, M, seed=2)
        ad, bd = full.to(DEV)[:, 3:3 + M], b.to(DEV)
        _, g3, p3 = K.sq_err_sample(ad, bd, w, want_per_sample=True)
        _, g1, p1 = K.sq_err_sample(ad[:1], bd[:1].contiguous(), w[:1].contiguous(), want_per_sample=True)
        assert torch.equal(p1[0], p3[0]) and torch.equal(g1[0], g3[0]), M


def _focal_raw(ld, td, w, gamma, loss, dl, per, ws):
    from dc_vic_amd._lib import check, lib
    from dc_vic_amd.ops import _p, _stream
    N, Cc, H, W = ld.shape
    check(lib().dcvic_focal_ce_sample_f32(_p(ld), _p(td), _p(w), C.c_double(gamma), _p(loss), _p(dl), _p(per), _p(ws), N, Cc, H * W, _stream()), "focal_ce_sample")


def _sq_raw(ad, bd, w, loss, da, per, ws):
    from dc_vic_amd._lib import check, lib
    from dc_vic_amd.ops import _p, _stream
    N, M = ad.shape
    check(lib().dcvic_sq_err_sample_f32(_p(ad), ad.stride(0), _p(bd), _p(w), _p(loss), _p(da), _p(per), _p(ws), N, M, _stream()), "sq_err_sample")


def test_two_runs_give_equal_bits_and_buffer_contents_change_nothing():
    """Two calls return the same bits; then every output and the workspace are pre-filled with NaN through the C ABI: the same bits
    again, and no NaN left in the part of the workspace the call sized."""
    from dc_vic_amd._lib import lib
    from dc_vic_amd.train import kernels as K
    w = wvec(WEIGHTS)
    nan = lambda *shape, dtype=torch.float32: torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    for Cc, HW in ((256, 1024), (300, 65)):
        lg, idx = focal_inputs(3, Cc, HW, seed=3)
        ld, td = lg.to(DEV), idx.to(DEV)
        a, b = K.focal_ce_sample(ld, td, w, 2.0, want_per_sample=True), K.focal_ce_sample(ld, td, w, 2.0, want_per_sample=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        need = int(lib().dcvic_focal_ce_sample_workspace_doubles(3, HW))
        ws, loss, dl, per = nan(need, dtype=torch.float64), nan(1), torch.full_like(ld, float("nan")), nan(3)
        _focal_raw(ld, td, w, 2.0, loss, dl, per, ws)
        assert torch.equal(loss, a[0]) and torch.equal(dl, a[1]) and torch.equal(per, a[2]) and not torch.isnan(ws).any()
    for M in (252, 64 * 2048 + 5):
        full, _, bb = sq_inputs(3, M, seed=3)
        ad, bd = full.to(DEV)[:, 3:3 + M], bb.to(DEV)
        a, b = K.sq_err_sample(ad, bd, w, want_per_sample=True), K.sq_err_sample(ad, bd, w, want_per_sample=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        need = int(lib().dcvic_sq_err_sample_workspace_doubles(3, M))
        ws, loss, da, per = nan(need, dtype=torch.float64), nan(1), nan(3, M), nan(3)
        _sq_raw(ad, bd, w, loss, da, per, ws)
        assert torch.equal(loss, a[0]) and torch.equal(da, a[1]) and torch.equal(per, a[2]) and not torch.isnan(ws).any()


@pytest.mark.parametrize("bad", [-1, None], ids=["-1", "C"])
@pytest.mark.parametrize("Cc", [256, 300], ids=["cached", "streaming"])
def test_bad_target_gives_nan_and_is_never_an_address(bad, Cc):
    """A target of C or -1 at one position of image 1: the loss and per_sample[1] are NaN, the other images' sums and every other
    position's gradient are those of the clean call, and the guard words on both sides of every output keep their bits.  The logits
    are exactly their own size: the index is compared, never added to a pointer."""
    from dc_vic_amd._lib import lib
    from dc_vic_amd.train import kernels as K
    N, HW, G, MARK = 3, 81, 64, 12345.0
    w = wvec((0.7, 1.3, 2.5))
    lg, idx = focal_inputs(N, Cc, HW, seed=4)
    ld = lg.to(DEV)
    clean_l, clean_g, clean_p = K.focal_ce_sample(ld, idx.to(DEV), w, 2.0, want_per_sample=True)
    idx2 = idx.clone()
    idx2[1, 40, 0] = Cc if bad is None else bad
    guarded = lambda n: torch.full((n + 2 * G,), MARK, dtype=torch.float32, device=DEV)
    lb, db, pb = guarded(1), guarded(ld.numel()), guarded(N)
    loss, dl, per = lb[G:G + 1], db[G:G + ld.numel()].view(ld.shape), pb[G:G + N]
    ws = torch.empty(int(lib().dcvic_focal_ce_sample_workspace_doubles(N, HW)), dtype=torch.float64, device=DEV)
    _focal_raw(ld, idx2.to(DEV), w, 2.0, loss, dl, per, ws)
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isfinite(clean_l).all()
    assert torch.isnan(per[1]) and torch.equal(per[0], clean_p[0]) and torch.equal(per[2], clean_p[2])
    keep = torch.ones((N, HW, 1), dtype=torch.bool, device=DEV)
    keep[1, 40, 0] = False
    keep = keep[:, None].expand(N, Cc, HW, 1)
    assert torch.equal(dl[keep], clean_g[keep])
    for buf, n in ((lb, 1), (db, ld.numel()), (pb, N)):
        assert (buf[:G] == MARK).all() and (buf[G + n:] == MARK).all()


# ---------------------------------------------------------------------------------------------------- the reference's own losses
def test_sample_losses_vs_reference_module_fixture():
    """tests/golden/sample_loss.npz (the reference's FocalCrossEntropyLoss and VanillaMSELoss in fp32, carried through
    apply_loss_weight; both beta policies, all three reductions) with w from losses.sample_loss_weights: values and gradients within
    2e-5, the bound test_gpu_focal.py holds the focal kernel to against focal.npz."""
    from dc_vic_amd.train import kernels as K
    from dc_vic_amd.train.losses import sample_loss_weights
    G = np.load(os.path.join(ROOT, "tests", "golden", "sample_loss.npz"))
    ld, td = torch.from_numpy(G["logits"]).to(DEV), torch.from_numpy(G["target"]).to(DEV)
    lat, gt = torch.from_numpy(G["latent"]).to(DEV), torch.from_numpy(G["gt_latent"]).to(DEV)
    beta = torch.from_numpy(G["beta_vq"])
    N = ld.shape[0]
    for policy in G["policies"]:
        bw = (beta + float(G["beta_offset"]) if policy == "linear" else torch.exp(beta)).to(DEV)
        for red in G["reductions"]:
            w = sample_loss_weights(float(G["ce_weight"]), str(red), N, td[0].numel(), bw)
            loss, dl, _ = K.focal_ce_sample(ld, td, w, float(G["gamma"]))
            ev, eg = relerr(loss, np.asarray(G[f"ce_{policy}_{red}"]).reshape(1)), relerr(dl, G[f"ce_grad_{policy}_{red}"])
            w = sample_loss_weights(float(G["mse_weight"]), str(red), N, lat[0].numel(), bw)
            loss, da, _ = K.sq_err_sample(lat, gt, w)
            ev2, eg2 = relerr(loss, np.asarray(G[f"mse_{policy}_{red}"]).reshape(1)), relerr(da, G[f"mse_grad_{policy}_{red}"])
            print(f"[sample losses vs reference modules] {policy} {red}: focal value {ev:.3e} gradient {eg:.3e}; mse value {ev2:.3e} gradient {eg2:.3e}")
            assert max(ev, eg, ev2, eg2) <= 2e-5, (policy, red, ev, eg, ev2, eg2)


# ---------------------------------------------------------------------------------------------------- the tape ops
def test_weighted_tape_ops_return_the_kernel_values_and_accumulate():
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import kernels as K
    w = wvec(WEIGHTS)
    lg, idx = focal_inputs(3, 256, 64, seed=5)
    ld, td = lg.to(DEV), idx.to(DEV).view(3, 8, 8)
    ld = ld.view(3, 256, 8, 8)
    kl, kg, _ = K.focal_ce_sample(ld, td, w, 2.0)
    v = A.Var(ld)
    val = A.focal_cross_entropy_loss_weighted(A.Ctx([]), v, td, w, 2.0)
    assert tuple(val.shape) == (1,) and val.is_cuda and torch.equal(val, kl) and torch.equal(v.grad, kg)
    prior = (rnd(3, 256, 8, 8, seed=540) * 1e-3).to(DEV)
    v2 = A.Var(ld)
    v2.grad = prior.clone()
    assert torch.equal(A.focal_cross_entropy_loss_weighted(A.Ctx([]), v2, td, w, 2.0), kl) and torch.equal(v2.grad, prior + kg)
    c = A.const(ld)
    assert torch.equal(A.focal_cross_entropy_loss_weighted(A.Ctx([]), c, td, w, 2.0), kl) and c.grad is None

    full, b = rnd(3, 8, 8, 8, seed=541).to(DEV), rnd(3, 4, 8, 8, seed=542).to(DEV)
    a = full[:, 4:]
    kl, kg, _ = K.sq_err_sample(a, b, w)
    v = A.Var(a)
    val = A.mse_loss_weighted(A.Ctx([]), v, b, w)
    assert tuple(val.shape) == (1,) and torch.equal(val, kl) and torch.equal(v.grad, kg) and v.grad.is_contiguous()
    prior = (rnd(3, 4, 8, 8, seed=543) * 1e-3).to(DEV)
    v2 = A.Var(a)
    v2.grad = prior.clone()
    assert torch.equal(A.mse_loss_weighted(A.Ctx([]), v2, b, w), kl) and torch.equal(v2.grad, prior + kg)
    c = A.const(a)
    assert torch.equal(A.mse_loss_weighted(A.Ctx([]), c, b, w), kl) and c.grad is None
    # at one weight per image the ops are the unweighted ones within the floors
    s = 0.5 / a.numel()
    u = A.Var(a)
    old = A.mse_loss(A.Ctx([]), u, b, 0.5)
    n = A.Var(a)
    new = A.mse_loss_weighted(A.Ctx([]), n, b, torch.full((3,), s, dtype=torch.float32, device=DEV))
    assert relerr(new, old) <= VALUE_TOL and relerr(n.grad, u.grad) <= GRAD_TOL
