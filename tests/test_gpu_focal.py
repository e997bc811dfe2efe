"""Stage 1-3 training on a real MI355X: the focal cross-entropy kernel (csrc/chan_ce.hip) against torch fp64 autograd of the
reference expression, its bits, a target outside the classes, the reference's own FocalCrossEntropyLoss (tests/golden/focal.npz),
the tape op, and the trainer with the beta grid sampler and the focal code loss."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def relerr(a, b):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


def focal_fp64(logits, target, gamma, weight, reduction="mean"):
    """(loss, d loss / d logits) of FocalCrossEntropyLoss.forward (cross_entropy_loss.py:42-53) in torch fp64 on the CPU."""
    lg = logits.detach().cpu().double().requires_grad_(True)
    tgt = target.cpu().long()
    ce = F.cross_entropy(lg, tgt, reduction="none")
    pt = F.softmax(lg, dim=1).gather(1, tgt.unsqueeze(1)).squeeze(1)
    f = ((1 - pt) ** gamma) * ce
    loss = weight * (f.mean() if reduction == "mean" else f.sum())
    loss.backward()
    return loss.detach().reshape(1), lg.grad


# (N, C, H, W, what, logits scale or None for "max |x| = 80"): the trainer's shape, the fixture's, one position, ragged tails below
# and above one 64-position workgroup, the streaming path (C > 272), the smallest C, both sides of the register-resident threshold
CASES = [(8, 256, 32, 32, "trainer", 2.0), (2, 256, 8, 8, "fixture shape", 2.0), (1, 256, 1, 1, "one position", 2.0), (3, 5, 7, 11, "ragged 77", 2.0),
         (2, 1000, 10, 13, "ragged 130, streaming", 2.0), (2, 2, 5, 9, "C = 2", 2.0), (2, 256, 8, 8, "+-80", None), (2, 1000, 3, 5, "+-80 streaming", None),
         (2, 272, 9, 9, "last cached C", 2.0), (2, 273, 9, 9, "first streaming C", 2.0)]
GAMMAS = (0.0, 1.0, 2.0, 5.0)
VALUE_TOL, GRAD_TOL = 1e-6, 1e-5           # the bounds tests/test_gpu_oasis.py holds dcvic_cross_entropy_f32 and dcvic_oasis_ce_f32 to


def make_case(case):
    """Logits and targets of a case: targets include 0 and C - 1; every case with more than one position has exactly one position made
    confidently right (target logit + 40)."""
    N, C, H, W, what, scale = case
    lg = rnd(N, C, H, W, seed=300 + C + H)
    lg = lg * scale if scale is not None else lg * (80.0 / float(lg.abs().max()))
    idx = torch.randint(0, C, (N, H, W), generator=torch.Generator().manual_seed(301))
    if N * H * W > 1:
        idx.view(-1)[0], idx.view(-1)[-1] = 0, C - 1
        n, y, x = N - 1, H // 2, W // 2
        lg[n, idx[n, y, x], y, x] += 40.0
    return lg.contiguous(), idx


@pytest.fixture(scope="module")
def references():
    """The fp64 references, computed once per (case, gamma) and shared."""
    cache = {}

    def get(i, gamma):
        if (i, gamma) not in cache:
            lg, idx = make_case(CASES[i])
            cache[(i, gamma)] = (lg, idx) + focal_fp64(lg, idx, gamma, 0.5)
        return cache[(i, gamma)]
    return get


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[4] for c in CASES])
def test_focal_ce_kernel_vs_fp64(i, references):
    """Prints every measured error (profiles/focal_kernel_errors_vs_fp64.log keeps one run's lines) before it asserts."""
    from dc_vic_amd.train import kernels as K
    N, Cc, H, W, what, _ = CASES[i]
    m = N * H * W
    for gamma in GAMMAS:
        lg, idx, ref_l, ref_g = references(i, gamma)
        ld, td = lg.to(DEV), idx.to(DEV)
        loss, dl = K.focal_ce(ld, td, gamma, 0.5 / m, want_grad=True)
        ev, eg = relerr(loss, ref_l), relerr(dl, ref_g)
        line = f"[focal_ce] {what} {(N, Cc, H, W)} gamma {gamma:g}: value {float(loss):.9e} err {ev:.3e}, gradient err {eg:.3e}"
        if gamma == 0.0:                               # the path the trainer's plain cross entropy takes, on the same inputs
            nll, dl_old = K.cross_entropy(ld, td, 0.5 / m, want_grad=True)
            old = K.reduce_loss(3, nll, None, 0.5 / m)
            e_old_v, e_old_g = relerr(loss, old), relerr(dl, dl_old)
            line += f"; vs cross_entropy_f32 + reduce_loss: value {e_old_v:.3e}, gradient {e_old_g:.3e}"
        print(line)
        assert torch.isfinite(loss).all() and torch.isfinite(dl).all(), (what, gamma)
        assert ev <= VALUE_TOL and eg <= GRAD_TOL, (what, gamma, ev, eg)
        if gamma == 0.0:
            assert e_old_v <= VALUE_TOL and e_old_g <= GRAD_TOL, (what, e_old_v, e_old_g)
        # value only: the same bits, and no gradient buffer
        l2, d2 = K.focal_ce(ld, td, gamma, 0.5 / m, want_grad=False)
        assert d2 is None and torch.equal(l2, loss)
        # reduction sum = mean * N*HW
        ls, _ = K.focal_ce(ld, td, gamma, 0.5, want_grad=False)
        assert abs(float(ls) - float(loss) * m) <= 1e-6 * abs(float(loss) * m), (what, gamma, float(ls), float(loss) * m)


def test_focal_ce_is_bit_reproducible_and_ignores_buffer_contents():
    from dc_vic_amd._lib import check, lib
    from dc_vic_amd.ops import _p, _stream
    from dc_vic_amd.train import kernels as K
    for N, Cc, H, W in ((8, 256, 32, 32), (2, 1000, 10, 13)):
        ld = (rnd(N, Cc, H, W, seed=310) * 2).to(DEV)
        td = torch.randint(0, Cc, (N, H, W), generator=torch.Generator().manual_seed(311)).to(DEV)
        scale = 0.05 / (N * H * W)
        a = K.focal_ce(ld, td, 2.0, scale, want_grad=True)
        b = K.focal_ce(ld, td, 2.0, scale, want_grad=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(K.focal_ce(ld, td, 2.0, scale, want_grad=False)[0], a[0])
        # every output and the workspace pre-filled with NaN
        need = int(lib().dcvic_focal_ce_workspace_doubles(N, H * W))
        ws = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)
        loss, dl = torch.full((1,), float("nan"), device=DEV), torch.full_like(ld, float("nan"))
        check(lib().dcvic_focal_ce_f32(_p(ld), _p(td), C.c_double(2.0), C.c_double(scale), _p(loss), _p(dl), _p(ws), N, Cc, H * W, _stream()), "focal_ce")
        assert torch.equal(loss, a[0]) and torch.equal(dl, a[1])
        assert not torch.isnan(ws).any()


@pytest.mark.parametrize("shape", [(3, 5, 7, 11), (2, 272, 9, 9), (2, 273, 9, 9)], ids=["ragged, C < waves", "last cached C", "first streaming C"])
def test_focal_gamma0_and_oasis_real_share_one_core(shape):
    """The two entry points are one kernel template: focal at gamma 0 on the classes idx + 1 and OASIS (real) on the indices idx
    return the same bits, value and gradient."""
    from dc_vic_amd.train import kernels as K
    N, Cc, H, W = shape
    ld = (rnd(N, Cc, H, W, seed=340 + Cc) * 2).to(DEV)
    idx = torch.randint(0, Cc - 1, (N, H, W), generator=torch.Generator().manual_seed(341))
    idx.view(-1)[0], idx.view(-1)[-1] = 0, Cc - 2
    td = idx.to(DEV)
    s = 0.5 / (N * H * W)
    fl, fg = K.focal_ce(ld, td + 1, 0.0, s, want_grad=True)
    ol, og, _ = K.oasis_ce(ld, td, True, s, want_grad=True)
    assert torch.isfinite(fl).all() and torch.equal(fl, ol) and torch.equal(fg, og)


@pytest.mark.parametrize("bad", [-1, None], ids=["-1", "C"])
@pytest.mark.parametrize("Cc", [256, 300], ids=["cached", "streaming"])
def test_focal_ce_bad_target_gives_nan_and_is_never_an_address(bad, Cc):
    """A target of C or -1 at one position: the loss is NaN, the other positions' gradients are those of the clean call.  The logits
    are exactly their own size (no guard): the index is compared, never added to a pointer."""
    from dc_vic_amd.train import kernels as K
    N, H, W = 2, 9, 9
    ld = (rnd(N, Cc, H, W, seed=320) * 2).to(DEV)
    idx = torch.randint(0, Cc, (N, H, W), generator=torch.Generator().manual_seed(321))
    clean_l, clean_g = K.focal_ce(ld, idx.to(DEV), 2.0, 1.0 / (N * H * W), want_grad=True)
    idx2 = idx.clone()
    idx2[1, 4, 5] = Cc if bad is None else bad
    for want_grad in (True, False):
        loss, dl = K.focal_ce(ld, idx2.to(DEV), 2.0, 1.0 / (N * H * W), want_grad=want_grad)
        torch.cuda.synchronize()
        assert torch.isnan(loss).all() and torch.isfinite(clean_l).all()
        if want_grad:
            keep = torch.ones((N, H, W), dtype=torch.bool, device=DEV)
            keep[1, 4, 5] = False
            keep = keep[:, None].expand(N, Cc, H, W)
            assert torch.equal(dl[keep], clean_g[keep])


def test_focal_ce_vs_reference_module_fixture():
    """tests/golden/focal.npz (the reference's own FocalCrossEntropyLoss in fp32): values and gradients within 2e-5, the bound the
    OASIS fixture test uses."""
    from dc_vic_amd.train import kernels as K
    G = np.load(os.path.join(ROOT, "tests", "golden", "focal.npz"))
    ld, td, w = torch.from_numpy(G["logits"]).to(DEV), torch.from_numpy(G["target"]).to(DEV), float(G["loss_weight"])
    m = td.numel()
    for gamma in (0.0, 1.0, 2.0):
        for red in ("mean", "sum"):
            loss, dl = K.focal_ce(ld, td, gamma, w / m if red == "mean" else w, want_grad=True)
            ev = relerr(loss, np.asarray(G[f"loss_g{gamma:g}_{red}"]).reshape(1))
            eg = relerr(dl, G[f"grad_g{gamma:g}_{red}"])
            print(f"[focal_ce vs reference module] gamma {gamma:g} {red}: value {ev:.3e}, gradient {eg:.3e}")
            assert ev <= 2e-5 and eg <= 2e-5, (gamma, red, ev, eg)


def test_focal_tape_op_returns_the_kernel_value_and_accumulates():
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train import kernels as K
    from dc_vic_amd.train.losses import FocalCrossEntropyLoss
    N, Cc, H, W = 2, 256, 8, 8
    ld = (rnd(N, Cc, H, W, seed=330) * 2).to(DEV)
    td = torch.randint(0, Cc, (N, H, W), generator=torch.Generator().manual_seed(331)).to(DEV)
    for red, scale in (("mean", 0.05 / (N * H * W)), ("sum", 0.05)):
        kl, kg = K.focal_ce(ld, td, 2.0, scale, want_grad=True)
        v = A.Var(ld)
        val = A.focal_cross_entropy_loss(A.Ctx([]), v, td, 0.05, 2.0, red)
        assert tuple(val.shape) == (1,) and val.is_cuda and torch.equal(val, kl) and torch.equal(v.grad, kg)
        prior = (rnd(N, Cc, H, W, seed=332) * 1e-3).to(DEV)
        v2 = A.Var(ld)
        v2.grad = prior.clone()
        val2 = FocalCrossEntropyLoss(0.05, 2.0, red)(A.Ctx([]), v2, td)
        assert torch.equal(val2, kl) and torch.equal(v2.grad, prior + kg)
    with pytest.raises(ValueError, match="reduction"):
        A.focal_cross_entropy_loss(A.Ctx([]), A.Var(ld), td, 0.05, 2.0, "none")


# ------------------------------------------------------------------------------------------------ the trainer
@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


def _disc(seed=5):
    from dc_vic_amd.train import DualBetaCondTamingNLayerDiscriminator
    torch.manual_seed(seed)
    D = DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, L=10, cond_ch=8,
                                              use_pi=False, include_x=True)
    g = torch.Generator().manual_seed(seed)
    for p in D.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
    return D.to(DEV)


def _on_grid(beta, max_beta, levels=100):
    k = np.rint(beta.numpy().astype(np.float64) * levels / max_beta)
    return bool(np.array_equal(beta.numpy(), np.float32(max_beta) * (k.astype(np.float32) / np.float32(levels))) and k.min() >= 0 and k.max() <= levels)


def test_trainer_draws_betas_from_the_grid_without_selected_pairs(model):
    """config/exp1_stage1_3.yaml: use_selected_beta_pairs off.  One optimize_parameters without betas gives a finite log and leaves the
    pair it drew -- rate first, then vq, from the trainer's own generator -- as last_beta_rate / last_beta_vq."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    was = model.use_selected_beta_pairs
    model.use_selected_beta_pairs = False
    try:
        tr = DualBetaCondGanDistortionVqCodeTrainer(model, _disc(), loss_weights={"perceptual": 0.0}, seed=3)
        x = torch.rand((2, 3, 256, 256), generator=torch.Generator().manual_seed(91)) * 2 - 1
        log = tr.optimize_parameters(1, {"real_images": x})
        assert log is not None and all(np.isfinite(v) for v in log.values()), log
        ref = np.random.RandomState(3)
        for got, mx in ((tr.last_beta_rate, 3.0), (tr.last_beta_vq, 3.5)):
            want = np.float32(mx) * (ref.randint(0, 101, 2).astype(np.float32) / np.float32(100))
            assert tuple(got.shape) == (2,) and got.dtype == torch.float32 and _on_grid(got, mx) and np.array_equal(got.numpy(), want)
        tr.sample_beta_batch = False
        log = tr.optimize_parameters(2, {"real_images": x})
        assert log is not None and all(np.isfinite(v) for v in log.values()), log
        assert tuple(tr.last_beta_rate.shape) == (1,) and tuple(tr.last_beta_vq.shape) == (1,)
        assert _on_grid(tr.last_beta_rate, 3.0) and _on_grid(tr.last_beta_vq, 3.5)
        # a batch that brings its betas is trained with them
        b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
        assert tr.optimize_parameters(3, {"real_images": x, "beta_rate": b1, "beta_vq": b2}) is not None
        assert tr.last_beta_rate is b1 and tr.last_beta_vq is b2
    finally:
        model.use_selected_beta_pairs = was


def test_trainer_focal_code_loss(model):
    """The focal code loss (gamma 2) of the first step is positive and below the plain cross entropy on the same batch, betas and
    weights ((1 - p)^2 <= 1 at every position); gamma 0 is the plain value within 1e-6."""
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer
    from dc_vic_amd.train import autograd as A
    from dc_vic_amd.train.losses import CrossEntropyLoss, FocalCrossEntropyLoss
    tr = DualBetaCondGanDistortionVqCodeTrainer(model, _disc(), loss_weights={"perceptual": 0.0}, seed=3, code_ce_loss=FocalCrossEntropyLoss(0.5, 2.0))
    x = torch.rand((2, 3, 256, 256), generator=torch.Generator().manual_seed(92)) * 2 - 1
    b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])

    def code_ce(loss_obj):
        tr.code_ce_loss = loss_obj
        tr.g_group.zero_grad()
        ctx = A.Ctx([tr.g_group])
        o = tr.generator_forward(ctx, x, None, b1, b2)
        log = tr.calc_g_loss(ctx, o, b1, b2)
        ctx.tape = []
        return float(log["code_ce"].item())
    focal2 = code_ce(FocalCrossEntropyLoss(0.5, 2.0))
    plain = code_ce(None)
    assert code_ce(CrossEntropyLoss(0.5)) == plain                # the registered class is today's path, bit for bit
    focal0 = code_ce(FocalCrossEntropyLoss(0.5, 0.0))
    print(f"[focal trainer] code_ce: plain {plain:.9e}, focal gamma 2 {focal2:.9e}, focal gamma 0 {focal0:.9e}")
    assert 0.0 < focal2 < plain, (focal2, plain)
    assert abs(focal0 - plain) <= 1e-6 * plain, (focal0, plain)
    # the whole step with the focal loss given to the constructor: its first log carries that value
    tr.code_ce_loss = FocalCrossEntropyLoss(0.5, 2.0)
    log = tr.optimize_parameters(1, {"real_images": x, "beta_rate": b1, "beta_vq": b2})
    assert log is not None and all(np.isfinite(v) for v in log.values()), log
    assert abs(log["code_ce"] - focal2) <= 1e-6 * focal2, (log["code_ce"], focal2)
