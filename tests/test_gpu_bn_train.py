"""The batch-statistics kernels (csrc/bn_train.hip, include/dcvic_bn.h) on a real MI355X against torch fp64 on the CPU:
F.batch_norm(training=True) + LeakyReLU(0.2) with autograd, and scale * (x + loc) for ActNorm.

Shapes: test_disc_norm_host.GPU_SHAPES, the smallest at which each path of the kernels is reached (the host test restates the loop
arithmetic and names the path of each).  Every shape runs in four input regimes (normal; offset: mean = 1e3 x std; small: std 1e-3;
const: channel 0 constant) with and without the fused LeakyReLU, dense and on views with a foreign batch stride and a misaligned base
(which must give the dense run's bits), into NaN-filled outputs between NaN guards, and twice for equal bits.

Bounds: max(floor, 4 x the error of the same torch expressions run in fp32 on the CPU on the same inputs) -- floors 1e-6 of the
tensor's largest magnitude for y, mean, rstd / std and the running statistics, 1e-5 for gradients.  Gradient errors are measured
against the scale of their terms (dx: |gamma| * rstd * max|g| per channel; the parameter gradients: the sum of the terms'
magnitudes), not the result's own maximum: at M = 2 the exact dx cancels to about 0.

Fused LeakyReLU: the sign of y is a decision.  The kernel's own sign mask is fed to the references; the positions whose fp64 value
shows the other sign are capped at max(1, 1e-5 x elements) and must lie within 1e-4 of zero (analysis_train_ref.tie_report's rule).

Set DCVIC_TEST_RATIOS=<file> to have the worst error / bound of each family written there as JSON."""
import pytest
import torch
import torch.nn.functional as F

from kernel_bounds import DEV, TINY, ratios_mark, rnd, urnd, view_on_device, within, write_ratios
from test_disc_norm_host import GPU_SHAPES

pytestmark = pytest.mark.gpu

REGIMES = ("normal", "offset", "small", "const")
FLOOR, GRAD_FLOOR = 1e-6, 1e-5
EPS, MOM = 1e-5, 0.1
ACT_NONE, ACT_LRELU = 0, 2


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    mark = ratios_mark()
    yield
    write_ratios(since=mark)


def make_x(regime, shape, seed):
    x = rnd(*shape, seed=seed)
    if regime == "offset":
        x = x + 1000.0
    elif regime == "small":
        x = x * 1e-3
    elif regime == "const":
        x[:, 0] = 0.37
    return x


def guarded(shape, extra=5, offset=1, guard=64):
    """A NaN-filled device buffer and a [N, C, H, W] view into it with batch stride C*H*W + extra behind `guard + offset` floats."""
    N, Cc, H, W = shape
    bs = Cc * H * W + extra
    buf = torch.full((guard + offset + N * bs + guard,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf.as_strided((N, Cc, H, W), (bs, H * W, W, 1), guard + offset)


def assert_only_view_written(buf, view, what):
    mark = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    mark.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    assert torch.isnan(buf[~mark]).all(), f"{what}: written outside its view"
    assert torch.isfinite(view).all(), f"{what}: NaN left inside its view"


def guarded_vec(C):
    buf = torch.full((C + 32,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[16:16 + C]


def tie_check(mask, v64, what):
    flips = mask.cpu() != (v64 > 0)
    n = int(flips.sum())
    assert n <= max(1, int(1e-5 * v64.numel())), f"{what}: {n} sign flips against fp64"
    if n:
        assert float(v64[flips].abs().max()) < 1e-4, f"{what}: a flipped sign {float(v64[flips].abs().max()):.3g} from zero"
    return n


def lrelu_masked(v, mask):
    return v if mask is None else torch.where(mask, v, 0.2 * v)


def bn_reference(x, g, gamma, beta, rm, rv, mask, dtype):
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    x, gamma, beta = leaf(x), leaf(gamma), leaf(beta)
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    v = F.batch_norm(x, rm, rv, gamma, beta, True, MOM, EPS)
    y = lrelu_masked(v, mask)
    y.backward(g.to(dtype))
    with torch.no_grad():
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        rstd = 1 / torch.sqrt(var + EPS)
        gp = g.to(dtype) if mask is None else torch.where(mask, g.to(dtype), 0.2 * g.to(dtype))
        xhat = (x - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
        scales = dict(dbeta=gp.abs().sum((0, 2, 3)), dgamma=(gp * xhat).abs().sum((0, 2, 3)))
    return dict(v=v.detach(), y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, rm=rm, rv=rv, mean=mean, rstd=rstd, scales=scales)


def tol_abs(ref64, ref32, floor=FLOOR):
    """max(floor x the largest magnitude, 4 x the fp32 restatement's error), one number for the tensor."""
    return max(floor * float(ref64.abs().max()), 4 * float((ref32.double() - ref64).abs().max()))


def tol_scaled(ref64, ref32, scale, floor=GRAD_FLOOR):
    """A bound per element: scale x max(floor, 4 x the fp32 restatement's error over the same scale)."""
    scale = scale.double() + TINY
    return scale * max(floor, 4 * float(((ref32.double() - ref64).abs() / scale).max()))


def run_bn(K, x, g, gamma, beta, rm0, rv0, act, view):
    """One forward and backward through the kernels: dense operands, or every tensor a strided, misaligned view with NaN-guarded outputs."""
    shape = tuple(x.shape)
    Cc = shape[1]
    xd = view_on_device(x, extra=5, offset=1) if view else x.to(DEV)
    gd = view_on_device(g, extra=3, offset=2) if view else g.to(DEV)
    rm, rv = rm0.to(DEV).clone(), rv0.to(DEV).clone()
    ybuf, yv = guarded(shape, extra=7 if view else 0, offset=3 if view else 0)
    dxbuf, dxv = guarded(shape, extra=9 if view else 0, offset=1 if view else 0)
    y, mean, rstd = K.bn_train_fwd(xd, gamma.to(DEV), beta.to(DEV), rm, rv, MOM, EPS, act, out=yv)
    assert y is yv
    gbuf, dg = guarded_vec(Cc)
    bbuf, db = guarded_vec(Cc)
    dx = K.bn_train_bwd(xd, gd, yv if act else None, mean, rstd, gamma.to(DEV), dg, db, accumulate=False, act=act, dx=dxv)
    torch.cuda.synchronize()
    assert_only_view_written(ybuf, yv, "y")
    assert_only_view_written(dxbuf, dxv, "dx")
    for b, v in ((gbuf, dg), (bbuf, db)):
        assert torch.isnan(b[:16]).all() and torch.isnan(b[16 + Cc:]).all() and torch.isfinite(v).all()
    return dict(y=y.contiguous(), dx=dx.contiguous(), dgamma=dg.clone(), dbeta=db.clone(), mean=mean, rstd=rstd, rm=rm, rv=rv)


@pytest.mark.parametrize("shape", list(GPU_SHAPES), ids=["x".join(map(str, s)) for s in GPU_SHAPES])
def test_bn_train_against_fp64(shape):
    from dc_vic_amd.train import kernels as K
    N, Cc, H, W = shape
    for ri, regime in enumerate(REGIMES):
        x, g = make_x(regime, shape, 10 + ri), rnd(*shape, seed=20 + ri)
        gamma, beta = urnd(Cc, seed=30 + ri, lo=0.5, hi=1.5), rnd(Cc, seed=40 + ri, scale=0.5) + 0.1
        rm0, rv0 = rnd(Cc, seed=50 + ri), urnd(Cc, seed=60 + ri, lo=0.5, hi=2.0)
        for act in (ACT_NONE, ACT_LRELU):
            what = f"{shape} {regime} act {act}"
            out = run_bn(K, x, g, gamma, beta, rm0, rv0, act, view=False)
            again = run_bn(K, x, g, gamma, beta, rm0, rv0, act, view=False)
            viewed = run_bn(K, x, g, gamma, beta, rm0, rv0, act, view=True)
            for k in out:                      # two runs, and a run on foreign strides and a misaligned base: equal bits
                assert torch.equal(out[k], again[k]), f"{what}: {k} differs between two runs"
                assert torch.equal(out[k], viewed[k]), f"{what}: {k} differs on strided views"
            mask = (out["y"] > 0).cpu() if act else None
            r64, r32 = (bn_reference(x, g, gamma, beta, rm0, rv0, mask, dt) for dt in (torch.float64, torch.float32))
            if act:
                tie_check(out["y"] > 0, r64["v"], what)
            fam = f"bn_{regime}"
            within(fam + "_y", out["y"], r64["y"], tol_abs(r64["y"], r32["y"]), what)
            for k in ("mean", "rstd", "rm", "rv"):
                within(fam + "_stats", out[k], r64[k], tol_abs(r64[k], r32[k]), f"{what} {k}")
            dx_scale = (gamma.double().abs() * r64["rstd"] * float(g.abs().max())).view(1, -1, 1, 1).expand(shape)
            within(fam + "_dx", out["dx"], r64["dx"], tol_scaled(r64["dx"], r32["dx"], dx_scale), what)
            for k in ("dgamma", "dbeta"):
                within(fam + "_dparam", out[k], r64[k], tol_scaled(r64[k], r32[k], r64["scales"][k]), f"{what} {k}")
            if regime == "const":              # a constant channel: y is act(beta) exactly, nothing is NaN
                b0 = beta[0] if act == ACT_NONE or beta[0] > 0 else torch.tensor(0.2, dtype=torch.float32) * beta[0]
                assert torch.equal(out["y"][:, 0].cpu(), torch.full((N, H, W), float(b0))), what
                assert float(out["mean"][0]) == float(torch.tensor(0.37)), what


def test_bn_backward_accumulates_and_skips_absent_parameter_gradients():
    """accumulate adds onto what dgamma / dbeta held; without the two buffers dx has the same bits; no running pair: no update."""
    from dc_vic_amd.train import kernels as K
    shape = (3, 5, 3, 7)
    x, g = rnd(*shape, seed=1).to(DEV), rnd(*shape, seed=2).to(DEV)
    gamma, beta = urnd(5, seed=3, lo=0.5, hi=1.5).to(DEV), rnd(5, seed=4).to(DEV)
    y, mean, rstd = K.bn_train_fwd(x, gamma, beta, None, None, MOM, EPS, ACT_LRELU)
    dg, db = torch.empty(5, device=DEV), torch.empty(5, device=DEV)
    dx = K.bn_train_bwd(x, g, y, mean, rstd, gamma, dg, db, accumulate=False, act=ACT_LRELU)
    pg, pb = rnd(5, seed=5).to(DEV), rnd(5, seed=6).to(DEV)
    ag, ab = pg.clone(), pb.clone()
    K.bn_train_bwd(x, g, y, mean, rstd, gamma, ag, ab, accumulate=True, act=ACT_LRELU)
    within("bn_accumulate", ag, (pg.double() + dg.double()).cpu(), 2.0 ** -23 * float((pg.abs() + dg.abs()).max()))
    within("bn_accumulate", ab, (pb.double() + db.double()).cpu(), 2.0 ** -23 * float((pb.abs() + db.abs()).max()))
    assert torch.equal(dx, K.bn_train_bwd(x, g, y, mean, rstd, gamma, None, None, act=ACT_LRELU))
    # in place: y over x gives the same bits
    x2 = x.clone()
    y2, _, _ = K.bn_train_fwd(x2, gamma, beta, None, None, MOM, EPS, ACT_LRELU, out=x2)
    assert torch.equal(y2, y)


def an_reference(x, g, loc, scale, mask, dtype):
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    x, loc, scale = leaf(x), leaf(loc), leaf(scale)
    v = scale * (x + loc)
    y = lrelu_masked(v, mask)
    y.backward(g.to(dtype))
    with torch.no_grad():
        gp = g.to(dtype) if mask is None else torch.where(mask, g.to(dtype), 0.2 * g.to(dtype))
        scales = dict(dloc=scale.abs() * gp.abs().sum((0, 2, 3), keepdim=True), dscale=(gp * (x + loc)).abs().sum((0, 2, 3), keepdim=True))
        flat = x.transpose(0, 1).reshape(x.shape[1], -1)
        stats = dict(mean=flat.mean(1), std=flat.std(1))
    return dict(v=v.detach(), y=y.detach(), dx=x.grad, dloc=loc.grad, dscale=scale.grad, scales=scales, **stats)


def run_an(K, x, g, loc, scale, act, view):
    shape = tuple(x.shape)
    Cc = shape[1]
    xd = view_on_device(x, extra=5, offset=1) if view else x.to(DEV)
    gd = view_on_device(g, extra=3, offset=2) if view else g.to(DEV)
    ybuf, yv = guarded(shape, extra=7 if view else 0, offset=3 if view else 0)
    dxbuf, dxv = guarded(shape, extra=9 if view else 0, offset=1 if view else 0)
    ld, sd = loc.to(DEV), scale.to(DEV)
    K.actnorm_fwd(xd, ld, sd, act, out=yv)
    lbuf, dl = guarded_vec(Cc)
    sbuf, ds = guarded_vec(Cc)
    K.actnorm_bwd(xd, gd, yv if act else None, ld, sd, dl, ds, accumulate=False, act=act, dx=dxv)
    mean, std = K.bn_stats(xd)
    torch.cuda.synchronize()
    assert_only_view_written(ybuf, yv, "y")
    assert_only_view_written(dxbuf, dxv, "dx")
    for b, v in ((lbuf, dl), (sbuf, ds)):
        assert torch.isnan(b[:16]).all() and torch.isnan(b[16 + Cc:]).all() and torch.isfinite(v).all()
    return dict(y=yv.contiguous(), dx=dxv.contiguous(), dloc=dl.clone().view(1, Cc, 1, 1), dscale=ds.clone().view(1, Cc, 1, 1), mean=mean, std=std)


@pytest.mark.parametrize("shape", list(GPU_SHAPES), ids=["x".join(map(str, s)) for s in GPU_SHAPES])
def test_actnorm_and_stats_against_fp64(shape):
    from dc_vic_amd.train import kernels as K
    N, Cc, H, W = shape
    for ri, regime in enumerate(REGIMES):
        x, g = make_x(regime, shape, 110 + ri), rnd(*shape, seed=120 + ri)
        loc = -x.mean((0, 2, 3), keepdim=True) + rnd(1, Cc, 1, 1, seed=130 + ri, scale=0.1) * x.std()
        scale = urnd(1, Cc, 1, 1, seed=140 + ri, lo=0.5, hi=1.5) / (x.std() + 1e-6)
        for act in (ACT_NONE, ACT_LRELU):
            what = f"{shape} {regime} act {act}"
            out = run_an(K, x, g, loc, scale, act, view=False)
            again, viewed = run_an(K, x, g, loc, scale, act, view=False), run_an(K, x, g, loc, scale, act, view=True)
            for k in out:
                assert torch.equal(out[k], again[k]), f"{what}: {k} differs between two runs"
                assert torch.equal(out[k], viewed[k]), f"{what}: {k} differs on strided views"
            mask = (out["y"] > 0).cpu() if act else None
            r64, r32 = (an_reference(x, g, loc, scale, mask, dt) for dt in (torch.float64, torch.float32))
            if act:
                tie_check(out["y"] > 0, r64["v"], what)
            fam = f"actnorm_{regime}"
            within(fam + "_y", out["y"], r64["y"], tol_abs(r64["y"], r32["y"]), what)
            dx_scale = (scale.double().abs() * float(g.abs().max())).expand(shape)
            within(fam + "_dx", out["dx"], r64["dx"], tol_scaled(r64["dx"], r32["dx"], dx_scale), what)
            for k in ("dloc", "dscale"):
                within(fam + "_dparam", out[k], r64[k], tol_scaled(r64[k], r32[k], r64["scales"][k]), f"{what} {k}")
            for k in ("mean", "std"):
                within(f"bn_stats_{regime}", out[k], r64[k], tol_abs(r64[k], r32[k]), f"{what} {k}")
            # a per-image quantity: image 0 alone has the bits it has in the batch
            if N > 1:
                x0, g0 = x[:1].to(DEV), g[:1].to(DEV)
                y0 = K.actnorm_fwd(x0, loc.to(DEV), scale.to(DEV), act)
                assert torch.equal(y0, out["y"][:1]), what
                if H * W >= 2:
                    dx0 = K.actnorm_bwd(x0, g0, y0 if act else None, loc.to(DEV), scale.to(DEV), None, None, act=act)
                    assert torch.equal(dx0, out["dx"][:1]), what


def test_wrappers_refuse_mismatched_operands():
    from dc_vic_amd._lib import DcvicError
    from dc_vic_amd.train import kernels as K
    x = rnd(2, 4, 3, 3).to(DEV)
    v = torch.ones(4, device=DEV)
    with pytest.raises(ValueError):
        K.bn_train_fwd(x, v[:3], v, None, None, MOM, EPS)
    with pytest.raises(ValueError):
        K.bn_train_fwd(x, v, v, None, None, MOM, EPS, out=torch.empty(2, 4, 3, 4, device=DEV))
    with pytest.raises(DcvicError, match="bn_train_fwd: eps"):
        K.bn_train_fwd(x, v, v, None, None, MOM, 0.0)
    with pytest.raises(DcvicError, match="bn_stats: M = N \\* HW = 1"):
        K.bn_stats(rnd(1, 4, 1, 1).to(DEV))
