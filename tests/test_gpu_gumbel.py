"""dcvic_gumbel_lut_f32 / dcvic_gumbel_lut_bwd_f32 (csrc/gumbel.hip) against tests/gumbel_ref.py, the torch restatement of
F.gumbel_softmax(hard=True) times the codebook through post_quant_conv, evaluated in fp64 and in fp32 on the same draw.

Bounds.  idx: equal (the inputs keep every argmax 1e-3 clear of a tie).  lat: the bits of ops.argmax_lut on one-hot logits, and 1e-6 of
the fp64 latent's max (four to eight fmaf terms).  dlogits: the larger of 1e-5 of the fp64 gradient's max (the project's floor) and
4 x the fp32 restatement's own error on the same inputs.  Every measured figure is printed before it is asserted
(profiles/gumbel_errors_vs_fp64.log keeps one run's lines)."""
import pytest
import torch

import gumbel_ref as R
from dc_vic_amd import _lib, ops
from dc_vic_amd.ops import _p, _stream
from dc_vic_amd.train import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
SENTINEL = -12345.0

_REF = {}


def case(name, regime):
    """The inputs of one case and, per tau, the restatement in fp64 and fp32 (computed once, shared, never written to)."""
    key = (name, regime)
    if key not in _REF:
        t = R.build_inputs(name, regime)
        ref = {}
        for tau in R.TAUS:
            for bias in (True, False):
                b = t["pq_b"] if bias else None
                i64, l64, g64 = R.restate_grad(t["logits"], t["noise"], tau, t["codebook"], t["pq_w"], b, t["glatent"], torch.float64)
                i32, l32, g32 = R.restate_grad(t["logits"], t["noise"], tau, t["codebook"], t["pq_w"], b, t["glatent"], torch.float32)
                ref[(tau, bias)] = dict(idx=i64, lat=l64, dl=g64, idx32=i32, dl32=g32)
        dev = {k: v.to(DEV) for k, v in t.items() if isinstance(v, torch.Tensor)}
        _REF[key] = (t, dev, ref)
    return _REF[key]


def guarded(shape, dtype, fill):
    """An output buffer between two sentinel guards: (whole allocation, the view the kernel writes)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), SENTINEL if dtype.is_floating_point else int(SENTINEL), dtype=dtype, device=DEV)
    view = whole[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return whole, view


def guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def run_forward(d, tau, bias, fill=float("nan"), want_idx=True):
    N, Cc, H, W = d["logits"].shape
    D = d["codebook"].shape[1]
    wi, idx = guarded((N, H, W), torch.int64, -7)
    wl, lat = guarded((N, D, H, W), torch.float32, fill)
    rc = _lib.lib().dcvic_gumbel_lut_f32(_p(d["logits"]), _p(d["noise"]), _p(idx) if want_idx else None, _p(lat), _p(d["codebook"]), _p(d["pq_w"]),
                                         _p(d["pq_b"]) if bias else None, float(tau), N, Cc, D, H * W, _stream())
    _lib.check(rc, "gumbel_lut")
    torch.cuda.synchronize()
    assert guards_intact(wi) and guards_intact(wl), "gumbel_lut wrote outside its outputs"
    return idx, lat


def run_backward(d, tau, fill=float("nan")):
    N, Cc, H, W = d["logits"].shape
    D = d["codebook"].shape[1]
    wd, dl = guarded((N, Cc, H, W), torch.float32, fill)
    rc = _lib.lib().dcvic_gumbel_lut_bwd_f32(_p(d["logits"]), _p(d["noise"]), _p(d["glatent"]), _p(d["codebook"]), _p(d["pq_w"]), float(tau), _p(dl),
                                             N, Cc, D, H * W, _stream())
    _lib.check(rc, "gumbel_lut_bwd")
    torch.cuda.synchronize()
    assert guards_intact(wd), "gumbel_lut_bwd wrote outside dlogits"
    return dl


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_forward_and_backward_vs_fp64(name, regime):
    t, d, ref = case(name, regime)
    N, Cc, H, W, D = R.SHAPES[name]
    for tau in R.TAUS:
        dl = run_backward(d, tau)
        assert bool(torch.isfinite(dl).all()), (name, regime, tau)
        for bias in (True, False):
            r = ref[(tau, bias)]
            idx, lat = run_forward(d, tau, bias)
            assert torch.equal(r["idx"], r["idx32"])                       # the precondition: fp32 and fp64 restatements agree
            assert torch.equal(idx.cpu(), r["idx"]), (name, regime, tau, bias)
            assert bool(torch.isfinite(lat).all())
            onehot = torch.zeros_like(d["logits"]).scatter_(1, idx.unsqueeze(1), 1.0)
            idx_a, lat_a = ops.argmax_lut(onehot, d["codebook"], d["pq_w"], d["pq_b"] if bias else None)
            assert torch.equal(idx_a, idx) and torch.equal(lat_a, lat), "latent bits differ from argmax_lut's"
            e_lat = float((lat.cpu().double() - r["lat"]).abs().max()) / max(float(r["lat"].abs().max()), 1e-30)
            print(f"[gumbel err] {name}/{regime} tau {tau:g} bias {int(bias)}: lat {e_lat:.3e} of max (bound 1e-6)")
            assert e_lat <= 1e-6
            # the gradient does not depend on the bias; both references are checked
            gmax = float(r["dl"].abs().max())
            e32 = float((r["dl32"].double() - r["dl"]).abs().max())
            bound = max(1e-5 * gmax, 4.0 * e32)
            err = float((dl.cpu().double() - r["dl"]).abs().max())
            print(f"[gumbel err] {name}/{regime} tau {tau:g} bias {int(bias)}: dlogits {err:.3e} (max {gmax:.3e}, fp32 restatement {e32:.3e}, "
                  f"bound {bound:.3e}, error / bound {err / bound if bound > 0 else 0.0:.3f})")
            assert err <= bound
        if Cc == 1:
            assert float(dl.abs().max()) == 0.0 and int(idx.abs().max()) == 0


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_outputs_do_not_depend_on_buffers_or_runs(name):
    """NaN-filled and zero-filled output buffers give equal bits, twice; idx is optional."""
    t, d, ref = case(name, "normal")
    for tau in (0.5, 2.0):
        i1, l1 = run_forward(d, tau, True, fill=float("nan"))
        i2, l2 = run_forward(d, tau, True, fill=0.0)
        _, l3 = run_forward(d, tau, True, fill=3.0, want_idx=False)
        assert torch.equal(i1, i2) and torch.equal(l1, l2) and torch.equal(l1, l3)
        d1, d2 = run_backward(d, tau, fill=float("nan")), run_backward(d, tau, fill=0.0)
        assert torch.equal(d1, d2)
        # the wrappers the trainer calls give the same bits
        i4, l4 = ops.gumbel_lut(d["logits"], d["noise"], d["codebook"], d["pq_w"], d["pq_b"], tau)
        assert torch.equal(i4, i1) and torch.equal(l4, l1)
        assert torch.equal(K.gumbel_lut_bwd(d["logits"], d["noise"], d["glatent"], d["codebook"], d["pq_w"], tau), d1)


@pytest.mark.parametrize("name", ["odd_classes_tile_plus_1", "d8_129_positions"])
def test_image_0_does_not_depend_on_the_batch(name):
    t, d, ref = case(name, "normal")
    one = {k: (v[:1].contiguous() if k in ("logits", "noise", "glatent") else v) for k, v in d.items()}
    for tau in (0.5, 1.0):
        ib, lb = run_forward(d, tau, True)
        i1, l1 = run_forward(one, tau, True)
        assert torch.equal(i1, ib[:1]) and torch.equal(l1, lb[:1])
        assert torch.equal(run_backward(one, tau), run_backward(d, tau)[:1])


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_constant_noise_is_argmax_lut(name):
    """e = 1 everywhere: -log(e) = 0 and the sample is the argmax -- idx and lat have ops.argmax_lut's bits on the same logits, also where
    logits tie (a plateau: the lowest index wins)."""
    t, d, ref = case(name, "normal")
    logits = d["logits"].clone()
    logits[:, :, 0, :2] = 1.25                                             # whole-column ties
    if logits.shape[1] > 2:
        logits[:, 1::2, 1, 0] = 50.0                                       # the maximum shared by every other class
    for bias in (True, False):
        b = d["pq_b"] if bias else None
        i_a, l_a = ops.argmax_lut(logits, d["codebook"], d["pq_w"], b)
        i_g, l_g = ops.gumbel_lut(logits, torch.ones_like(logits), d["codebook"], d["pq_w"], b, 1.0)
        assert torch.equal(i_g, i_a) and torch.equal(l_g, l_a)
    assert int(i_g[:, 0, 0].max()) == 0 and (logits.shape[1] <= 2 or int(i_g[0, 1, 0]) == 1)


def test_noise_outside_the_exponentials_range_gives_no_nan():
    """0, negative, Inf and NaN draws are clamped to [FLT_MIN, FLT_MAX] on load: finite outputs, idx in range."""
    t, d, ref = case("odd_classes_tile_plus_1", "normal")
    e = d["noise"].clone()
    flat = e.view(-1)
    flat[0::7] = 0.0
    flat[1::7] = -3.0
    flat[2::7] = float("inf")
    flat[3::7] = float("nan")
    bad = dict(d, noise=e)
    idx, lat = run_forward(bad, 1.0, True)
    dl = run_backward(bad, 1.0)
    assert bool(torch.isfinite(lat).all()) and bool(torch.isfinite(dl).all())
    assert int(idx.min()) >= 0 and int(idx.max()) < d["logits"].shape[1]
    clamped = e.clone()
    clamped[~(clamped >= R.FLT_MIN)] = R.FLT_MIN                           # NaN, 0 and negatives
    clamped.clamp_(max=torch.finfo(torch.float32).max)
    i2, l2 = run_forward(dict(d, noise=clamped), 1.0, True)
    assert torch.equal(i2, idx) and torch.equal(l2, lat)
