"""The direct convolution kernels and their adjoints (csrc/conv.hip, conv3x3.hip, conv1x1.hip, conv_async.hip, conv_async16.hip, thin.hip,
the descriptor builders, the weight pack, ConvPlan's phase algebra, train/autograd._dgrad_plan) on a real MI355X against
tests/conv_direct_ref.py.  Every case of its table makes three comparisons, element by element:

  (a) order   the kernel against the CPU restatement of its own fp32 chain (conv_chain32 + epilogue32), within 2 U sum|terms|: the two can
              differ only where the restatement's second rounding differs from a true fma; the share of bit-equal elements is recorded
  (b) value   the kernel against fp64 through torch's operators, within MARGIN x k x U x terms64 and never below 16 U |ref|, k being the
              restatement's own worst err / (U terms64) on the same input -- the yardstick is the restatement, never the kernel
  (c) bits    a rerun gives the same bits, image 0 alone the bits of image 0 in the batch, and a fast kernel (DMA tap, 1x1 DMA, async
              twins, thin) the bits of the generic kernel, in every regime the case runs in

On the large grids (every tile above the smallest needs about 358 workgroups) comparison (a) runs on the border and partial-tile pixels of the
first and last image plus seeded others (conv_direct_ref.subset_pixels), with k measured there; (b) and (c) always run on every element.
Every case asserts through dcvic_conv_last_variant() that it reached the kernel the table names (tests/test_conv_direct_host.py derives the
same variant from the host-side rules at 256 CUs).  With DCVIC_TEST_RATIOS=<file> the worst error / bound per family, comparison and
regime, the bit-equal shares and the measured k per case are written there (profiles/conv_direct_ratios.json)."""
import pytest
import torch

import conv_direct_ref as R
from kernel_bounds import DEV, RATIOS, TINY, U, cpu64, ratios_mark, view_on_device, within, write_ratios

pytestmark = pytest.mark.gpu
EXTRA = {"bit_equal_share": {}, "k": {}}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    mark = ratios_mark()
    yield
    write_ratios(EXTRA, since=mark)


def O():
    from dc_vic_amd import ops
    return ops


def Lib():
    from dc_vic_amd._lib import lib
    return lib()


def build_plan(c, w, bias):
    ops, L = O(), c["L"]
    if L["kind"] == "phases2":
        return ops.ConvPlan.from_phases2([p.to(DEV) for p in w])
    b = None if bias is None else bias.to(DEV)
    if L["kind"] == "convT":
        return ops.ConvPlan(w.to(DEV), b, "convT")
    if L["kind"] == "ups":
        return ops.ConvPlan(w.to(DEV), b, "conv", pad=(1, 1), upsample=True)
    pad = 0 if L["out_hw"] is not None else L["pad"]
    return ops.ConvPlan(w.to(DEV), b, "conv", stride=L["stride"], pad=(pad, pad))


def run(c, plan, srcs, res, aff, init, wide=None):
    """One call of the plan -> (output, variant reached)."""
    ops = O()
    out = None if wide is None else wide[:, 3:3 + c["cout"]]
    ops.kernel_events_start()
    try:
        y = plan(srcs, out=out, act=c["act"], res=res, affine=aff, out_hw=c["L"]["out_hw"], init=init, use_bias=c["bias"])
        torch.cuda.synchronize()
    finally:
        names = list(ops.kernel_events_stop())
    v = int(Lib().dcvic_conv_last_variant())
    if any("thin_" in n for n in names):
        cin = sum(c["cins"])
        v = 9200 + c["cout"] if f"thin_cout_kernel<{c['cout']}>" in names[0] else 9210 + cin
        assert names == [ops.conv_kernel_name(v)], names
    else:
        assert ops.conv_kernel_name(v) in names, (v, names)
    return y, v


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_conv_direct(c, monkeypatch):
    ops, L = O(), Lib()
    fam = c["fam"]
    monkeypatch.setenv("DCVIC_UPS_PHASES", "1" if c["L"]["ups_phases"] else "0")
    monkeypatch.setattr(ops, "THIN_ENABLED", bool(c["thin"]))
    monkeypatch.setattr(ops, "THIN_MIN_PIXELS", 0)
    N, cout = c["N"], c["cout"]
    try:
        for name in c["regimes"]:
            what = f"{c['id']} {name}"
            ref = R.case_reference(c, name)
            # the plan of init + use_bias=False carries a bias that the call must not apply
            plan_bias = ref["bias"] if not (c["init"] and not c["bias"]) else torch.ones(cout)
            plan = build_plan(c, ref["w"], plan_bias)
            if c["views"]:
                srcs = [view_on_device(s, extra=5 * c["H"] * c["W"] + 2 * i, offset=2 * i + 1) for i, s in enumerate(ref["srcs"])]
            else:
                srcs = [s.to(DEV) for s in ref["srcs"]]
            res, init = (None if t is None else t.to(DEV) for t in (ref["res"], ref["init"]))
            aff = None if ref["aff"] is None else tuple(a.to(DEV).contiguous() for a in ref["aff"])
            Hf, Wf = R.out_size(c["L"], c["H"], c["W"])
            wide = torch.full((N, cout + 5, Hf, Wf), float("nan"), device=DEV) if c["out_slice"] else None
            L.dcvic_conv_set_tuning(*c["tuning"])
            y, v = run(c, plan, srcs, res, aff, init, wide)
            assert v == c["expect"], f"{what}: reached variant {v} ({ops.conv_kernel_name(v)}), the table says {c['expect']}"
            if wide is not None:
                assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, 3 + cout:]).all(), "wrote outside the channel slice"
            y = y.clone()
            got, idx = R.pm(cpu64(y)), ref["idx"]
            # (a) order
            share = float((got[idx] == ref["chain"].double()).double().mean())
            exact = c["act"] in (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU02) and not c["aff"]      # no libm call, no contractible a b + c
            skey = fam if exact else f"{fam}/transcendental_or_affine_epilogue"
            EXTRA["bit_equal_share"][skey] = min(EXTRA["bit_equal_share"].get(skey, 1.0), share)
            EXTRA["k"][what] = round(ref["k"], 3)
            print(f"{what}: variant {v}, k = {ref['k']:.2f}, bit-equal to the restated chain {share:.6f} of {idx.numel() * cout}")
            within(f"conv_direct/{fam}/order/{name}", got[idx], ref["chain"].double(), R.ORDER_K * U * ref["terms"][idx], what)
            # (b) value
            bound = torch.maximum(R.MARGIN * ref["k"] * U * ref["terms"], R.FLOOR * U * ref["ref"].abs())
            within(f"conv_direct/{fam}/value/{name}", got, ref["ref"], bound, what)
            # (c) bits
            y2, _ = run(c, plan, srcs, res, aff, init, None if wide is None else torch.full_like(wide, float("nan")))
            assert torch.equal(y2, y), f"{what}: a rerun differs"
            if N > 1:
                one = [s[:1] for s in srcs]
                aff1 = aff if aff is None or aff[0].shape[0] == 1 else tuple(a[:1].contiguous() for a in aff)
                y1, _ = run(c, plan, one, None if res is None else res[:1], aff1, None if init is None else init[:1],
                            None if wide is None else torch.full_like(wide[:1], float("nan")))
                assert torch.equal(y1[0], y[0]), f"{what}: image 0 alone differs from image 0 in the batch"
            if fam in R.FAST_FAMILIES:
                L.dcvic_conv_set_tuning(*R.GENERIC)
                ops.THIN_ENABLED = False
                yg, vg = run(c, plan, srcs, res, aff, init)
                ops.THIN_ENABLED = bool(c["thin"])
                assert vg < 7000, (what, vg)
                assert torch.equal(yg, y), f"{what}: variant {v} differs from the generic kernel (variant {vg})"
    finally:
        L.dcvic_conv_set_tuning(*R.TUNING_DEFAULT)


@pytest.mark.parametrize("d", R.DGRAD_CASES, ids=[d["id"] for d in R.DGRAD_CASES])
def test_conv_data_gradient(d):
    """train/autograd._dgrad_plan of a layers.Conv2d / ConvTranspose2d / Linear on a seeded output gradient g (N = 2, 12 -> 20 channels:
    Cin != Cout, neither a multiple of 8) against fp64 autograd of conv_ref64 of the forward layer, under (b) with the adjoint's own
    terms64 and the adjoint restatement's k; and the adjoint identity <dgrad(g), x> = <g, conv(x)> with both sides summed in fp64,
    conv(x) the forward layer's fp64 value, within 32 U sum |g| |w| |x| -- an fp64 reference with a mirrored mistake would miss it."""
    from dc_vic_amd import layers
    from dc_vic_amd.train import autograd
    cin, cout, k = d["cin"], d["cout"], d["k"]
    if d["mod"] == "conv":
        mod = layers.Conv2d(cin, cout, k, stride=d["s"], padding=d["p"])
    elif d["mod"] == "convT":
        mod = layers.ConvTranspose2d(cin, cout, k, 2 if k == 5 else 1, d["p"], 1 if k == 5 else 0)
    else:
        mod = layers.Linear(cin, cout)
    w = R.dgrad_weight(d)
    mod.weight.data.copy_(w)
    mod = mod.to(DEV)
    plan = autograd._dgrad_plan(mod)
    Hf, Wf = R.out_size(R.dgrad_forward_layer(d), d["H"], d["W"])
    x = R.regime("offset", (d["N"], cin, d["H"], d["W"]), 32)
    La, wa = R.dgrad_layer(d, w)
    for i, name in enumerate(("normal", R.OFF_REGIMES[R.DGRAD_CASES.index(d) % 3])):
        what = f"{d['id']} {name}"
        g = R.regime(name, (d["N"], cout, Hf, Wf), 31 + i)
        dx, y = R.dgrad_ref64(d, w, g, x)
        out = plan(g.to(DEV))
        assert tuple(out.shape) == tuple(x.shape), (out.shape, x.shape)
        terms = R.terms64(La, [g], wa)
        kk = float(((R.layer_chain32(La, [g], wa).double() - R.pm(dx)).abs() / (U * R.pm(terms) + TINY)).max())
        EXTRA["k"][f"dgrad/{what}"] = round(kk, 3)
        print(f"dgrad {what}: variant {int(Lib().dcvic_conv_last_variant())}, k = {kk:.2f}")
        within(f"conv_direct/dgrad/value/{name}", out, dx, torch.maximum(R.MARGIN * kk * U * terms, R.FLOOR * U * dx.abs()), what)
        lhs, rhs = float((cpu64(out) * x.double()).sum()), float((g.double() * y).sum())
        total = float((terms * x.double().abs()).sum())
        ratio = abs(lhs - rhs) / (R.ADJOINT_K * U * total)
        key = f"conv_direct/dgrad/adjoint_identity/{name}"
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
        assert ratio <= 1.0, f"{what}: <dgrad(g), x> = {lhs!r}, <g, conv(x)> = {rhs!r}, error / bound = {ratio:.3g}"
        assert torch.equal(plan(g.to(DEV)), out), f"{what}: a rerun differs"
        assert torch.equal(plan(g[:1].to(DEV))[0], out[0]), f"{what}: image 0 alone differs from image 0 in the batch"
