"""tests/conv_direct_ref.py checked on the CPU: the fp32 chain restatement against fp64 through torch's operators on every case of the
tables, the epilogue, the index-subset form, the `halves` predicate, and -- at 256 CUs -- that every case of the GPU file reaches the
kernel it asserts and that the table as a whole reaches every item the family's coverage list names."""
import pytest
import torch

import conv_direct_ref as R
from kernel_bounds import U


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_chain_against_fp64(c):
    """conv_chain32 + epilogue32 against conv_ref64 + the fp64 epilogue, every case, in each of its regimes: k <= 64.  Over the tables
    the worst k of this run was 16.1 (the outlier regime; 5.5 outside it)."""
    for name in c["regimes"]:
        k = R.case_reference(c, name)["k"]
        print(f"{c['id']} {name}: k = {k:.2f}")
        assert k <= R.K_MAX, (c["id"], name, k)


@pytest.mark.parametrize("d", R.DGRAD_CASES, ids=[d["id"] for d in R.DGRAD_CASES])
def test_adjoint_restatement_against_fp64_autograd(d):
    """The adjoint layers of dgrad_layer against fp64 autograd of the forward layer: k <= 64, and the adjoint identity in fp64."""
    w = R.dgrad_weight(d)
    Hf, Wf = R.out_size(R.dgrad_forward_layer(d), d["H"], d["W"])
    g = R.regime("offset", (d["N"], d["cout"], Hf, Wf), 31)
    x = R.regime("normal", (d["N"], d["cin"], d["H"], d["W"]), 32)
    dx, y = R.dgrad_ref64(d, w, g, x)
    La, wa = R.dgrad_layer(d, w)
    got = R.layer_chain32(La, [g], wa)
    terms = R.pm(R.terms64(La, [g], wa))
    k = float(((got.double() - R.pm(dx)).abs() / (U * terms)).max())
    assert k <= R.K_MAX, k
    lhs, rhs = float((dx * x.double()).sum()), float((g.double() * y).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((terms * R.pm(x).double().abs()).sum())


def test_epilogue_against_a_plain_expression():
    g = torch.Generator().manual_seed(3)
    acc = torch.randn(50, 7, generator=g)
    acc[0, 0] = -0.0
    bias, res = torch.randn(7, generator=g), torch.randn(50, 7, generator=g)
    s, t = torch.randn(50, 7, generator=g) * 0.3, torch.randn(50, 7, generator=g) * 0.3
    for a in R.ALL_ACTS:
        v = acc + bias
        v = {R.ACT_NONE: v, R.ACT_RELU: torch.relu(v), R.ACT_LRELU02: torch.nn.functional.leaky_relu(v, 0.2), R.ACT_SWISH: v * torch.sigmoid(v),
             R.ACT_GELU: torch.nn.functional.gelu(v), R.ACT_SIGMOID: torch.sigmoid(v), R.ACT_HALF_TANH: 0.5 * torch.tanh(v)}[a]
        want = (v + res) * (1 + s) + t
        got = R.epilogue32(acc, bias, a, res, (s, t))
        assert got.dtype == torch.float32
        assert float((got - want).abs().max()) <= 8 * U * float(want.abs().max() + 4), a
        assert float((R.epilogue64(acc, bias, a, res, (s, t)) - want.double()).abs().max()) <= 8 * U * float(want.abs().max() + 4), a
    # no bias keeps -0; the residual comes after the activation
    out = R.epilogue32(acc)
    assert out[0, 0] == 0 and torch.signbit(out[0, 0])
    r = torch.full((1, 1), 2.0)
    assert float(R.epilogue32(torch.full((1, 1), -1.0), None, R.ACT_RELU, r)) == 2.0
    assert float(R.epilogue32(torch.full((1, 1), 3.0), None, R.ACT_NONE, r, (torch.full((1, 1), 0.5), torch.full((1, 1), 1.0)))) == 8.5


@pytest.mark.parametrize("cid", ["s_k5s2_odd", "p_convT5_odd", "p_ups_phases", "u_ups_template", "s_downsample_asym", "e_init_nobias", "s_src3_on_chunks"])
def test_subset_form_equals_the_full_form(cid):
    c = R.CASES[R.CASE_IDS.index(cid)]
    srcs, w, _, _, _, init = R.case_inputs(c, "offset")
    full = R.layer_chain32(c["L"], srcs, w, init)
    idx = torch.randperm(full.shape[0], generator=torch.Generator().manual_seed(1))[:97]
    part = R.layer_chain32(c["L"], srcs, w, init, idx)
    assert torch.equal(part, full[idx])


def test_chain_order_is_the_stated_one():
    """(chunk asc, tap asc, channel asc), last chunk masked; halves = 2: (chunk, 4-channel half, tap, channel)."""
    assert list(R.chain_order(11, 2, 1)) == [(t, c) for t in (0, 1) for c in range(8)] + [(t, c) for t in (0, 1) for c in (8, 9, 10)]
    assert list(R.chain_order(8, 2, 2)) == [(t, c) for h in (0, 4) for t in (0, 1) for c in range(h, h + 4)]
    assert sorted(R.chain_order(20, 9, 1)) == sorted((t, c) for t in range(9) for c in range(20))
    assert sorted(R.chain_order(24, 9, 2)) == sorted((t, c) for t in range(9) for c in range(24))


HALVES_TABLE = [
    # layer, source channels, halves
    (R.C3, [64], 2), (R.C3, [8, 16], 2), (R.C3, [8, 8, 16], 2), (R.C3, [12], 1), (R.C3, [4, 4], 1), (R.C3, [5, 11], 1), (R.C3, [3], 1),
    (R.C5, [64], 1), (R.C1, [64], 1), (R.C3S2, [64], 1), (R.layer("conv", 3, 1, 0), [64], 1), (R.layer("conv", 3, 2, 0, out_hw=(4, 4)), [64], 1),
    (R.UPS_TEMPLATE, [64], 1), (R.UPS, [64], 1), (R.CT3, [64], 1), (R.CT5, [64], 1), (R.PH2, [64], 1),
]


@pytest.mark.parametrize("L,cins,want", HALVES_TABLE)
def test_halves_predicate(L, cins, want):
    """2 only for Conv2d(k3, s1, p1) whose sources are all multiples of 8 channels: not the transposed k3 (its taps step by -1), not the
    upsample template, not the 2x2 phases."""
    phases, _ = R.phases_of(L, None, 8, 8)
    assert {R.halves_of(g["desc"], cins) for g in phases} == {want}


def test_descriptors():
    d = R.desc_conv(3, 3, 2, 0, 0)
    assert d["taps"][0] == (0, 0, 0, 0) and d["taps"][8] == (2, 2, 2, 2) and R.tap_grid(d) == (3, 0, 0, 1)
    assert R.tap_grid(R.desc_convT(3)) == (3, 1, 1, -1)
    # ConvTranspose2d(k5, s2, p2, op1): phase (1, 0) has taps ky in {1, 3}, kx in {0, 2, 4}
    d = R.desc_convT(5, 1, 0)
    assert [t[:2] for t in d["taps"]] == [(1, 0), (1, 2), (1, 4), (3, 0), (3, 2), (3, 4)]
    assert [t[2:] for t in d["taps"]] == [(1, 1), (1, 0), (1, -1), (0, 1), (0, 0), (0, -1)] and R.tap_grid(d) == (3, 1, 1, -1)
    assert [R.tile_width_log(w) for w in (1, 4, 5, 8, 9, 16, 17, 33)] == [2, 2, 3, 3, 4, 4, 5, 5]
    assert [R.choose_class(c) for c in (3, 32, 33, 64, 96, 97, 128, 160, 192, 224, 320)] == [2, 2, 1, 1, 3, 1, 0, 1, 3, 0, 0]


def test_variant_score_thresholds():
    """variant_score by hand, class 0 on 8 x 17 maps (one 8 x 32 tile or two 4 x 32 tiles per image, the same useful fraction): P = 256
    scores fill = wg / 384, P = 128 scores 0.93 with twice the workgroups, so 256 pixels win from 358 workgroups on (358 / 384 = 0.9323).
    Below 128 pixels class 2 has tiles in conv_async16.hip only."""
    assert R.variant_of(0, 128, 358, 8, 17, False) == 256 and R.variant_of(0, 128, 357, 8, 17, False) == 128
    assert R.select_class(128, 358, 8, 17, False) == 0
    assert R.variant_of(2, 32, 2, 16, 16, False) == 32 and R.variant_of(2, 32, 2, 16, 16, False, use_async=0) == 128
    assert R.variant_of(2, 32, 2, 16, 16, False, use_async=2) == 128 and R.variant_of(2, 32, 2, 8, 8, True) == 128


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_case_reaches_the_variant_the_gpu_test_asserts(c):
    assert R.case_plan(c)["variant"] == c["expect"]


def test_every_listed_item_is_reached():
    tags = set()
    for c in R.CASES:
        tags |= R.reached(c)
    missing = [t for t in R.REQUIRED if t not in tags]
    assert not missing, missing
    # every family has one case in every regime, the zero-sum weights included
    for fam in {c["fam"] for c in R.CASES}:
        assert any(c["fam"] == fam and set(c["regimes"]) == set(R.ALL_REGIMES) for c in R.CASES), fam
    assert len(set(R.CASE_IDS)) == len(R.CASE_IDS)
