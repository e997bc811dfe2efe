"""The inference-kernel tests' CPU side (no GPU): every fp32 restatement of tests/infer_kernels_ref.py against fp64 in every regime --
within its own bound (trivially for the measured kind; for the derived kind this checks that k is not too small for a faithful fp32
evaluation) --, the loop and grid arithmetic of the kernels restated in Python, asserting that each shape of
tests/test_gpu_infer_kernels.py reaches the path it is listed for, and the fused GroupNorm statistics emulated by |mean| / std."""
import pytest
import torch

import infer_kernels_ref as R
from kernel_bounds import FEATURE_REGIMES, PEAK, SCORE_REGIMES, U, last_tile_start, regime, rnd


def worst(got, ref, bound):
    return float(((got.double() - ref).abs() / (torch.as_tensor(bound, dtype=torch.float64) + 2.0 ** -126)).max())


# ------------------------------------------------------------------------------------------------ regimes
def test_regimes_are_what_their_names_say():
    shape = (2, 80, 16, 16)
    x = {n: regime(n, shape, 1) for n in FEATURE_REGIMES}
    assert torch.equal(x["normal"], regime("normal", shape, 1)) and not torch.equal(x["normal"], regime("normal", shape, 2))
    assert abs(float(x["normal"].mean())) < 0.02 and abs(float(x["normal"].std()) - 1) < 0.02
    cm = x["offset"].mean((0, 2, 3))
    assert abs(float(cm.mean()) - 2) < 1.5 and 2 < float(cm.std()) < 4 and abs(float((x["offset"] - cm[None, :, None, None]).std()) - 1) < 0.02
    big = x["outlier"].std((0, 2, 3)) > 25
    assert big.nonzero().flatten().tolist() == [0, 37, 74]
    assert float(x["swish"].min()) > -0.3 and 0.2 < float(x["swish"].mean()) < 0.7
    s = {n: regime(n, (3, 5, 200), 2) for n in SCORE_REGIMES}
    assert float(s["flat"].max()) == float(s["flat"].min())
    assert 19 < float(s["wide"].std()) < 21
    for n in ("peak_first", "peak_last"):
        j = s[n].argmax(-1)
        lo, hi = (0, 64) if n == "peak_first" else (last_tile_start(200), 200)
        assert bool(((j >= lo) & (j < hi)).all()), n
        top = s[n].topk(2, -1).values
        assert float((top[..., 0] - top[..., 1]).min()) > PEAK - 8
    # attention inputs: the scaled scores follow the regime
    for C, HW in ((128, 128), (512, 64)):
        for n in ("peak_first", "peak_last", "flat", "wide", "normal"):
            qkv = R.attn_inputs(n, 2, C, HW, 5).double()
            S = C ** -0.5 * qkv[:, :C].transpose(1, 2) @ qkv[:, C:2 * C]
            if n.startswith("peak"):
                j = S.argmax(-1)
                lo = 0 if n == "peak_first" else HW - 64
                assert bool(((j >= lo) & (j < lo + 64)).all()) and bool((j == j[:, :1]).all())
                top = S.topk(2, -1).values
                assert float((top[..., 0] - top[..., 1]).min()) > PEAK - 12
            elif n == "flat":
                assert float(S.abs().max()) == 0
            else:
                assert abs(float(S.std()) / (20 if n == "wide" else 1) - 1) < 0.1
    q = R.swin_inputs("wide", 1, 32, 8, 8, 3)
    assert 15 < float((0.25 * (q[0, :16] * q[0, 32:48]).sum(0)).std()) < 25


# ------------------------------------------------------------------------------------------------ derived bounds: k is large enough
@pytest.mark.parametrize("name", FEATURE_REGIMES)
def test_groupnorm_restatement_within_the_derived_bound(name):
    """The apply pass in fp32 from fp64 statistics stays within 16 U sum|terms| of fp64, with room: k is not too small."""
    for c in R.GN_CASES:
        x = regime(name, (c["N"], c["C"], c["H"], c["W"]), 7)
        gamma, beta = rnd(c["C"], seed=3) + 1, rnd(c["C"], seed=4)
        for swish in (False, True):
            ref, _, _, _, terms = R.gn_forward64(x, gamma, beta, c["groups"], 1e-6, swish)
            w = worst(R.gn_forward32(x, gamma, beta, c["groups"], 1e-6, swish), ref, 16 * U * terms)
            assert w <= 0.5, (name, c["path"], swish, w)


def test_elementwise_restatements_within_their_derived_bounds():
    """sft (k = 4), add_mul_sigmoid (k = 8), chan_affine (k = 4) evaluated in fp32 as the kernels write them."""
    shape = R.EW_SMALL
    a, b, c = regime("offset", shape, 1), regime("outlier", shape, 2), regime("normal", shape, 3) * 3
    A, B, Cd = a.double(), b.double(), c.double()
    wf = torch.tensor(0.37)
    assert worst(a + wf * (a * b + c), A + wf.double() * (A * B + Cd), 4 * U * (A.abs() + 0.37 * ((A * B).abs() + Cd.abs()))) <= 1
    assert worst(a + b * (1 / (1 + torch.exp(-c))), A + B * torch.sigmoid(Cd), 8 * U * (A.abs() + B.abs() * torch.sigmoid(Cd))) <= 1
    sc, sh = rnd(3, 5, seed=6)[:, :, None, None], rnd(3, 5, seed=7, scale=2.0)[:, :, None, None]
    got = a * (1 + sc) + sh + b
    ref = A * (1 + sc.double()) + sh.double() + B
    assert worst(got, ref, 4 * U * (A.abs() * (1 + sc.double().abs()) + sh.double().abs() + B.abs())) <= 1
    # the bgemm epilogue: one rounding of alpha * acc
    acc = rnd(64, 64, seed=1, scale=30.0)
    assert worst(wf * acc, wf.double() * acc.double(), U * (wf.double() * acc.double()).abs()) <= 1


# ------------------------------------------------------------------------------------------------ measured bounds: the yardsticks
def _own_over_bound(restated, ref):
    bound, own = R.measured_bound(restated, ref)
    assert own <= bound / R.MARGIN + 1e-300 and bound >= R.FLOOR * U * float(ref.abs().max())
    return own / bound


@pytest.mark.parametrize("name", R.SOFTMAX_REGIMES)
def test_softmax_restatement(name):
    for C in R.SOFTMAX_CS:
        for P in (1, 65):
            x = R.softmax_input(name, 3, C, P, C + P)
            ref = R.softmax_c_onepass(x, torch.float64)
            assert float((ref.sum(1) - 1).abs().max()) < 1e-12
            assert float((ref - torch.softmax(x.double(), 1)).abs().max()) < 1e-14
            assert _own_over_bound(R.softmax_c_onepass(x), ref) <= 1 / R.MARGIN


def test_gemm_restatement():
    for M, N, K in ((1, 150, 15), (65, 63, 150), (64, 1, 1)):
        A, B = regime("offset", (2, M, K), 1), regime("normal", (2, K, N), 2)
        ref, _ = R.gemm_ref64(A, B, 0.37)
        assert float((R.gemm_chain(A, B, 0.37, torch.float64) - ref).abs().max()) <= 1e-12 * float(ref.abs().max()) + 1e-300
        assert _own_over_bound(R.gemm_chain(A, B, 0.37), ref) <= 1 / R.MARGIN


@pytest.mark.parametrize("name", R.ATTN_REGIMES)
def test_attention_restatement(name):
    """The online form equals the plain softmax in fp64 (so the restatement is the same function), and in fp32 sets a finite bound."""
    for C, HW, N in ((128, 64, 2), (256, 256, 1)):
        qkv = R.attn_inputs(name, N, C, HW, 9)
        qs = R.attn_queries(HW)
        ref = R.attn_ref64(qkv, C, qs)
        assert float((R.attn_online(qkv, C, qs, torch.float64) - ref).abs().max()) <= 1e-11 * float(ref.abs().max())
        r = _own_over_bound(R.attn_online(qkv, C, qs), ref)
        assert r <= 1 / R.MARGIN
    assert len(set(R.attn_queries(6144).tolist())) == 64 and int(R.attn_queries(6144).max()) == 6143


@pytest.mark.parametrize("name", list(R.SWIN_REGIMES))
def test_swin_restatement(name):
    """In fp64 the chain form equals matmul + softmax written independently; in fp32 it sets the bound."""
    for shift in (0, 4):
        qkv = R.swin_inputs(name, 2, 32, 8, 24, 4)
        table = rnd(225, 2, seed=3, scale=8.0)
        ref = R.swin_forward(qkv, table, 2, shift, torch.float64)
        # independent: per pixel of the un-shifted map, attention over the other pixels of its shifted window
        xs = torch.roll(qkv.double(), (-shift, -shift), (2, 3))
        out = torch.zeros(2, 32, 8, 24, dtype=torch.float64)
        lab = torch.zeros(8, 24, dtype=torch.long)
        if shift:
            for i, ys in enumerate((slice(0, 0), slice(0, 8 - shift), slice(8 - shift, 8))):
                for j, xsl in enumerate((slice(0, 16), slice(16, 24 - shift), slice(24 - shift, 24))):
                    lab[ys, xsl] = i * 3 + j
        for wx in range(3):
            blk = xs[:, :, :, 8 * wx:8 * wx + 8].reshape(2, 3, 2, 16, 64)             # n, qkv, head, d, token
            lb = lab[:, 8 * wx:8 * wx + 8].reshape(64)
            S = 0.25 * blk[:, 0].transpose(-1, -2) @ blk[:, 1]
            ty, tx = torch.arange(64) // 8, torch.arange(64) % 8
            rel = (ty[:, None] - ty[None, :] + 7) * 15 + (tx[:, None] - tx[None, :] + 7)
            S = S + table.double()[rel].permute(2, 0, 1)[None] + (lb[:, None] != lb[None, :]).double() * -100.0
            o = torch.softmax(S, -1) @ blk[:, 2].transpose(-1, -2)                   # n, head, token, d
            out[:, :, :, 8 * wx:8 * wx + 8] = o.transpose(-1, -2).reshape(2, 32, 8, 8)
        out = torch.roll(out, (shift, shift), (2, 3))
        assert float((out - ref).abs().max()) < 1e-12 * float(ref.abs().max())
        assert _own_over_bound(R.swin_forward(qkv, table, 2, shift), ref) <= 1 / R.MARGIN


def test_activation_restatements():
    c = regime("normal", R.EW_SMALL, 3) * 3
    for a in (R.ACT_SWISH, R.ACT_GELU, R.ACT_SIGMOID, R.ACT_HALF_TANH):
        assert _own_over_bound(R.act(a, c), R.act(a, c.double())) <= 1 / R.MARGIN
    assert torch.equal(R.act(R.ACT_LRELU02, c), torch.nn.functional.leaky_relu(c, 0.2))


def test_winograd_inputs():
    x, w, b, r = R.wino_inputs("offset_zero_sum", "wino44", 31)
    assert float(w.sum(1).abs().max()) < 1e-5 and r is not None and all(R.wino_inputs("swish", rt, 31)[3] is not None for rt in R.WINO_ROUTE_CASES)
    for route, (Cin, Cout, H, W, N, ups, res) in R.WINO_ROUTE_CASES.items():
        Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
        th = 16 if "44" in route else 8
        assert Ho % th and Wo % 32 and Cout % 64 and W % 4 == 0 and Cin % 8 == 0, route       # ragged both ways; what the kernels need


# ------------------------------------------------------------------------------------------------ the shapes reach their paths
def test_groupnorm_shapes_reach_the_loops_they_are_listed_for():
    """groupnorm_kernel's apply loop walked in Python (512 threads): the unrolled loop needs n4 > 3 * 512; in it the incremental channel
    counter must agree with i // (HW / 4) at every element (asserted inside gn_loop_counts)."""
    seen = set()
    for c in R.GN_CASES:
        HW, cg = c["H"] * c["W"], c["C"] // c["groups"]
        seen.add(c["path"])
        if c["path"] == "scalar":
            assert HW % 4 != 0
            continue
        k = R.gn_loop_counts(c["C"], HW, c["groups"])
        if c["path"] == "unrolled_sc0":
            assert cg * HW > 6144 and HW // 4 > 512 and k["sc"] == 0 and k["unrolled_min"] > 0 and k["wraps_min"] > 0
        elif c["path"] == "unrolled_twice_wraps":
            assert cg * HW > 6144 and HW // 4 < 512 and cg >= 16 and k["sc"] > 0 and k["n4"] >= 2048 + 1536
            assert k["unrolled_max"] >= 2 and k["unrolled_min"] >= 1 and k["tail_max"] > 0 and k["wraps_max"] > 2
        elif c["path"] == "unrolled_beside_tail_only":
            assert 1536 < k["n4"] % 2048 < 2048                           # some threads unrolled, the others only the tail
            assert k["unrolled_min"] == 0 and k["unrolled_max"] > 0 and k["tail_max"] >= 3 and k["wraps_max"] > 0
        elif c["path"] == "short":
            assert k["n4"] < 512 and k["unrolled_max"] == 0 and k["tail_max"] == 1
    assert seen == {"unrolled_sc0", "unrolled_twice_wraps", "unrolled_beside_tail_only", "scalar", "short"}
    for v in R.GN_VIEWS[1:]:
        assert v[0] % 4 == 0                                              # batch strides of whole float4s: only the offset misaligns
    assert R.GN_VIEWS[1][1] % 4 == 0 and R.GN_VIEWS[2][1] % 4 != 0


def test_elementwise_shapes_reach_the_grid_stride_passes():
    n, c, h, w = R.EW_BIG
    assert c * h * w > 2048 * 256 and R.ew_passes(c * h * w) >= 2 and (c * h * w) % 256
    n, c, h, w = R.EW_SMALL
    assert R.ew_passes(c * h * w) == 1 and (c * h * w) % 256
    n, c, h, w = R.PLANE_BIG
    assert R.plane_passes(h * w) >= 2 and R.plane_passes((h - 1) * (w - 1)) >= 2 and (h * w) % 256
    n, c, h, w = R.PLANE_SMALL
    assert R.plane_passes(h * w) == 1
    assert R.crop_passes(R.CROP_BIG[1] * R.CROP_BIG_OUT[0] * R.CROP_BIG_OUT[1]) >= 2
    assert R.crop_passes(R.CROP_SMALL[1] * R.CROP_SMALL_OUT[0] * R.CROP_SMALL_OUT[1]) == 1
    assert R.CROP_BIG_OUT[0] < R.CROP_BIG[2] and R.CROP_BIG_OUT[1] < R.CROP_BIG[3]


def test_gemm_and_attention_cases_cover_what_the_issue_lists():
    layouts = {(at, bt) for at, bt, *_ in R.GEMM_PATTERNS.values()}
    assert layouts == {(False, False), (False, True), (True, False), (True, True)}          # the four a_kfast / b_kfast stagings
    assert len(R.GEMM_PATTERNS) == 8
    ks = {(M, R.GEMM_KS[(i + j) % 5]) for i, M in enumerate(R.GEMM_SIZES) for j in range(5)}
    assert len(ks) == 25                                                                     # every K meets every M (and N)
    blocks = [N * hw[0] * hw[1] // 64 for _, hw, N in R.ATTN_CASES]
    assert any(b % 8 == 0 for b in blocks) and any(b % 8 for b in blocks) and any(hw == (8, 8) for _, hw, _ in R.ATTN_CASES)
    assert sum(1 for _, hw, _ in R.ATTN_CASES if hw == (64, 96)) == 1
    assert 64 * (256 // 128) ** 2 >= 256                                                     # tiles128 * batch >= the CU count (256)


# ------------------------------------------------------------------------------------------------ fused statistics by |mean| / std
def test_fused_statistics_emulated_by_mean_over_std(capsys):
    """The F(4x4) epilogue's partial sums (32 fp32 terms per lane, four shuffle levels, tiles added in fp64) emulated on unit-variance
    maps shifted to |mean| / std = 0 .. 100: the GroupNorm + swish output against the same apply pass from fp64 statistics, relative to
    the maximum.  2e-6 holds up to a ratio of 10 and not at 30; the error grows with E[x^2] / var = 1 + ratio^2."""
    rows = []
    for ratio in R.FUSED_RATIOS:
        rows.append((ratio, R.fused_stats_error(ratio, 128, 128, 128, 32), R.fused_stats_error(ratio, 512, 64, 64, 32)))
    with capsys.disabled():
        print("\n|mean|/std   cg = 4 at 128x128   cg = 16 at 64x64")
        for r in rows:
            print(f"{r[0]:>10}   {r[1]:>17.2e}   {r[2]:>16.2e}")
    for ratio, a, b in rows:
        if ratio <= R.FUSED_HOLDS_TO:
            assert max(a, b) < R.FUSED_TOL, (ratio, a, b)
        assert max(a, b) < 36 * U * (1 + ratio * ratio) * (1 + 0.75 * 4) * 1.1, (ratio, a, b)   # the derived term at |xh| <= 4, gamma = 1
    assert max(rows[-1][1:]) > R.FUSED_TOL                                          # ... and does not hold at 100
    # the emulated partials are the sums of the map
    x = regime("swish", (2, 8, 19, 36), 3)
    S, Q = R.fused_stats(x)
    assert float((S - x.double().sum((2, 3))).abs().max()) < 36 * U * float(x.double().abs().sum((2, 3)).max())
    assert float((Q - (x.double() ** 2).sum((2, 3))).abs().max()) < 36 * U * float((x.double() ** 2).sum((2, 3)).max())
