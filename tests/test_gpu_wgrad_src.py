"""dcvic_conv_wgrad_src_f32 on a real MI355X: the weight gradient of a multi-source convolution, one call per channel-slice source,
against dcvic_conv_wgrad_f32 on the concatenated input -- bit for bit (both perform the same per-channel reduction: the same fp32
MFMA chain over each slab's pixels and the same ascending slab order; the slabs are those of the whole layer)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def K():
    from dc_vic_amd.train import kernels
    return kernels


@pytest.mark.parametrize("k,p,s", [(3, 1, 1), (5, 2, 1), (3, 1, 2), (5, 2, 2)], ids=lambda v: str(v))
def test_per_source_wgrad_equals_wgrad_of_the_concatenation(k, p, s):
    """Sources of 5 and 37 channels (+ a third of 32), M 33 and 224, maps 4x8 and 16x16, write and accumulate; the sources are
    non-contiguous channel slices of a larger NaN-padded buffer; a second run gives the same bits."""
    for chans in ((5, 37), (5, 37, 32)):
        for M in (33, 224):
            for Hx, Wx in ((4, 8), (16, 16)):
                for acc in (False, True):
                    N, Ct = 2, sum(chans)
                    Hg, Wg = (Hx + 2 * p - k) // s + 1, (Wx + 2 * p - k) // s + 1
                    seed = 100 * M + 10 * Hx + len(chans)
                    G = rnd(N, M, Hg, Wg, seed=seed).to(DEV)
                    big = torch.full((N, Ct + 2 * len(chans) + 3, Hx, Wx), NAN, device=DEV)          # gaps between the sources stay NaN
                    srcs, off = [], 3
                    for i, c in enumerate(chans):
                        v = big[:, off:off + c]
                        v.copy_(rnd(N, c, Hx, Wx, seed=seed + 1 + i).to(DEV))
                        srcs.append(v)
                        off += c + 2
                    assert not any(v.is_contiguous() for v in srcs)
                    X = torch.cat(srcs, dim=1).contiguous()
                    dW0 = rnd(M, Ct, k, k, seed=seed + 7).to(DEV) if acc else torch.full((M, Ct, k, k), NAN, device=DEV)
                    want = dW0.clone()
                    K().conv_wgrad(G, X, want, k, k, s, p, accumulate=acc)
                    runs = []
                    for _ in range(2):
                        got = dW0.clone()
                        off = 0
                        for v, c in zip(srcs, chans):
                            K().conv_wgrad_src(G, v, got, off, k, k, s, p, accumulate=acc)
                            off += c
                        runs.append(got)
                    what = f"chans {chans} M {M} map {Hx}x{Wx} k{k} p{p} s{s} acc {acc}"
                    assert torch.isfinite(want).all() and bool(want.abs().max() > 0), what
                    assert torch.equal(runs[0], want), f"{what}: max |diff| {float((runs[0] - want).abs().max()):.3e}"
                    assert torch.equal(runs[1], runs[0]), f"{what}: not reproducible"


def test_one_source_touches_only_its_channels():
    """Write mode into channels [2, 39) of a 41-channel gradient full of NaN: the other channels stay NaN, and the written ones equal the
    existing entry point's on the input padded with zero channels to the same 41 (same Cx_total, hence the same slabs)."""
    N, M, Cs, H, W, k = 2, 33, 37, 16, 16, 5
    G, X = rnd(N, M, H, W, seed=1).to(DEV), rnd(N, Cs, H, W, seed=2).to(DEV)
    got = torch.full((M, Cs + 4, k, k), NAN, device=DEV)
    K().conv_wgrad_src(G, X, got, 2, k, k, 1, 2, accumulate=False)
    assert bool(torch.isnan(got[:, :2]).all()) and bool(torch.isnan(got[:, 2 + Cs:]).all())
    Xp = torch.zeros((N, Cs + 4, H, W), device=DEV)
    Xp[:, 2:2 + Cs] = X
    want = torch.empty((M, Cs + 4, k, k), device=DEV)
    K().conv_wgrad(G, Xp, want, k, k, 1, 2, accumulate=False)
    assert torch.equal(got[:, 2:2 + Cs], want[:, 2:2 + Cs])
    with pytest.raises(Exception, match="dcvic_conv_wgrad_src_f32"):
        K().conv_wgrad_src(G, X, got, 5, k, k, 1, 2)                  # 5 + 37 > 41: refused before any launch
