"""What the kernel tests that compare with fp64 share: the unit roundoff, seeded inputs, the per-element comparison that records the worst
error / bound of each kernel family, device views with a batch stride and a storage offset, and the named input regimes.

A plain module: no fixtures, nothing that needs a GPU at import."""
import json
import os

import torch
import torch.nn.functional as F

DEV = "cuda:0"
U = 2.0 ** -24                    # unit roundoff of fp32
TINY = 2.0 ** -126                # absolute floor: results below the smallest normal may be flushed
RATIOS = {}


def ratios_mark():
    """The families recorded so far: a test module takes this mark before its tests run and hands it to write_ratios, so that the file
    it writes holds its own families only, whatever other module ran before it in the session."""
    return set(RATIOS)


def write_ratios(extra=None, since=()):
    """With DCVIC_TEST_RATIOS=<file>: the worst error / bound of each kernel family first checked after the mark `since` (ratios_mark),
    and `extra` (a dict of further records), written there as JSON."""
    path = os.environ.get("DCVIC_TEST_RATIOS")
    if path:
        rec = {k: v for k, v in sorted(RATIOS.items()) if k not in since}
        rec.update(extra or {})
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def urnd(*shape, seed=0, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


def cpu64(t):
    return t.detach().cpu().double()


def within(family, got, ref, bound, what=""):
    """|got - ref| <= bound + TINY element by element; records the worst ratio of the family."""
    got = cpu64(got)
    ref = ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{family} {what}: non-finite output"
    ratio = (got - ref).abs() / (bound + TINY)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    if worst > 1.0:
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError(f"{family} {what}: error / bound = {worst:.3g} at {idx}: got {got.flatten()[i].item()!r} "
                             f"ref {ref.flatten()[i].item()!r} bound {bound.flatten()[i].item():.3g}")
    return worst


def view_on_device(t, extra=0, offset=0):
    """A device copy of the contiguous [N, C, H, W] tensor t with batch stride C*H*W + extra and storage offset `offset` (floats):
    a channel-slice-like view (batch stride != C*H*W); an odd offset makes the base pointer misaligned for 16-byte loads."""
    N, Cc, H, W = t.shape
    bs = Cc * H * W + extra
    buf = torch.full((offset + N * bs,), float("nan"), dtype=torch.float32, device=DEV)
    v = buf.as_strided((N, Cc, H, W), (bs, H * W, W, 1), offset)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------------ input regimes
FEATURE_REGIMES = ("normal", "offset", "outlier", "swish")
SCORE_REGIMES = ("normal", "flat", "wide", "peak_first", "peak_last")
PEAK = 60.0                       # how far the dominant key of a peak_* row stands above the others


def last_tile_start(keys):
    """First key of the last 64-key tile."""
    return (keys - 1) // 64 * 64


def regime(name, shape, seed):
    """A seeded fp32 input of one named family.

    Feature maps, shape [N, C, H, W] (what a trained decoder feeds its kernels, next to the N(0, 1) data the error budgets were measured on):
      normal   randn
      offset   randn plus a per-channel mean drawn N(0, 3^2), plus 2   (a residual stream)
      outlier  randn with every 37th channel (0, 37, 74, ...) times 50
      swish    silu(1.5 randn + 0.5)                                   (positive, mean about 0.3)
    Scores, shape [..., rows, keys]:
      flat        all equal
      wide        20 randn
      peak_first  randn, one key per row raised by 60, inside the first 64-key tile
      peak_last   the same inside the last 64-key tile"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if name == "normal":
        return x
    if name == "offset":
        mean = 3.0 * torch.randn(shape[1], generator=g)
        return x + mean.reshape((1, -1) + (1,) * (len(shape) - 2)) + 2.0
    if name == "outlier":
        x[:, ::37] *= 50.0
        return x
    if name == "swish":
        return F.silu(1.5 * x + 0.5)
    if name == "flat":
        return torch.full(shape, 0.75)
    if name == "wide":
        return 20.0 * x
    if name in ("peak_first", "peak_last"):
        keys = shape[-1]
        lo = 0 if name == "peak_first" else last_tile_start(keys)
        hi = min(keys, 64) if name == "peak_first" else keys
        j = torch.randint(lo, hi, tuple(shape[:-1]) + (1,), generator=g)
        return x.scatter_add(-1, j, torch.full(j.shape, PEAK))
    raise ValueError(name)
