"""Shared by tests/test_data_feed_host.py and tests/test_gpu_data_feed.py: generated images and folders, Pillow's own resize + crop +
flip + conversion as the yardstick, and the kernel-case builder.  Nothing here reads a file the tests did not write."""
import os

import numpy as np
import torch

from dc_vic_amd.train import data as D


def noise(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def ramp(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)], axis=2).astype(np.uint8)


def steps(H, W):
    """0 / 255 blocks of 3 x 5 pixels: bicubic overshoots at every edge, so the clip acts."""
    y, x = np.mgrid[0:H, 0:W]
    v = (((x // 3 + y // 5) % 2) * 255).astype(np.uint8)
    return np.stack([v, 255 - v, v], axis=2)


CONTENT = {"noise": lambda H, W: noise(H, W, H * 1000 + W), "ramp": ramp, "steps": steps}


def pil_resize(a, w, h, filt):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((w, h), getattr(Image, filt.upper())), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- Pillow's two passes in numpy
PRECISION_BITS = D.PRECISION_BITS


def resample_axis_u8(a, coeffs, xmin, count, axis):
    """One of Pillow's integer passes along `axis` of a uint8 [H, W, C] array: clip8((2^21 + sum_k pixel * coeff) >> 22) in int32
    with an arithmetic shift (ImagingResampleHorizontal_8bpc / Vertical_8bpc)."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + a.shape[1:], dtype=np.uint8)
    for i in range(len(xmin)):
        n = int(count[i])
        acc = np.tensordot(coeffs[i, :n].astype(np.int64), a[int(xmin[i]):int(xmin[i]) + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize_u8(a, out_w, out_h, filt="bicubic"):
    """PIL.Image.resize((out_w, out_h), filt) of a uint8 [H, W, 3] array restated: the horizontal pass, then the vertical one, each
    skipped when it leaves its axis's size unchanged."""
    H, W = a.shape[:2]
    if out_w != W:
        a = resample_axis_u8(a, *D.pil_coeffs(W, out_w, filt), axis=1)
    if out_h != H:
        a = resample_axis_u8(a, *D.pil_coeffs(H, out_h, filt), axis=0)
    return a


def resample_window_u8(win_pixels, win):
    """The two integer passes on a window's pixels (the numpy statement of what the kernel computes, before flip and conversion)."""
    a = win_pixels
    if win.tab_x is not None:
        a = resample_axis_u8(a, *win.tab_x, axis=1)
    if win.tab_y is not None:
        a = resample_axis_u8(a, *win.tab_y, axis=0)
    return a


def to_model_range(crop_u8):
    """uint8 [S, S, 3] -> fp32 [3, S, S], CropDataset's expression."""
    return (torch.from_numpy(np.array(crop_u8, dtype=np.uint8)).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5


def record(H, W, scale, filt, S, y0, x0, flip, path="memory"):
    """A CropRecord stated by hand (scale None = no resize)."""
    w, h = (W, H) if scale is None else (int(W * scale), int(H * scale))
    assert h >= S and w >= S and 0 <= y0 <= h - S and 0 <= x0 <= w - S, (H, W, scale, S, y0, x0)
    return D.CropRecord(path, H, W, scale, h, w, False, y0, x0, flip, filt)


def pillow_crop(img, rec, S):
    """Pillow's own resize of the whole image, then the crop and the flip: uint8 [S, S, 3]."""
    a = img if rec.scale is None else pil_resize(img, rec.w, rec.h, rec.interpolation)
    c = a[rec.y0:rec.y0 + S, rec.x0:rec.x0 + S]
    return c[:, ::-1] if rec.flip else c


def kernel_entry(img, rec, S):
    """(window pixels, window, flip): what the feed's worker puts into the slab for this record."""
    win = D.window(rec, S)
    return np.ascontiguousarray(img[win.r0:win.r1, win.c0:win.c1]), win, rec.flip


POSITIONS = ("top_left", "top_right", "bottom_left", "bottom_right", "interior")


def position(name, h, w, S):
    return {"top_left": (0, 0), "top_right": (0, w - S), "bottom_left": (h - S, 0), "bottom_right": (h - S, w - S),
            "interior": ((h - S) // 2, (w - S) // 2)}[name]


def pad_side(S, lo, hi):
    """A side length in [lo, hi) that the minimum factor S / side resizes to S - 1 (data_transform.py:66-72: int(side * (S / side)))."""
    for side in range(lo, hi):
        if int(side * (float(S) / float(side))) == S - 1:
            return side
    raise AssertionError(f"no pad-case side in [{lo}, {hi}) for crop {S}")


def write_folder(root, S, seed=0):
    """Five generated files for crop size S, JPEG and PNG mixed: three larger than the crop, one whose short side is a pad-case side
    above the crop, and one less high than the crop whose short side the minimum factor resizes to S - 1.  -> sorted paths."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    big, small = pad_side(S, S + 1, 4 * S), pad_side(S, S // 2, S)
    specs = [("a.jpg", 2 * S + 9, 3 * S + 5), ("b.png", S + 31, 2 * S + 2), ("c.jpeg", 3 * S, S + 17), ("d.png", big + 11, big), ("e.jpg", small, small + 2)]
    for i, (name, H, W) in enumerate(specs):
        a = (ramp(H, W).astype(np.int32) // 2 + noise(H, W, seed + i) // 2).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(root, name), **({"quality": 90} if not name.endswith("png") else {}))
    return sorted(os.path.join(root, n) for n, _, _ in specs)


def read_slab(buf, N, S):
    """A packed slab read back the way the kernel indexes it (descriptor fields, coefficients [S][k] then xmin [S] then count [S] per
    axis, rows of src_stride bytes) and run through the numpy passes -> fp32 [N, 3, S, S].  Pins the slab layout without a GPU."""
    desc = buf[:N * D.DESC_DTYPE.itemsize].view(D.DESC_DTYPE)
    out = torch.empty((N, 3, S, S), dtype=torch.float32)
    for n in range(N):
        d = desc[n]
        rows = [buf[int(d["src_off"]) + r * int(d["src_stride"]):][:3 * int(d["src_w"])].reshape(-1, 3) for r in range(int(d["src_h"]))]
        a = np.stack(rows, axis=0)
        for axis, k, tab in ((1, int(d["kx"]), int(d["tab_x"])), (0, int(d["ky"]), int(d["tab_y"]))):
            if k:
                t = buf[tab:tab + 4 * S * (k + 2)].view(np.int32)
                a = resample_axis_u8(a, t[:S * k].reshape(S, k), t[S * k:S * k + S], t[S * k + S:], axis=axis)
        assert a.shape == (S, S, 3)
        out[n] = to_model_range(a[:, ::-1] if d["flip"] else a)
    return out


# Kernel cases: (S, H, W, scale, filter, position, flip, content).  S = 37 crosses the 8 x 32 tile's edges in both directions, 64 and
# 256 are whole tiles, 3 and 16 less than one; scale 0.25 is the tap limit, 1.0 is "copy" on both axes, (40, 3) at 1.2 on one axis.
KERNEL_CASES = [
    (3, 40, 3, 1.2, "bicubic", "interior", False, "noise"), (3, 40, 3, 1.2, "bilinear", "bottom_left", True, "steps"),
    (3, 20, 31, 0.61, "bicubic", "top_right", True, "noise"),
    (16, 90, 70, 0.25, "bicubic", "top_left", False, "noise"), (16, 70, 90, 0.37, "bilinear", "bottom_right", True, "steps"),
    (16, 40, 50, 1.0, "bicubic", "interior", True, "noise"), (16, 16, 16, None, "bicubic", "top_left", False, "steps"),
    (16, 30, 41, 2.0, "bicubic", "bottom_right", False, "steps"),
    (37, 300, 424, 0.25, "bicubic", "top_left", False, "noise"), (37, 300, 424, 0.25, "bicubic", "bottom_right", True, "steps"),
    (37, 301, 425, 0.25, "bilinear", "interior", True, "noise"), (37, 150, 131, 0.37, "bicubic", "top_right", True, "steps"),
    (37, 150, 131, 0.37, "bilinear", "bottom_left", False, "noise"), (37, 90, 77, 0.61, "bicubic", "interior", False, "steps"),
    (37, 90, 77, 0.61, "bilinear", "top_left", True, "noise"), (37, 60, 51, 1.0, "bicubic", "bottom_right", True, "noise"),
    (37, 60, 51, 1.3, "bicubic", "top_right", False, "steps"), (37, 60, 51, 1.3, "bilinear", "bottom_left", True, "noise"),
    (37, 31, 40, 2.0, "bicubic", "interior", True, "noise"), (37, 31, 40, 2.0, "bilinear", "bottom_right", False, "steps"),
    (64, 300, 424, 0.25, "bicubic", "interior", True, "steps"), (64, 120, 110, 0.61, "bicubic", "bottom_left", False, "noise"),
    (64, 70, 80, 1.3, "bilinear", "top_right", True, "noise"), (64, 64, 64, 1.0, "bilinear", "top_left", True, "steps"),
    (256, 300, 340, 1.3, "bicubic", "interior", True, "noise"),
]


def build_case(case):
    """-> (slab entry, the expected fp32 [3, S, S] from Pillow's own resize + crop + flip + conversion)."""
    S, H, W, scale, filt, pos, flip, content = case
    img = CONTENT[content](H, W)
    w, h = (W, H) if scale is None else (int(W * scale), int(H * scale))
    y0, x0 = position(pos, h, w, S)
    rec = record(H, W, scale, filt, S, y0, x0, flip)
    return kernel_entry(img, rec, S), to_model_range(pillow_crop(img, rec, S))
