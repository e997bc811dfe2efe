"""The beta-selection set of stage 2: a folder of <name>.png crops and, where present, <name>.npy VQ tokens, as written by
scripts/build_openimage_val_dataset.py and read by scripts/binary_rate_search.py and scripts/beta_selection.py.

A probe of the search encodes every item, and the search makes about 700 probes.  Where the folder allows it the set therefore lives
on the device once: the images as ONE uint8 [M, H, W, 3] array, the tokens as ONE [M, h, w] array (uint8 as stored, else int64).
`batches(bs)` then yields (x, tokens) with x = dcvic_u8_hwc_to_f32_nchw over a slice of the image array (csrc/tokens.hip) and tokens a
slice of the token array, which the model's vq_encode hands to dcvic_vq_token_feat_f32 as it is; run_one_search and run_model take the
encoder's feature tensor from the same launch, so the ingest has no upload and no torch compute op.

The device-resident case needs all images of one shape and tokens for every image (of shape (H / 8, W / 8)) or for none, within a byte
budget.  Any other folder is served from host tensors exactly as binary_rate_search.load_dataset and batches serve it.

Tokens are validated once on the host, at load: a wrong shape, a non-integer dtype or a value outside [0, n_embed) is a ValueError
naming the file."""
from __future__ import annotations

import os
import sys
from glob import glob
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .io_pipeline import decode_png_u8

TOKEN_STRIDE = 8                  # the f8 VQGAN: one token per 8 x 8 pixels
PAD_STRIDE = 64                   # BaseModel.stride: the model pads an image to multiples of it before it tokenises
DEFAULT_BUDGET = 2 << 30


def padded_token_shape(H: int, W: int) -> Tuple[int, int]:
    """Shape of the tokens the model computes for an H x W image (pad_images, then one token per 8 x 8 pixels)."""
    up = lambda v: -(-v // PAD_STRIDE) * PAD_STRIDE
    return up(H) // TOKEN_STRIDE, up(W) // TOKEN_STRIDE


def validate_tokens(path: str, tok: np.ndarray, H: int, W: int, n_embed: int) -> np.ndarray:
    """The array of a token file, checked against its H x W image and the codebook size."""
    if not isinstance(tok, np.ndarray) or tok.dtype.kind not in "iu":
        raise ValueError(f"{path}: tokens must be integers, the file holds {getattr(tok, 'dtype', type(tok).__name__)}")
    want = padded_token_shape(H, W)
    if tuple(tok.shape) != want:
        raise ValueError(f"{path}: tokens of shape {tuple(tok.shape)}, a {H} x {W} image has {want}")
    if tok.size and (int(tok.min()) < 0 or int(tok.max()) >= n_embed):
        raise ValueError(f"{path}: token values span [{int(tok.min())}, {int(tok.max())}], outside [0, n_embed = {n_embed})")
    return tok


def residency(shapes: Sequence[Tuple[int, int]], tokens: Sequence[Optional[Tuple[Tuple[int, int], str]]], budget: int = DEFAULT_BUDGET):
    """(resident, reason): whether a folder takes the device-resident path.  shapes: (H, W) per image; tokens: per image None or
    (token shape, dtype name).  Pure: the decision of SelectionSet, testable without a device."""
    if not shapes:
        return False, "the folder holds no png"
    H, W = shapes[0]
    if any(s != (H, W) for s in shapes):
        return False, "the images differ in shape"
    have = [t is not None for t in tokens]
    if any(have) and not all(have):
        return False, f"only {sum(have)} of {len(have)} images have tokens"
    nbytes = len(shapes) * H * W * 3
    if all(have):
        if H % TOKEN_STRIDE or W % TOKEN_STRIDE or any(t[0] != (H // TOKEN_STRIDE, W // TOKEN_STRIDE) for t in tokens):
            return False, f"the tokens are not of shape ({H} / {TOKEN_STRIDE}, {W} / {TOKEN_STRIDE})"
        item = 1 if all(t[1] == "uint8" for t in tokens) else 8
        nbytes += len(shapes) * (H // TOKEN_STRIDE) * (W // TOKEN_STRIDE) * item
    if nbytes > budget:
        return False, f"the set needs {nbytes} bytes on the device, over the budget of {budget} bytes (max_device_bytes)"
    return True, f"{len(shapes)} images of {H} x {W}, {'with' if all(have) else 'without'} tokens, {nbytes} bytes on the device"


def host_item(img: np.ndarray, tok: Optional[np.ndarray]):
    """One item of the host list (binary_rate_search.load_dataset calls this): fp32 [3, H, W] in [-1, 1] and int64 tokens or None."""
    x = (torch.from_numpy(img.copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5
    return x, (None if tok is None else torch.from_numpy(tok.astype(np.int32)).long())


def host_batches(items, bs: int):
    """The host list's partition (binary_rate_search.batches calls this): consecutive items of equal shape, all with or all without
    tokens, up to bs."""
    i = 0
    while i < len(items):
        j = i + 1
        while j < len(items) and j - i < bs and items[j][0].shape == items[i][0].shape and (items[j][1] is None) == (items[i][1] is None):
            j += 1
        x = torch.stack([it[0] for it in items[i:j]])
        idx = torch.stack([it[1] for it in items[i:j]]) if items[i][1] is not None else None
        yield x, idx
        i = j


class SelectionSet:
    """SelectionSet(root, device, n_embed): the sorted *.png of `root` with their tokens.  `resident` says which path the folder took
    and `reason` why; `names` are the png file names in order; `items` is the host list of the fallback (None when resident)."""

    def __init__(self, root: str, device, n_embed: int, max_device_bytes: int = DEFAULT_BUDGET):
        self.root, self.device, self.n_embed = root, torch.device(device), int(n_embed)
        paths = sorted(glob(os.path.join(root, "*.png")))
        self.names: List[str] = [os.path.basename(p) for p in paths]
        imgs, toks = [], []
        for p in paths:
            img = decode_png_u8(p)
            npy = p.replace(".png", ".npy")
            tok = None
            if os.path.exists(npy):
                tok = validate_tokens(npy, np.load(npy), img.shape[0], img.shape[1], self.n_embed)
            imgs.append(img)
            toks.append(tok)
        self.resident, self.reason = residency([im.shape[:2] for im in imgs], [None if t is None else (tuple(t.shape), t.dtype.name) for t in toks],
                                               max_device_bytes)
        self.images = self.tokens = self.table = self.items = None
        if self.resident:
            from .train.data import conversion_table
            self.images = torch.from_numpy(np.stack(imgs)).to(self.device)
            if toks[0] is not None:
                u8 = all(t.dtype == np.uint8 for t in toks)
                self.tokens = torch.from_numpy(np.stack([t if u8 else t.astype(np.int64) for t in toks])).to(self.device)
            self.table = conversion_table().to(self.device)
        else:
            if paths:
                print(f"[selection_set] {root}: served from host memory, {self.reason}", file=sys.stderr, flush=True)
            self.items = [host_item(im, t) for im, t in zip(imgs, toks)]

    def __len__(self) -> int:
        return len(self.names)

    def batches(self, bs: int) -> Iterator[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
        """(x fp32 [n, 3, H, W], tokens [n, h, w] or None) over consecutive chunks of bs items, the last one ragged: on the device
        when resident, else the host tensors of binary_rate_search.batches."""
        if not self.resident:
            yield from host_batches(self.items, bs)
            return
        from . import ops
        for i in range(0, len(self), bs):
            x = ops.u8_hwc_to_f32_nchw(self.images[i:i + bs], self.table)
            yield x, (None if self.tokens is None else self.tokens[i:i + bs])
