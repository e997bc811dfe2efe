"""The training data feed (the reference's OpenImageImageDataset + PilTrainTransform, openimage_dataset.py:14-34 and
data_transform.py:19-73): file listing, the seeded plan of the crop stream, Pillow's 8-bit resampling tables restated, and two feeds
that turn the plan into batches.

`CropPlanner` is pure host code: from the file list, the seed and the image headers it yields one `CropRecord` per image with exactly
the generator calls of scripts/train.py's `CropDataset` (the statement of the stream without resize), so nothing downstream draws a
random number.  `HostFeed` runs the records serially with Pillow (`--data_workers 0`, and the yardstick of the tests).  `TrainFeed`
decodes on worker threads, copies only the source window a crop reads as uint8 through pinned memory, and lets one HIP launch per
batch (csrc/data.hip, include/dcvic_data.h) do Pillow's two integer resampling passes, the flip, the [-1, 1] conversion and the NCHW
layout.  Every step is integer or single-rounding fp32 arithmetic: the two feeds give equal bits.
"""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2                     # Pillow's Resample.c: 8-bit coefficients carry 22 fraction bits
FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}
MAX_KSIZE = 17                                  # the kernel's tap limit (DCVIC_DATA_MAX_KSIZE): bicubic at scale 0.25
MIN_THREADED_SCALE = 0.25
DESC_DTYPE = np.dtype([("src_off", "<i8"), ("tab_x", "<i8"), ("tab_y", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("src_stride", "<i4"),
                       ("flip", "<i4"), ("kx", "<i4"), ("ky", "<i4")])          # dcvic_crop_desc, 48 bytes


# ------------------------------------------------------------------------------------------------ listing
def list_train_images(root: str, subset_list: Optional[Sequence[int]] = None) -> List[str]:
    """Without `subset_list` the flat listing of CropDataset (sorted *.png, *.jpg, *.jpeg of `root`); with it the reference's
    root/train_{k}/*.jpg over every k, sorted over all (openimage_dataset.py:14-34).  A missing train_{k} is a ValueError."""
    if subset_list is None:
        return sorted(p for ext in ("png", "jpg", "jpeg") for p in glob(os.path.join(root, f"*.{ext}")))
    paths: List[str] = []
    for k in subset_list:
        d = os.path.join(root, f"train_{k}")
        if not os.path.isdir(d):
            raise ValueError(f'subset folder "{d}" (train_{k} of subset_list) does not exist')
        paths.extend(glob(os.path.join(d, "*.jpg")))
    paths.sort()
    return paths


# ------------------------------------------------------------------------------------------------ the YAML section
def read_train_dataset(opt, threaded: bool = True) -> dict:
    """dict(root_dir, subset_list, image_size, resize_range, interpolation, batch_size) of a parsed config's `dataset` section
    (config/_base_/dataset/train_openimage_eval_kodak.yaml), pure: no file is touched.  ValueError names key and value of what is not
    built.  `threaded`: the limits of TrainFeed apply (f_min >= 0.25); HostFeed serves any positive factor."""
    ds = _get(opt, "dataset", default=None) or {}
    tr = _get(ds, "train_dataset", default=None) or {}
    known = {"name", "type", "image_size", "resize_range", "interpolation", "root_dir", "subset_list"}
    for k in tr:
        if k not in known:
            raise ValueError(f"dataset.train_dataset.{k}: {tr[k]!r} is not a key this feed reads (known: {', '.join(sorted(known))})")
    size = tr.get("image_size", 256)
    if isinstance(size, (list, tuple)) and len(size) == 2 and size[0] == size[1]:
        size = size[0]
    if not isinstance(size, int) or isinstance(size, bool) or size != 256:
        raise ValueError(f"dataset.train_dataset.image_size: {size!r} is not built, the training path is built for 256 (32 x 32 tokens)")
    interp = tr.get("interpolation", "bicubic")
    if interp not in FILTER_SUPPORT:
        raise ValueError(f"dataset.train_dataset.interpolation: {interp!r} is unknown, expected bicubic or bilinear")
    rr = tr.get("resize_range", None)
    if rr is not None:
        try:
            f_min, f_max = (float(v) for v in rr)
        except (TypeError, ValueError):
            raise ValueError(f"dataset.train_dataset.resize_range: {rr!r} is not a pair [f_min, f_max]") from None
        if not (f_min > 0.0) or not (f_min <= f_max) or f_max == float("inf"):
            raise ValueError(f"dataset.train_dataset.resize_range: {list(rr)!r} needs 0 < f_min <= f_max")
        if threaded and f_min < MIN_THREADED_SCALE:
            raise ValueError(f"dataset.train_dataset.resize_range: {list(rr)!r} has f_min < {MIN_THREADED_SCALE}, past the threaded feed's "
                             f"{MAX_KSIZE} taps per output; --data_workers 0 serves it on the host")
        rr = (f_min, f_max)
    sub = tr.get("subset_list", None)
    if sub is not None:
        if not isinstance(sub, (list, tuple)) or not sub or any(isinstance(k, bool) or not isinstance(k, int) or k < 0 for k in sub):
            raise ValueError(f"dataset.train_dataset.subset_list: {sub!r} is not a list of subset numbers")
        sub = [int(k) for k in sub]
    root = tr.get("root_dir", None)
    if root is not None and not isinstance(root, str):
        raise ValueError(f"dataset.train_dataset.root_dir: {root!r} is not a path")
    bs = ds.get("batch_size", None) if hasattr(ds, "get") else None
    if bs is not None and (isinstance(bs, bool) or not isinstance(bs, int) or bs < 1):
        raise ValueError(f"dataset.batch_size: {bs!r} is not a positive integer")
    return dict(root_dir=root, subset_list=sub, image_size=256, resize_range=rr, interpolation=interp, batch_size=bs)


def _get(d, *keys, default=None):
    for k in keys:
        try:
            d = d[k]
        except (KeyError, TypeError):
            return default
    return d


# ------------------------------------------------------------------------------------------------ Pillow's tables
def _filter(name: str, x: np.ndarray) -> np.ndarray:
    """Resample.c bicubic_filter (a = -0.5) / bilinear_filter, in double, operation for operation."""
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _coeffs_range(in_size: int, out_size: int, filt: str, lo: int, hi: int):
    """Rows lo..hi-1 of pil_coeffs (Resample.c precompute_coeffs + normalize_coeffs_8bpc)."""
    if filt not in FILTER_SUPPORT:
        raise ValueError(f"interpolation {filt!r} is unknown, expected bicubic or bilinear")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = FILTER_SUPPORT[filt] * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    centre = (np.arange(lo, hi, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((centre - support + 0.5).astype(np.int64), 0)              # (int) truncates toward zero, as astype does
    xmax = np.minimum((centre + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    k = np.arange(ksize, dtype=np.int64)[None, :]
    live = k < count[:, None]
    w = np.where(live, _filter(filt, ((k + xmin[:, None]).astype(np.float64) - centre[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(hi - lo, dtype=np.float64)
    for j in range(ksize):                                                        # the C loop's order of additions
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    return np.where(live, kk, 0).astype(np.int32), xmin.astype(np.int32), count.astype(np.int32)


def pil_coeffs(in_size: int, out_size: int, filt: str = "bicubic"):
    """Pillow's 8-bit resampling tables of one axis: (int32 coefficients [out_size, ksize], xmin [out_size], count [out_size]).
    Centre (xx + 0.5) * in / out, support filter_support * max(in / out, 1), bounds int(centre -+ support + 0.5) clipped to the image,
    weights normalised in double and rounded to int(+-0.5 + k * 2^22)."""
    return _coeffs_range(in_size, out_size, filt, 0, out_size)


# ------------------------------------------------------------------------------------------------ the plan
class CropRecord(NamedTuple):
    path: str
    H: int                       # source size, from the header
    W: int
    scale: Optional[float]       # None without resize_range
    h: int                       # size after the resize (= source size without)
    w: int
    pad: bool                    # a side is shorter than the crop: reflect-padded bottom / right, produced on the host
    y0: int                      # crop origin in the resized (and padded) image
    x0: int
    flip: bool
    interpolation: str


class Window(NamedTuple):
    """What one crop reads of its source image: rows r0..r1-1, columns c0..c1-1, and per axis None ("copy": the resize leaves the
    axis unchanged, the rectangle is the crop itself) or (coefficients [S, ksize], xmin [S], count [S]) relative to the rectangle."""
    r0: int
    r1: int
    c0: int
    c1: int
    tab_x: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]
    tab_y: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]


def _axis_window(in_size: int, out_size: int, filt: str, o0: int, S: int):
    if in_size == out_size:
        return o0, o0 + S, None
    kk, xmin, count = _coeffs_range(in_size, out_size, filt, o0, o0 + S)
    lo, hi = int(xmin.min()), int((xmin + count).max())
    kk = np.ascontiguousarray(kk[:, :max(1, int(count.max()))])       # the table's pitch: the most taps any of these outputs has
    return lo, hi, (kk, (xmin - lo).astype(np.int32), count)


def window(rec: CropRecord, size: int) -> Window:
    """The source rectangle that the crop's `size` output rows and columns read, with the tables shifted to its origin.  Resampling
    that rectangle with the tables equals cropping Pillow's resize of the whole image.  Not for pad records."""
    if rec.pad:
        raise ValueError(f"{rec.path}: a padded record has no source window (it is produced on the host)")
    r0, r1, ty = _axis_window(rec.H, rec.h, rec.interpolation, rec.y0, size)
    c0, c1, tx = _axis_window(rec.W, rec.w, rec.interpolation, rec.x0, size)
    return Window(r0, r1, c0, c1, tx, ty)


class CropPlanner:
    """The crop stream as records: file order and random draws are CropDataset's generator calls (the per-epoch permutation, including
    that every epoch after the first uses the same one; then per image randint y0, randint x0, rand() < 0.5).  With `resize_range`
    = (f_min, f_max) one draw comes first per image, scale = rng.uniform(scale_low, scale_high) with scale_low = max(size / min(H, W),
    f_min), scale_high = max(scale_low, f_max), and the resized size is (int(W * scale), int(H * scale)) (data_transform.py:54-73).
    Image sizes come from the header alone."""

    def __init__(self, paths: Sequence[str], size: int, rank: int, world: int, seed: int, resize_range=None, interpolation: str = "bicubic"):
        self.paths = list(paths)
        if not self.paths:
            raise ValueError("the image list is empty")
        if interpolation not in FILTER_SUPPORT:
            raise ValueError(f"interpolation {interpolation!r} is unknown, expected bicubic or bilinear")
        if resize_range is not None:
            f_min, f_max = float(resize_range[0]), float(resize_range[1])
            if not (0.0 < f_min <= f_max):
                raise ValueError(f"resize_range {resize_range!r} needs 0 < f_min <= f_max")
            resize_range = (f_min, f_max)
        self.size, self.rank, self.world = int(size), rank, world
        self.resize_range, self.interpolation = resize_range, interpolation
        self.rng = np.random.RandomState(seed * 1000 + rank)
        self.order: List[int] = []
        self.pos = 0
        self._sizes = {}

    def _next_path(self) -> str:
        if self.pos >= len(self.order):
            perm = np.random.RandomState(len(self.order) + 17).permutation(len(self.paths))     # same permutation on every rank
            self.order = [int(i) for i in perm[self.rank::self.world]] or [int(perm[0])]
            self.pos = 0
        p = self.paths[self.order[self.pos]]
        self.pos += 1
        return p

    def _header_size(self, path: str) -> Tuple[int, int]:
        hw = self._sizes.get(path)
        if hw is None:
            from PIL import Image
            try:
                with Image.open(path) as im:
                    W, H = im.size
            except Exception as e:
                raise RuntimeError(f"{path}: cannot read the image header ({type(e).__name__}: {e})") from e
            hw = self._sizes[path] = (int(H), int(W))
        return hw

    def next(self) -> CropRecord:
        path = self._next_path()
        H, W = self._header_size(path)
        S = self.size
        scale, h, w = None, H, W
        if self.resize_range is not None:
            scale_low = max(float(S) / float(min(H, W)), self.resize_range[0])
            scale_high = max(scale_low, self.resize_range[1])
            scale = float(self.rng.uniform(scale_low, scale_high))
            w, h = int(W * scale), int(H * scale)
        pad = h < S or w < S
        hp, wp = max(h, S), max(w, S)
        y0, x0 = int(self.rng.randint(0, hp - S + 1)), int(self.rng.randint(0, wp - S + 1))
        flip = bool(self.rng.rand() < 0.5)
        return CropRecord(path, H, W, scale, h, w, pad, y0, x0, flip, self.interpolation)

    def take(self, n: int) -> List[CropRecord]:
        return [self.next() for _ in range(n)]

    def skip(self, n_images: int) -> None:
        """Advance the stream by n_images records (header reads alone; nothing is decoded)."""
        for _ in range(n_images):
            self.next()



# ------------------------------------------------------------------------------------------------ host production
_PIL_FILTER = {"bicubic": "BICUBIC", "bilinear": "BILINEAR"}


def _decode(path: str):
    from PIL import Image
    try:
        with Image.open(path) as im:
            return im.convert("RGB")
    except Exception as e:
        raise RuntimeError(f"{path}: cannot decode ({type(e).__name__}: {e})") from e


def host_crop_u8(rec: CropRecord, size: int) -> np.ndarray:
    """The record's crop before the flip, uint8 [size, size, 3], by Pillow's own resize, np.pad reflect (bottom and right) and a slice:
    what the reference's transform and CropDataset compute."""
    from PIL import Image
    im = _decode(rec.path)
    if (im.size[1], im.size[0]) != (rec.H, rec.W):
        raise RuntimeError(f"{rec.path}: decoded size {im.size[1]} x {im.size[0]} differs from its header's {rec.H} x {rec.W}")
    if rec.scale is not None:
        im = im.resize((rec.w, rec.h), getattr(Image, _PIL_FILTER[rec.interpolation]))
    a = np.asarray(im, dtype=np.uint8)
    H, W = a.shape[:2]
    if H < size or W < size:        # RandomCrop(pad_if_needed, padding_mode='reflect')
        a = np.pad(a, ((0, max(0, size - H)), (0, max(0, size - W)), (0, 0)), mode="reflect")
    return a[rec.y0:rec.y0 + size, rec.x0:rec.x0 + size]


def window_pixels_u8(rec: CropRecord, win: Window) -> np.ndarray:
    """The record's source window, uint8 [r1 - r0, c1 - c0, 3], decoded and cut (a worker thread's share)."""
    im = _decode(rec.path)
    if (im.size[1], im.size[0]) != (rec.H, rec.W):
        raise RuntimeError(f"{rec.path}: decoded size {im.size[1]} x {im.size[0]} differs from its header's {rec.H} x {rec.W}")
    return np.asarray(im.crop((win.c0, win.r0, win.c1, win.r1)), dtype=np.uint8)


def conversion_table() -> torch.Tensor:
    """uint8 -> [-1, 1] as the 256 fp32 values of the project's expression (io_pipeline.u8_to_model_range)."""
    return (torch.arange(256).float().div(255.0) - 0.5) / 0.5


class HostFeed:
    """The stream served serially on the host: Pillow's resize, pad, crop, flip, conversion.  Without resize its batches equal
    CropDataset.batch bit for bit.  batch(n) returns a CPU tensor [n, 3, size, size]."""

    def __init__(self, paths, size: int, rank: int, world: int, seed: int, resize_range=None, interpolation: str = "bicubic"):
        self.plan = CropPlanner(paths, size, rank, world, seed, resize_range, interpolation)
        self.size = int(size)

    def skip(self, n_images: int) -> None:
        self.plan.skip(n_images)

    def batch(self, n: int) -> torch.Tensor:
        out = torch.empty((n, 3, self.size, self.size), dtype=torch.float32)
        for i, rec in enumerate(self.plan.take(n)):
            c = host_crop_u8(rec, self.size)
            if rec.flip:
                c = c[:, ::-1]
            out[i] = (torch.from_numpy(c.copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5
        return out

    def close(self) -> None:
        pass


# ------------------------------------------------------------------------------------------------ the slab
def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class SlabItem(NamedTuple):
    src_off: int
    tab_x: int
    tab_y: int
    src_h: int
    src_w: int
    kx: int
    ky: int


def slab_layout(wins: Sequence[Window], size: int) -> Tuple[List[SlabItem], int]:
    """Byte offsets of a batch in one slab: the descriptor array first, then per image its x tables, y tables (coefficients [S][k],
    xmin [S], count [S], int32) and its pixels (rows of 3 * width bytes), each 16-byte aligned.  -> (items, bytes used)."""
    off = _align(len(wins) * DESC_DTYPE.itemsize)
    items = []
    for wn in wins:
        kx = 0 if wn.tab_x is None else int(wn.tab_x[0].shape[1])
        ky = 0 if wn.tab_y is None else int(wn.tab_y[0].shape[1])
        tx, off = off, off + _align(4 * size * (kx + 2) if kx else 0)
        ty, off = off, off + _align(4 * size * (ky + 2) if ky else 0)
        sh, sw = wn.r1 - wn.r0, wn.c1 - wn.c0
        items.append(SlabItem(off, tx, ty, sh, sw, kx, ky))
        off += _align(sh * sw * 3)
    return items, off


def slab_capacity(n: int, size: int, resize_range, interpolation: str) -> int:
    """Bytes a slab needs for any batch of n records of the plan (scale >= max(f_min, the threaded limit))."""
    if resize_range is None:
        side, k = size, 0
    else:
        f = min(max(float(resize_range[0]), MIN_THREADED_SCALE), 1.0)
        fs = FILTER_SUPPORT[interpolation]
        side = int((size - 1 + 2 * fs) / f * 1.02) + 8           # int(W * scale) / W falls short of scale by up to 1 / W
        k = MAX_KSIZE
    per = 2 * _align(4 * size * (k + 2)) + _align(side * side * 3)
    return _align(n * DESC_DTYPE.itemsize) + n * per


def write_tables(buf: np.ndarray, item: SlabItem, win: Window) -> None:
    """An image's tables into the slab (a uint8 numpy view): per resampled axis coefficients, then xmin, then count."""
    for off, tab in ((item.tab_x, win.tab_x), (item.tab_y, win.tab_y)):
        if tab is not None:
            kk, xmin, count = tab
            n = kk.size
            v = buf[off:off + 4 * (n + 2 * len(xmin))].view(np.int32)
            v[:n] = kk.reshape(-1)
            v[n:n + len(xmin)] = xmin
            v[n + len(xmin):] = count


def write_desc(buf: np.ndarray, i: int, item: SlabItem, flip: bool) -> None:
    d = buf[i * DESC_DTYPE.itemsize:(i + 1) * DESC_DTYPE.itemsize].view(DESC_DTYPE)
    d[0] = (item.src_off, item.tab_x, item.tab_y, item.src_h, item.src_w, item.src_w * 3, 1 if flip else 0, item.kx, item.ky)


def write_pixels(buf: np.ndarray, item: SlabItem, pixels: np.ndarray) -> None:
    if pixels.shape != (item.src_h, item.src_w, 3) or pixels.dtype != np.uint8:
        raise ValueError(f"window pixels {pixels.shape} {pixels.dtype}, the slab expects ({item.src_h}, {item.src_w}, 3) uint8")
    buf[item.src_off:item.src_off + pixels.size].reshape(pixels.shape)[...] = pixels


def pack_batch(buf: np.ndarray, entries: Sequence[Tuple[np.ndarray, Window, bool]], size: int) -> int:
    """Pack (window pixels, window, flip) entries into `buf` (uint8, C-contiguous) -> bytes used.  The serial form of what the feed's
    workers do, for tests and tools."""
    items, used = slab_layout([e[1] for e in entries], size)
    if used > buf.size:
        raise ValueError(f"the batch needs {used} bytes, the slab holds {buf.size}")
    for i, ((px, wn, flip), item) in enumerate(zip(entries, items)):
        write_desc(buf, i, item, flip)
        write_tables(buf, item, wn)
        write_pixels(buf, item, px)
    return used


# ------------------------------------------------------------------------------------------------ the threaded feed
class _Job:
    def __init__(self, slab: int, n: int):
        self.slab, self.n, self.left = slab, n, n
        self.lock = threading.Lock()
        self.done = threading.Event()
        self.error: Optional[BaseException] = None
        self.out: Optional[torch.Tensor] = None
        self.event = None
        self.used = 0


class TrainFeed:
    """The stream served ahead of the trainer: the planner runs in order on the caller's thread, `workers` threads decode each image
    and write its source window (without resize: its crop) into a pinned slab of a ring of depth + 1, the last worker of a batch
    enqueues one host-to-device copy and the one launch on the feed's own stream, and batch(n) makes the current stream wait on that
    batch's event and returns the device tensor [n, 3, size, size].  Pad records are produced on the host and enter the slab as plain
    crops.  A worker's exception is re-raised by batch() with the path in its message.  No process is started."""

    def __init__(self, paths, size: int, rank: int, world: int, seed: int, device, workers: Optional[int] = None, depth: int = 2,
                 resize_range=None, interpolation: str = "bicubic"):
        from ..io_pipeline import default_workers
        self.plan = CropPlanner(paths, size, rank, world, seed, resize_range, interpolation)
        if resize_range is not None and float(resize_range[0]) < MIN_THREADED_SCALE:
            raise ValueError(f"resize_range {list(resize_range)!r} has f_min < {MIN_THREADED_SCALE}, past the threaded feed's {MAX_KSIZE} taps "
                             "per output; HostFeed serves it")
        self.size = int(size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"TrainFeed needs a GPU device, got {device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.workers = int(workers) if workers else default_workers()
        self.depth = max(1, int(depth))
        self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="dcvic-train-dec")
        self.stream = torch.cuda.Stream(device=self.device)
        self.table = conversion_table().to(self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))      # the table's copy was enqueued on the caller's stream
        self.n: Optional[int] = None
        self.pinned: List[torch.Tensor] = []
        self.dev: List[torch.Tensor] = []
        self.copied: List[Optional[torch.cuda.Event]] = []
        self.jobs: List[_Job] = []
        self.seq = 0
        self.closed = False

    def skip(self, n_images: int) -> None:
        if self.jobs:
            raise RuntimeError("skip() after the first batch(): the stream is already being produced ahead")
        self.plan.skip(n_images)

    # -- producer side
    def _allocate(self, n: int) -> None:
        cap = slab_capacity(n, self.size, self.plan.resize_range, self.plan.interpolation)
        for _ in range(self.depth + 1):
            self.pinned.append(torch.empty(cap, dtype=torch.uint8, pin_memory=True))
            self.dev.append(torch.empty(cap, dtype=torch.uint8, device=self.device))
            self.copied.append(None)
        self.n = n

    def _schedule(self) -> None:
        n, S = self.n, self.size
        recs = self.plan.take(n)
        wins = [Window(0, S, 0, S, None, None) if r.pad else window(r, S) for r in recs]
        items, used = slab_layout(wins, S)
        slab = self.seq % (self.depth + 1)
        self.seq += 1
        if used > self.pinned[slab].numel():
            raise RuntimeError(f"a batch needs {used} bytes, the slab holds {self.pinned[slab].numel()}")
        if self.copied[slab] is not None:
            self.copied[slab].synchronize()                # the slab's previous copy has left the pinned memory
        buf = self.pinned[slab].numpy()
        job = _Job(slab, n)
        job.used = used
        for i, (r, wn, it) in enumerate(zip(recs, wins, items)):
            write_desc(buf, i, it, r.flip)
            write_tables(buf, it, wn)
        self.jobs.append(job)
        for r, wn, it in zip(recs, wins, items):
            self.pool.submit(self._work, job, buf, r, wn, it)

    def _work(self, job: _Job, buf: np.ndarray, rec: CropRecord, win: Window, item: SlabItem) -> None:
        try:
            if not self.closed and job.error is None:
                write_pixels(buf, item, host_crop_u8(rec, self.size) if rec.pad else window_pixels_u8(rec, win))
        except BaseException as e:                                   # noqa: BLE001  (handed to batch())
            with job.lock:
                if job.error is None:
                    job.error = e if rec.path in str(e) else RuntimeError(f"{rec.path}: {type(e).__name__}: {e}")
        with job.lock:
            job.left -= 1
            last = job.left == 0
        if last:
            try:
                if job.error is None and not self.closed:
                    self._launch(job)
            except BaseException as e:                               # noqa: BLE001
                job.error = e
            finally:
                job.done.set()

    def _launch(self, job: _Job) -> None:
        from . import kernels as K
        pinned, dev = self.pinned[job.slab], self.dev[job.slab]
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            dev[:job.used].copy_(pinned[:job.used], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
            self.copied[job.slab] = ev
            job.out = torch.empty((job.n, 3, self.size, self.size), dtype=torch.float32, device=self.device)
            K.u8_resample_crop(dev, job.used, pinned.data_ptr(), job.n, self.size, self.table, job.out, stream=self.stream.cuda_stream)
            job.event = torch.cuda.Event()
            job.event.record(self.stream)

    # -- consumer side
    def batch(self, n: int) -> torch.Tensor:
        if self.closed:
            raise RuntimeError("TrainFeed.batch() after close()")
        if self.n is None:
            self._allocate(int(n))
        elif n != self.n:
            raise ValueError(f"TrainFeed was started with batches of {self.n}, batch({n}) would break the stream produced ahead")
        while len(self.jobs) < self.depth:
            self._schedule()
        job = self.jobs.pop(0)
        job.done.wait()
        if job.error is not None:
            raise job.error
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(job.event)
        job.out.record_stream(cur)
        self._schedule()
        return job.out

    def close(self) -> None:
        """Joins the worker threads (work not yet started is dropped) and drains the feed's stream."""
        if self.closed:
            return
        self.closed = True
        self.pool.shutdown(wait=True, cancel_futures=True)
        self.jobs = []
        self.stream.synchronize()
