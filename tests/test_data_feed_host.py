"""The training data feed without a GPU (dc_vic_amd/train/data.py): the restatement of Pillow's 8-bit resampling against PIL.Image.resize,
the window form against resize-then-crop, the planned stream against scripts/train.py's CropDataset, the YAML section's reading, the
listing, include/dcvic_data.h against _lib.DATA_SIGNATURES and the entry point's argument checks.  Every comparison is exact."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import data_feed_ref as R
import test_cabi
from dc_vic_amd import _lib
from dc_vic_amd.train import data as D
from test_focal_host import loss_header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("dcvic_train_cli_data_feed", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------- Pillow restated
SIZES = ((64, 48), (100, 161), (257, 300), (512, 768))
SCALES = (0.5, 0.61, 0.75, 1.0, 1.3, 2.0, "min")           # "min": the minimum factor 256 / min(H, W) of the reference's transform


def _scale(s, H, W):
    return 256.0 / min(H, W) if s == "min" else s


@pytest.mark.parametrize("filt", ("bicubic", "bilinear"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow(size, filt):
    H, W = size
    for s in SCALES:
        w, h = int(W * _scale(s, H, W)), int(H * _scale(s, H, W))
        if max(w, h) > 1600:                    # the minimum factor of the smallest image is 5.3: its 64 x 48 case is kept, nothing larger
            continue
        for content in ("noise", "ramp", "steps"):
            a = R.CONTENT[content](H, W)
            assert np.array_equal(R.pil_resize_u8(a, w, h, filt), R.pil_resize(a, w, h, filt)), (size, s, filt, content)


def test_clip_acts_on_the_step_pattern():
    """Bicubic overshoot: without the clip the step pattern's sums leave [0, 255] (so the exact match above tests the clip)."""
    a = R.steps(60, 45)
    kk, xmin, count = D.pil_coeffs(45, 58, "bicubic")
    acc = np.array([[int(np.dot(kk[i, :count[i]].astype(np.int64), a[r, xmin[i]:xmin[i] + count[i], 0].astype(np.int64)) + (1 << 21)) >> 22
                     for i in range(58)] for r in range(60)])
    assert acc.min() < 0 and acc.max() > 255


def test_one_axis_only():
    """3 wide at scale 1.2: int(3 * 1.2) = 3, Pillow skips the horizontal pass; the window form marks the axis "copy"."""
    a = R.noise(40, 3, 5)
    for filt in ("bicubic", "bilinear"):
        assert np.array_equal(R.pil_resize_u8(a, 3, 48, filt), R.pil_resize(a, 3, 48, filt))
        rec = R.record(40, 3, 1.2, filt, 3, 20, 0, False)
        win = D.window(rec, 3)
        assert win.tab_x is None and win.tab_y is not None and (win.c0, win.c1) == (0, 3)
        assert np.array_equal(R.resample_window_u8(a[win.r0:win.r1, win.c0:win.c1], win), R.pillow_crop(a, rec, 3))


def test_coefficient_tables():
    kk, xmin, count = D.pil_coeffs(400, 100, "bicubic")         # scale 1/4: support 8, ksize 17, centres at 4 xx + 2: 16 taps
    assert kk.shape == (100, 17) and kk.dtype == np.int32 and count.max() == 16 and (xmin + count).max() == 400 and xmin.min() == 0
    kk19, _, count19 = D.pil_coeffs(401, 100, "bicubic")        # int(W * 0.25) / W just under 1/4: Pillow's pitch is 19, the taps stay <= 17
    assert kk19.shape == (100, 19) and count19.max() == 17 and not kk19[:, 17:].any()
    assert np.all(np.abs(kk.sum(axis=1) - (1 << 22)) <= 17)      # each weight is rounded once
    kk, xmin, count = D.pil_coeffs(100, 200, "bilinear")        # upscaling: support 1, ksize 3
    assert kk.shape == (200, 3) and count.max() <= 3
    with pytest.raises(ValueError, match="lanczos"):
        D.pil_coeffs(10, 20, "lanczos")


@pytest.mark.parametrize("scale,filt", ((0.37, "bicubic"), (1.3, "bicubic"), (0.25, "bicubic"), (0.61, "bilinear"), (2.0, "bilinear")))
def test_window_form_equals_resize_then_crop(scale, filt):
    H, W, S = 300, 424, 37
    a = R.noise(H, W, 11)
    h, w = int(H * scale), int(W * scale)
    full = R.pil_resize(a, w, h, filt)
    for name in R.POSITIONS:
        y0, x0 = R.position(name, h, w, S)
        rec = R.record(H, W, scale, filt, S, y0, x0, False)
        win = D.window(rec, S)
        assert 0 <= win.r0 < win.r1 <= H and 0 <= win.c0 < win.c1 <= W
        for tab, ext in ((win.tab_x, win.c1 - win.c0), (win.tab_y, win.r1 - win.r0)):
            kk, xmin, count = tab
            assert kk.shape[1] <= D.MAX_KSIZE and xmin.min() == 0 and (xmin + count).max() == ext
        assert np.array_equal(R.resample_window_u8(a[win.r0:win.r1, win.c0:win.c1], win), full[y0:y0 + S, x0:x0 + S]), name
    # the whole image as one window
    S2 = min(h, w)
    sq = R.noise(120, 120, 3)
    hs = int(120 * scale)
    rec = R.record(120, 120, scale, filt, hs, 0, 0, False)
    win = D.window(rec, hs)
    assert (win.r0, win.r1, win.c0, win.c1) == (0, 120, 0, 120) and S2 > 0
    assert np.array_equal(R.resample_window_u8(sq, win), R.pil_resize(sq, hs, hs, filt))


# ---------------------------------------------------------------------------------------------------- the stream
S_FEED = 48


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("feed")
    return str(root), R.write_folder(str(root), S_FEED)


def test_host_feed_equals_crop_dataset(cli, folder):
    """4 batches of 3 from 5 files: crosses an epoch boundary; JPEG and PNG mixed; one file smaller than the crop."""
    root, paths = folder
    assert D.list_train_images(root) == paths == cli.CropDataset(root, S_FEED, 0, 1, 3).paths
    for rank, world in ((0, 1), (1, 2)):
        old, new = cli.CropDataset(root, S_FEED, rank, world, 3), D.HostFeed(paths, S_FEED, rank, world, 3)
        for _ in range(4):
            assert torch.equal(new.batch(3), old.batch(3))


def test_planner_records_and_skip(folder):
    _, paths = folder
    for kw in (dict(), dict(resize_range=(0.5, 1.0)), dict(resize_range=(0.7, 0.7), interpolation="bilinear")):
        whole = D.CropPlanner(paths, S_FEED, 0, 1, 9, **kw).take(14)
        again = D.CropPlanner(paths, S_FEED, 0, 1, 9, **kw).take(14)
        assert whole == again
        for k in (0, 1, 5, 6, 11):
            p = D.CropPlanner(paths, S_FEED, 0, 1, 9, **kw)
            p.skip(k)
            assert p.take(14 - k) == whole[k:], (kw, k)
        for r in whole:
            assert (r.scale is None) == (not kw) and r.interpolation == kw.get("interpolation", "bicubic")
            assert r.pad == (r.h < S_FEED or r.w < S_FEED)
            assert 0 <= r.y0 <= max(r.h, S_FEED) - S_FEED and 0 <= r.x0 <= max(r.w, S_FEED) - S_FEED
            if r.scale is not None:
                assert (r.w, r.h) == (int(r.W * r.scale), int(r.H * r.scale))
                assert r.scale >= max(S_FEED / min(r.H, r.W), kw["resize_range"][0])
    # without resize no extra draw is made: the records' draws are CropDataset's
    plain = D.CropPlanner(paths, S_FEED, 0, 1, 9).take(3)
    rng = np.random.RandomState(9 * 1000)
    for r in plain:
        hp, wp = max(r.H, S_FEED), max(r.W, S_FEED)
        assert (r.y0, r.x0, r.flip) == (rng.randint(0, hp - S_FEED + 1), rng.randint(0, wp - S_FEED + 1), bool(rng.rand() < 0.5))


def test_host_feed_with_resize_is_the_reference_transform(folder):
    """HostFeed with resize_range against the transform written out with Pillow: resize, reflect pad, crop, flip, conversion."""
    from PIL import Image
    _, paths = folder
    recs = D.CropPlanner(paths, S_FEED, 0, 1, 4, resize_range=(0.5, 1.0)).take(6)
    got = D.HostFeed(paths, S_FEED, 0, 1, 4, resize_range=(0.5, 1.0)).batch(6)
    assert any(r.pad for r in recs) and any(not r.pad for r in recs)
    for i, r in enumerate(recs):
        a = np.asarray(Image.open(r.path).convert("RGB").resize((r.w, r.h), Image.BICUBIC))
        a = np.pad(a, ((0, max(0, S_FEED - r.h)), (0, max(0, S_FEED - r.w)), (0, 0)), mode="reflect")
        c = a[r.y0:r.y0 + S_FEED, r.x0:r.x0 + S_FEED]
        assert torch.equal(got[i], R.to_model_range(c[:, ::-1] if r.flip else c)), r


def test_pad_case_at_the_minimum_factor(tmp_path):
    """Crop 256, shortest side 322: int(322 * (256 / 322)) = 255, one short of the crop; the plan pads as CropDataset pads."""
    from PIL import Image
    assert int(322 * (256.0 / 322.0)) == 255 and R.pad_side(256, 257, 400) <= 322
    assert sum(int(s * (256.0 / s)) == 255 for s in range(257, 3000)) == 272
    a = R.noise(340, 322, 1)
    Image.fromarray(a).save(tmp_path / "p.png")
    paths = [str(tmp_path / "p.png")]
    rec = D.CropPlanner(paths, 256, 0, 1, 0, resize_range=(0.1, 0.1)).next()
    assert rec.scale == 256.0 / 322.0 and (rec.h, rec.w) == (int(340 * rec.scale), 255) and rec.pad and rec.x0 == 0
    with pytest.raises(ValueError, match="padded"):
        D.window(rec, 256)
    got = D.HostFeed(paths, 256, 0, 1, 0, resize_range=(0.1, 0.1)).batch(1)[0]
    r = np.pad(R.pil_resize(a, rec.w, rec.h, "bicubic"), ((0, 0), (0, 1), (0, 0)), mode="reflect")[rec.y0:rec.y0 + 256]
    assert torch.equal(got, R.to_model_range(r[:, ::-1] if rec.flip else r))


# ---------------------------------------------------------------------------------------------------- listing and the YAML section
def test_subset_listing(tmp_path):
    from PIL import Image
    for k, names in ((0, ("b.jpg", "a.jpg")), (3, ("0.jpg", "z.png"))):
        os.makedirs(tmp_path / f"train_{k}")
        for n in names:
            Image.fromarray(R.noise(8, 8, 0)).save(tmp_path / f"train_{k}" / n)
    got = D.list_train_images(str(tmp_path), [3, 0])
    assert got == sorted(str(tmp_path / d / n) for d, n in (("train_0", "a.jpg"), ("train_0", "b.jpg"), ("train_3", "0.jpg")))
    assert D.list_train_images(str(tmp_path)) == []                   # flat: no image at the top level
    with pytest.raises(ValueError, match="train_7"):
        D.list_train_images(str(tmp_path), [0, 7])


REFERENCE_SECTION = dict(batch_size=6, train_dataset=dict(name="openimage", type="ImageDataset", image_size=256, resize_range=None,
                                                           root_dir="../datasets/openimage", subset_list=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9]),
                         eval_dataset=dict(name="Kodak", type="ImageDataset", root_dir="../datasets/kodak"))


def _opt(**train):
    return dict(dataset=dict(REFERENCE_SECTION, train_dataset=dict(REFERENCE_SECTION["train_dataset"], **train)))


def test_read_train_dataset():
    assert D.read_train_dataset(dict(dataset=REFERENCE_SECTION)) == dict(
        root_dir="../datasets/openimage", subset_list=list(range(10)), image_size=256, resize_range=None, interpolation="bicubic", batch_size=6)
    assert D.read_train_dataset({}) == dict(root_dir=None, subset_list=None, image_size=256, resize_range=None, interpolation="bicubic", batch_size=None)
    got = D.read_train_dataset(_opt(resize_range=[0.5, 1.0], interpolation="bilinear"))
    assert got["resize_range"] == (0.5, 1.0) and got["interpolation"] == "bilinear"
    for train, words in ((dict(image_size=128), r"image_size: 128"), (dict(interpolation="lanczos"), r"interpolation: 'lanczos'"),
                         (dict(resize_range=[0.0, 1.0]), r"resize_range: \[0.0, 1.0\]"), (dict(resize_range=[-0.5, 1.0]), r"resize_range: \[-0.5, 1.0\]"),
                         (dict(resize_range=[0.8, 0.5]), r"resize_range: \[0.8, 0.5\]"), (dict(resize_range=[0.2, 1.0]), r"resize_range: \[0.2, 1.0\].*--data_workers 0"),
                         (dict(resize_range=0.5), r"resize_range: 0.5"), (dict(subset_list="all"), r"subset_list: 'all'"),
                         (dict(mirror=True), r"mirror: True")):
        with pytest.raises(ValueError, match=r"dataset\.train_dataset\." + words):
            D.read_train_dataset(_opt(**train))
    assert D.read_train_dataset(_opt(resize_range=[0.2, 1.0]), threaded=False)["resize_range"] == (0.2, 1.0)      # the host path serves it


def test_cli_listing_rules(cli, folder, tmp_path):
    """list_training_set: flat --dataset_root, the train_{k} layout, the YAML's root_dir, and the refusals, all without a GPU."""
    import argparse
    root, paths = folder
    a = argparse.Namespace(synthetic_data=False, dataset_root=root, data_workers=None, data_depth=2, batch_size=8, seed=0)
    got = cli.list_training_set(a, {})
    assert got["paths"] == paths and got["layout"] == "flat"
    assert cli.list_training_set(argparse.Namespace(**dict(vars(a), synthetic_data=True)), {}) is None
    from PIL import Image
    os.makedirs(tmp_path / "oi" / "train_1")
    Image.fromarray(R.noise(8, 8, 0)).save(tmp_path / "oi" / "train_1" / "x.jpg")
    opt = _opt(root_dir=str(tmp_path / "oi"), subset_list=[1])
    for ns in (dict(dataset_root=str(tmp_path / "oi")), dict(dataset_root=None)):
        got = cli.list_training_set(argparse.Namespace(**dict(vars(a), **ns)), opt)
        assert got["layout"] == "subsets" and got["paths"] == [str(tmp_path / "oi" / "train_1" / "x.jpg")]
    for ns, o, words in ((dict(dataset_root=None), {}, "--dataset_root"), (dict(dataset_root=str(tmp_path / "none")), {}, "none"),
                         (dict(dataset_root=None), _opt(root_dir=str(tmp_path / "oi"), subset_list=[1, 2]), "train_2"),
                         (dict(dataset_root=str(tmp_path)), {}, "holds no image"), (dict(), _opt(image_size=64), "image_size: 64"),
                         (dict(), _opt(resize_range=[0.1, 1.0]), "--data_workers 0")):
        with pytest.raises(SystemExit, match=words):
            cli.list_training_set(argparse.Namespace(**dict(vars(a), **ns)), o)
    # --data_workers 0: the host feed, from the same wiring, equals CropDataset
    feed, line = cli.build_train_data(argparse.Namespace(**dict(vars(a), data_workers=0, seed=2)), _opt(), 0, 1, "cpu")
    assert isinstance(feed, D.HostFeed) and line.startswith("data: 5 images") and "resize off" in line and "dataset.batch_size 6" in line
    assert torch.equal(feed.batch(2)[:, :, :8, :8], cli.CropDataset(root, 256, 0, 1, 2).batch(2)[:, :, :8, :8])


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_data_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_data.h"))
    P, I, Q = C.c_void_p, C.c_int, C.c_longlong
    assert protos == {"dcvic_u8_resample_crop_f32": (I, [P, Q, P, P, I, I, P, P, P])}
    assert test_cabi.signature_mismatches(_lib.DATA_SIGNATURES, protos) == []
    others, tables = set(), set()
    for h in ("dcvic.h", "dcvic_loss.h", "dcvic_rate.h", "dcvic_train.h", "dcvic_vq.h", "dcvic_sample_loss.h", "dcvic_gumbel.h", "dcvic_msssim_loss.h"):
        others |= set(loss_header_prototypes(os.path.join(ROOT, "include", h)))
    for t in (_lib.SIGNATURES, _lib.LOSS_SIGNATURES, _lib.RATE_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.VQ_SIGNATURES, _lib.SAMPLE_LOSS_SIGNATURES,
              _lib.GUMBEL_SIGNATURES, _lib.MSSSIM_LOSS_SIGNATURES):
        tables |= set(t)
    assert not set(protos) & others and not set(_lib.DATA_SIGNATURES) & tables
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert test_cabi.signature_mismatches(dict(_lib.DATA_SIGNATURES, dcvic_u8_resample_crop_f32="i:pippiippp"), protos) != []
    assert D.DESC_DTYPE.itemsize == 48 and _lib.DATA_MAX_KSIZE == D.MAX_KSIZE == 17
    txt = open(os.path.join(ROOT, "include", "dcvic_data.h")).read()
    assert "#define DCVIC_DATA_MAX_KSIZE 17" in txt


FAKE = 256                      # non-null and aligned, never dereferenced: every refusal precedes the launch


def _descs(*rows):
    """Host descriptors (the entry point reads these): rows of (src_off, tab_x, tab_y, src_h, src_w, src_stride, flip, kx, ky)."""
    d = np.zeros(len(rows), dtype=D.DESC_DTYPE)
    for i, r in enumerate(rows):
        d[i] = r
    return d


def _call(d, slab=FAKE, slab_bytes=1 << 20, desc_dev=FAKE, N=None, S=16, table=FAKE, out=FAKE, host=True):
    return _lib.lib().dcvic_u8_resample_crop_f32(slab, slab_bytes, desc_dev, d.ctypes.data if host else None, len(d) if N is None else N, S, table, out, None)


def check_refusals():
    """Every refusal returns DCVIC_EINVAL with "u8_resample_crop:" in front (shared with the GPU test file)."""
    L = _lib.lib()
    ok = (1024, 0, 0, 16, 16, 48, 0, 0, 0)              # a plain 16 x 16 crop, both axes "copy"
    tabs = (4096, 64, 2048, 20, 20, 60, 1, 5, 5)        # both axes resampled, ksize 5

    def edit(row, **kw):
        names = D.DESC_DTYPE.names
        return tuple(kw.get(n, v) for n, v in zip(names, row))
    cases = [
        (dict(slab=None), ok, "null pointer"), (dict(desc_dev=None), ok, "null pointer"), (dict(host=False), ok, "null pointer"),
        (dict(table=None), ok, "null pointer"), (dict(out=None), ok, "null pointer"),
        (dict(N=0), ok, "empty batch"), (dict(S=0), ok, "empty batch"), (dict(N=-2), ok, "empty batch"),
        (dict(N=65536), ok, "65535"), (dict(S=32769), ok, "S=32769"), (dict(slab=FAKE + 2), ok, "4-byte aligned"), (dict(desc_dev=FAKE + 4), ok, "8-byte aligned"),
        (dict(), edit(tabs, kx=18), "ksize x 18"), (dict(), edit(tabs, ky=-1), "y -1"),
        (dict(), edit(ok, src_off=-1), "window"), (dict(), edit(ok, src_off=(1 << 20) - 16 * 48 + 1), "window"), (dict(), edit(ok, src_stride=47), "window"),
        (dict(), edit(ok, src_h=0), "window"), (dict(), edit(ok, src_off=1 << 40), "window"),
        (dict(), edit(ok, src_w=15, src_stride=45), "copies an axis"), (dict(), edit(tabs, ky=0), "copies an axis"),
        (dict(), edit(tabs, tab_x=66), "x table"), (dict(), edit(tabs, tab_y=(1 << 20) - 4 * 16 * 7 + 4), "y table"), (dict(), edit(tabs, tab_x=-4), "x table"),
    ]
    for kw, row, words in cases:
        assert _call(_descs(ok, row), **kw) == -1, (kw, row)
        msg = L.dcvic_last_error().decode()
        assert msg.startswith("u8_resample_crop:") and words in msg, (msg, words)
    return len(cases)


def test_argument_refusals_without_gpu():
    assert check_refusals() == 24


# ---------------------------------------------------------------------------------------------------- the slab
def test_slab_layout_read_back_equals_pillow():
    """Every kernel case of the GPU tests, packed and read back with the kernel's indexing on the host: the slab's layout, the shifted
    tables and the GPU tests' expectations agree before any launch."""
    for S in sorted({c[0] for c in R.KERNEL_CASES}):
        built = [R.build_case(c) for c in R.KERNEL_CASES if c[0] == S]
        entries = [b[0] for b in built]
        items, used = D.slab_layout([e[1] for e in entries], S)
        buf = np.zeros(used, dtype=np.uint8)
        assert D.pack_batch(buf, entries, S) == used
        assert all(it.src_off % 16 == 0 and it.tab_x % 16 == 0 and it.tab_y % 16 == 0 and it.kx <= D.MAX_KSIZE and it.ky <= D.MAX_KSIZE for it in items)
        got = R.read_slab(buf, len(entries), S)
        for i, (_, want) in enumerate(built):
            assert torch.equal(got[i], want), (S, i)
    assert D.slab_capacity(8, 256, None, "bicubic") >= 8 * 256 * 256 * 3
    with pytest.raises(ValueError, match="slab holds"):
        D.pack_batch(np.zeros(64, dtype=np.uint8), [R.build_case(R.KERNEL_CASES[0])[0]], 3)


def test_conversion_table_is_the_projects_expression():
    from dc_vic_amd.io_pipeline import u8_to_model_range
    u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 256, 1, 1).expand(1, 256, 1, 3).contiguous()
    assert torch.equal(D.conversion_table(), u8_to_model_range(u8)[0, 0, :, 0])
