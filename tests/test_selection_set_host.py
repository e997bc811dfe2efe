"""Stage 2's selection set without a GPU: the builder's crop plan, folder name and refusals (scripts/build_openimage_val_dataset.py),
SelectionSet's host fallback, token validation and residency decision (dc_vic_amd/selection_set.py), include/dcvic_tokens.h against
_lib.TOKEN_SIGNATURES, the entry points' argument checks and the CPU restatements the GPU tests compare with.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

import test_cabi
import tokens_ref as R
from test_focal_host import loss_header_prototypes

import build_openimage_val_dataset as B            # tokens_ref puts scripts/ on sys.path
import binary_rate_search as brs
from dc_vic_amd import _lib
from dc_vic_amd.selection_set import SelectionSet, residency

ROOT = R.ROOT
CONFIG = os.path.join(ROOT, "config", "dc_vic_synthetic.yaml")


# ---------------------------------------------------------------------------------------------------- the crop plan
def test_plan_crops_literal_case():
    paths = [f"/x/validation/{i:04d}.jpg" for i in range(10)]
    sizes = [(300 + 7 * i, 256 + 5 * i) if i % 3 else (200, 400) for i in range(10)]
    plan = B.plan_crops(paths, sizes, seed=0, num_img=4)
    assert [(os.path.basename(p)[:4], t, l) for p, t, l in plan] == [("0002", 6, 48), ("0008", 26, 5), ("0004", 8, 65), ("0001", 3, 25)]


@pytest.mark.parametrize("seed", [0, 3, 11])
def test_plan_crops_equals_the_reference_loop(seed):
    rng = np.random.default_rng(seed)
    n = 23
    paths = sorted(f"/data/validation/{int(v):08x}.jpg" for v in rng.choice(1 << 30, n, replace=False))
    sizes = [(int(rng.integers(200, 700)), int(rng.integers(200, 700))) for _ in range(n)]
    sizes[1], sizes[5], sizes[9] = (400, 256), (256, 256), (255, 600)      # randint(0, 0) still draws; 255 is skipped without a draw
    state = (np.random.get_state()[1].copy(), __import__("random").getstate())
    for num in (1, 7, 100):
        got = B.plan_crops(paths, sizes, seed, num)
        assert (np.random.get_state()[1] == state[0]).all() and __import__("random").getstate() == state[1], "plan_crops touched a global generator"
        want = R.reference_loop(paths, dict(zip(paths, sizes)), seed, num)
        state = (np.random.get_state()[1].copy(), __import__("random").getstate())
        assert got == want, (seed, num)
        assert all(min(sizes[paths.index(p)]) >= 256 for p, _, _ in got)
    eligible = sum(min(s) >= 256 for s in sizes)
    assert len(B.plan_crops(paths, sizes, seed, 100)) == eligible < 100
    # a draw of randint(0, 0) happens: dropping it would shift every later draw
    assert any(sizes[paths.index(p)] == (256, 256) and (t, l) == (0, 0) for p, t, l in B.plan_crops(paths, sizes, seed, 100))


def test_output_folder_name():
    assert B.save_dir_of("./dataset", "f8-n256", 2000, 0) == os.path.join("./dataset", "vq_f8_n256", "crop_256_2000_seed_0")
    assert B.save_dir_of("/d", "f8-n256", 3, 7) == "/d/vq_f8_n256/crop_256_3_seed_7"
    a = B.arg_parser().parse_args(["--vqgan_type", "f8-n256", "--openimage_root", "/o"])
    assert (a.save_root, a.device, a.seed, a.num_img, a.batch_size, a.synthetic_weights) == ("./dataset", "cuda:0", 0, 2000, 16, False)
    assert os.path.samefile(a.config_path, CONFIG)


# ---------------------------------------------------------------------------------------------------- the builder's refusals
def _validation(tmp_path):
    d = tmp_path / "oi" / "validation"
    d.mkdir(parents=True)
    (d / "a.jpg").write_bytes(b"not decoded before the refusals")
    return str(tmp_path / "oi")


@pytest.mark.parametrize("vqgan_type", ["f16", "f8"])
def test_builder_refuses_types_that_are_not_built(tmp_path, vqgan_type):
    with pytest.raises(SystemExit, match=f"--vqgan_type {vqgan_type} is not built.*subnet.vq_model.n_embed.*subnet.vq_model.embed_dim") as e:
        B.main(["--vqgan_type", vqgan_type, "--openimage_root", _validation(tmp_path), "--save_root", str(tmp_path / "out"), "--synthetic_weights"])
    assert "\n" not in str(e.value) and not (tmp_path / "out").exists()


def test_builder_refuses_a_config_that_disagrees(tmp_path):
    cfg = yaml.safe_load(open(CONFIG))
    cfg["subnet"]["vq_model"]["n_embed"] = 1024
    path = tmp_path / "other.yaml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit, match="f8-n256 means subnet.vq_model.n_embed 256 and subnet.vq_model.embed_dim 4, but the config has subnet.vq_model.n_embed 1024"):
        B.main(["--vqgan_type", "f8-n256", "--openimage_root", _validation(tmp_path), "--save_root", str(tmp_path / "out"), "--synthetic_weights",
                "--config_path", str(path)])
    assert not (tmp_path / "out").exists()


def test_builder_refuses_a_missing_validation_folder(tmp_path):
    (tmp_path / "oi").mkdir()
    args = ["--vqgan_type", "f8-n256", "--save_root", str(tmp_path / "out"), "--synthetic_weights", "--openimage_root", str(tmp_path / "oi")]
    with pytest.raises(SystemExit, match="validation is not a folder"):
        B.main(args)
    (tmp_path / "oi" / "validation").mkdir()
    (tmp_path / "oi" / "validation" / "a.png").write_bytes(b"")
    with pytest.raises(SystemExit, match="holds no .jpg"):
        B.main(args)
    assert not (tmp_path / "out").exists()


def test_builder_refuses_a_missing_checkpoint(tmp_path):
    args = ["--vqgan_type", "f8-n256", "--openimage_root", _validation(tmp_path), "--save_root", str(tmp_path / "out")]
    with pytest.raises(SystemExit, match="VQGAN checkpoint None .*does not exist.*--synthetic_weights"):          # the config's ckpt_path: null
        B.main(args)
    with pytest.raises(SystemExit, match="VQGAN checkpoint '.*absent.ckpt' .*does not exist"):
        B.main(args + ["--vqgan_ckpt", str(tmp_path / "absent.ckpt")])
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------------------------- SelectionSet
def test_mixed_folder_equals_load_dataset_plus_batches(tmp_path):
    """Mixed shapes and tokens for some items only (what tests/test_gpu_cli.py feeds the scripts): the host fallback."""
    root = R.make_folder(tmp_path / "mixed", [(64, 64), (64, 64), (64, 64), (128, 64), (128, 64), (64, 64), (100, 72)], tokens={1, 2, 4, 6}, dtype=np.int64)
    s = SelectionSet(root, "cpu", 256)
    assert not s.resident and s.images is None and s.names == [f"{i}.png" for i in range(7)] and len(s) == 7
    before = R.list_before(root)                       # the scripts' functions call the package now: both are held to the restatement
    for items in (s.items, brs.load_dataset(root)):
        assert len(items) == len(before) == 7
        for (x, t), (xr, tr) in zip(items, before):
            assert torch.equal(x, xr) and x.dtype == xr.dtype and ((t is None and tr is None) or (torch.equal(t, tr) and t.dtype == tr.dtype))
    for bs in (1, 2, 3, 16):
        want = R.batches_before(before, bs)
        for got in (list(s.batches(bs)), list(brs.batches(brs.load_dataset(root), bs))):
            assert len(got) == len(want)
            for (x, t), (xr, tr) in zip(got, want):
                assert torch.equal(x, xr) and ((t is None and tr is None) or torch.equal(t, tr))


def test_token_file_errors_name_the_file(tmp_path):
    def folder(name, tok):
        d = tmp_path / name
        d.mkdir()
        R.write_png(str(d / "img.png"), 64, 64, 1)
        np.save(d / "img.npy", tok)
        return str(d)
    good = np.random.default_rng(0).integers(0, 256, (8, 8))
    assert SelectionSet(folder("ok", good.astype(np.uint8)), "cpu", 256).resident
    top = good.copy(); top[3, 4] = 256
    neg = good.copy(); neg[7, 7] = -1
    for name, tok, words in (("shape", good[:, :7].astype(np.uint8), r"shape \(8, 7\).*\(8, 8\)"), ("flat", good.reshape(-1), r"shape \(64,\)"),
                             ("float", good.astype(np.float32), "must be integers.*float32"), ("top", top, r"\[\d+, 256\].*n_embed = 256"),
                             ("neg", neg, r"\[-1, \d+\]"), ("small_codebook", good, "n_embed = 16")):
        with pytest.raises(ValueError, match=f"{name}/img.npy: .*{words}"):
            SelectionSet(folder(name, tok), "cpu", 16 if name == "small_codebook" else 256)


def test_device_path_chosen_or_refused(tmp_path, capsys):
    u = [(64, 128)] * 5
    s = SelectionSet(R.make_folder(tmp_path / "with", u, tokens=set(range(5))), "cpu", 256)
    assert s.resident and s.items is None
    assert s.images.dtype == torch.uint8 and tuple(s.images.shape) == (5, 64, 128, 3) and s.tokens.dtype == torch.uint8 and tuple(s.tokens.shape) == (5, 8, 16)
    for i in range(5):
        assert np.array_equal(s.images[i].numpy(), R.write_png(str(tmp_path / "again.png"), 64, 128, 100 + i))
        assert np.array_equal(s.tokens[i].numpy(), np.load(tmp_path / "with" / f"{i}.npy"))
    assert torch.equal(s.table, R.table())
    s = SelectionSet(R.make_folder(tmp_path / "int64", u, tokens=set(range(5)), dtype=np.int64), "cpu", 256)
    assert s.resident and s.tokens.dtype == torch.int64
    np.save(tmp_path / "int64" / "0.npy", np.zeros((8, 16), dtype=np.uint8))          # one uint8 file among int64 ones: the array is int64
    s = SelectionSet(str(tmp_path / "int64"), "cpu", 256)
    assert s.resident and s.tokens.dtype == torch.int64 and not s.tokens[0].any()
    s = SelectionSet(R.make_folder(tmp_path / "without", u, tokens=set()), "cpu", 256)
    assert s.resident and s.tokens is None and tuple(s.images.shape) == (5, 64, 128, 3)
    s = SelectionSet(R.make_folder(tmp_path / "odd", [(50, 30)] * 2, tokens=set()), "cpu", 256)       # any one shape, without tokens
    assert s.resident
    capsys.readouterr()
    s = SelectionSet(R.make_folder(tmp_path / "some", u, tokens={0, 3}), "cpu", 256)
    assert not s.resident and "only 2 of 5 images have tokens" in s.reason and s.reason in capsys.readouterr().err
    s = SelectionSet(R.make_folder(tmp_path / "shapes", u + [(128, 64)], tokens=set(range(6))), "cpu", 256)
    assert not s.resident and "differ in shape" in s.reason
    s = SelectionSet(R.make_folder(tmp_path / "padded", [(100, 72)] * 2, tokens={0, 1}), "cpu", 256)      # tokens of the padded image, (16, 16)
    assert not s.resident and "not of shape (100 / 8, 72 / 8)" in s.reason
    need = 5 * 64 * 128 * 3 + 5 * 8 * 16
    assert SelectionSet(str(tmp_path / "with"), "cpu", 256, max_device_bytes=need).resident
    s = SelectionSet(str(tmp_path / "with"), "cpu", 256, max_device_bytes=need - 1)
    assert not s.resident and f"{need} bytes" in s.reason and f"budget of {need - 1} bytes" in s.reason and len(s.items) == 5
    # the default budget is 2 GiB; the reference's set (2000 crops of 256 x 256 with uint8 tokens) is resident, 11000 such crops are not
    full = lambda m: residency([(256, 256)] * m, [((32, 32), "uint8")] * m)
    assert full(2000)[0] and not full(11000)[0] and str(2 << 30) in full(11000)[1]
    assert residency([], []) == (False, "the folder holds no png")


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_tokens_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_tokens.h"))
    P, I = C.c_void_p, C.c_int
    assert protos == {"dcvic_u8_hwc_to_f32_nchw": (I, [P, I, I, I, P, P, P]), "dcvic_vq_token_feat_f32": (I, [P, I, P, I, I, I, I, I, P, P, P, P])}
    assert test_cabi.signature_mismatches(_lib.TOKEN_SIGNATURES, protos) == []
    others, tables = set(), set()
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "dcvic_tokens.h":
            others |= set(loss_header_prototypes(os.path.join(ROOT, "include", h)))
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "TOKEN_SIGNATURES":
            tables |= set(getattr(_lib, name))
    assert not set(protos) & others and not set(_lib.TOKEN_SIGNATURES) & tables
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert test_cabi.signature_mismatches(dict(_lib.TOKEN_SIGNATURES, dcvic_u8_hwc_to_f32_nchw="i:piiqppp"), protos) != []


def test_argument_refusals_without_gpu():
    assert R.check_refusals() == 26


# ---------------------------------------------------------------------------------------------------- the restatements
def test_restatements_agree_with_the_torch_expressions():
    """Kernel A's restatement is the table expression bit for bit; kernel B's is the torch chain on valid tokens, and states the rule
    for invalid ones."""
    for shape in ((1, 8, 8), (3, 24, 40), (2, 7, 13)):
        src = R.u8_case(*shape, seed=sum(shape))
        assert torch.equal(R.u8_hwc_to_f32_nchw_ref(src, R.table()), R.table_expression(src))
    for (N, h, w, D, n_e) in ((1, 1, 1, 4, 256), (2, 3, 5, 4, 256), (3, 32, 32, 4, 256), (2, 5, 3, 8, 16)):
        cb = R.codebook_case(n_e, D, 5)
        tok = R.token_case(N, h, w, n_e, 9)
        for got, want in zip(R.vq_token_feat_ref(tok, cb), R.torch_chain(tok, cb)):
            assert torch.equal(got, want)
        assert torch.equal(R.vq_token_feat_ref(tok.to(torch.uint8), cb)[2], R.torch_chain(tok, cb)[2])
    cb, tok = R.codebook_case(16, 8, 5), R.token_case(2, 5, 3, 16, 9)
    bad = tok.clone()
    bad[0, 1, 1], bad[1, 4, 2] = 16, -1
    idx, zq, feat = R.vq_token_feat_ref(bad, cb)
    _, zq0, feat0 = R.torch_chain(tok, cb)
    hit = (bad != tok).unsqueeze(1)
    assert torch.equal(idx, bad) and torch.isnan(zq[hit.expand_as(zq)]).all() and torch.equal(torch.where(hit, zq0, zq), zq0)
    assert not feat[:, 8:][hit.expand(-1, 16, -1, -1)].any() and torch.equal(torch.where(hit, feat0, feat)[:, 8:], feat0[:, 8:])
