"""Stage-level and end-to-end parity of the HIP path on a real MI355X.  Stage tolerances are absolute, ~10x the error
measured on MI355X in round 2 (recorded per tag in gpurun_out/parity_report.json -> "stage_goldens").

 * stages vs the committed goldens (produced by the reference's own modules, oracle/gen_golden.py);
 * end-to-end vs the CPU oracle on the same seeded inputs, with integer decisions (VQ indices,
   symbols, cdf indexes) compared exactly up to itemised fp32 near-ties;
 * size-independent properties at the benchmark size: encode -> bytes -> decode round trip is
   bit-exact, results do not depend on the batch an image travels in.
Tolerances are stated where used (fp32 MFMA fma-chains vs MKL/oneDNN summation order)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available()
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": "cuda:0"})
    m = build_comp_model(opt)
    load_synth_weights(m, 1234)
    m.codec_setup()
    return m


def dev(a):
    return torch.from_numpy(np.asarray(a)).to("cuda:0")


_STAGE_ERR = {}


def close(a, b, rtol, atol, tag=None):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    if tag is not None:          # measured error, written to gpurun_out/parity_report.json so the tolerances can be audited
        _STAGE_ERR[tag] = max(_STAGE_ERR.get(tag, 0.0), float(np.abs(a - b).max()))
        from parity_util import Report
        rep = Report("stage_goldens")
        rep.err = dict(_STAGE_ERR)
        rep.dump()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def img(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1


# ------------------------------------------------------------------------------ stages vs goldens
def test_stage_vqgan_encoder(model, golden):
    z = model.vq_model.encode(dev(golden["a4_x"]))
    close(z, golden["a4_z"], rtol=0, atol=1.5e-4, tag="a4_z")     # 30 layers of fp32 re-association
    z = model.vq_model.encode(dev(golden["a4b_x"]))
    close(z, golden["a4b_z"], rtol=0, atol=1.5e-4, tag="a4b_z")


def test_stage_vq_indices(model, golden):
    zq, _, (_, _, idx) = model.vq_model.quantize(dev(golden["a4_z"]))
    assert np.array_equal(idx.cpu().numpy(), golden["a5_idx"])          # same z_e in -> index-exact
    assert np.array_equal(zq.cpu().numpy(), golden["a5_zq"])
    # a5b: a dense random cloud around the codebook (many near-equidistant codes).  Identical z in -> every disagreement must be
    # a tie within the fp32 slack of the expanded-form distance itself (vq_flips with dz = 0), itemised and capped
    from parity_util import Report, vq_flips
    zq, _, (_, _, idx) = model.vq_model.quantize(dev(golden["a5b_z"]))
    rep = Report("stage_a5b_vq")
    zb = torch.from_numpy(golden["a5b_z"])
    vq_flips(rep, "vq_idx(a5b cloud)", idx, torch.from_numpy(golden["a5b_idx"]), zb, zb, model.vq_model.quantize.embedding.weight)
    rep.dump()
    ok = idx.cpu().numpy() == golden["a5b_idx"]
    assert np.array_equal(zq.cpu().numpy().transpose(0, 2, 3, 1)[ok], golden["a5b_zq"].transpose(0, 2, 3, 1)[ok])


def test_stage_elic_encoder(model, golden):
    from dc_vic_amd import ops
    x = dev(golden["a4_x"])
    _, _, feat = ops.vq_argmin(dev(golden["a4_z"]), model.vq_model.quantize.embedding.weight, want_zq=False, want_feat=True)
    for q in (0, 3):
        y = model.encoder(x, feat, model.selected_beta_rate[q], model.selected_beta_vq[q])
        close(y, golden[f"a6_y_q{q}"], rtol=0, atol=2e-5, tag="a6_y")
    # per-sample beta tensors
    g = torch.Generator().manual_seed(15)
    f2 = (torch.randn((2, 260, 8, 8), generator=g) * 0.3).to("cuda:0")
    y = model.encoder(img((2, 3, 64, 64), 14).to("cuda:0"), f2, torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5]))
    close(y, golden["a6b_y"], rtol=0, atol=2e-5, tag="a6b_y")


def test_stage_hyper(model, golden):
    close(model.hyperencoder(dev(golden["a6_y_q0"])), golden["a7_z"], rtol=0, atol=5e-6, tag="a7_z")
    close(model.hyperdecoder(dev(golden["a9_zhat"])), golden["a9_out"], rtol=0, atol=6e-5, tag="a9_out")


def test_stage_elic_decoder_feats(model, golden):
    f1, fd = model.decoder.get_feats(dev(golden["a14_yhat"]), model.selected_beta_rate[1], model.selected_beta_vq[1])
    close(f1, golden["a14_feat1"], rtol=0, atol=4e-4, tag="a14_feat1")
    close(fd["block_1_4"][:, :, :8, :8], golden["a14_b14_crop"], rtol=0, atol=4e-4, tag="a14_b14")
    close(fd["block_1_2"][:, :, 10:18, 20:28], golden["a14_b12_crop"], rtol=0, atol=4e-4, tag="a14_b12")


@pytest.mark.parametrize("tag", ["a15", "a15b"])
def test_stage_swin_estimator(model, golden, tag):
    pe, lg = model.vq_estimator(dev(golden[f"{tag}_feat"]), want_embed=True)
    close(pe, golden[f"{tag}_pred_embed"], rtol=0, atol=1e-4, tag="a15_pred_embed")
    close(lg[:, ::16, :4, :4], golden[f"{tag}_logits_crop"], rtol=0, atol=5e-4, tag="a15_logits")
    # argmax decisions: exact, except where the reference's own top-2 margin is below the logit difference measured at that
    # position (itemised near-ties)
    from parity_util import Report, argmax_flips
    rep = Report(f"stage_{tag}_argmax")
    lo = torch.from_numpy(golden[f"{tag}_logits"])
    assert np.array_equal(lo.argmax(1).numpy(), golden[f"{tag}_argmax"])
    close(lg, lo, rtol=0, atol=5e-4, tag="a15_logits")
    argmax_flips(rep, "argmax", lg.argmax(1), lg, lo)
    rep.dump()
    assert rep.n_flips() <= 2


def test_stage_fusion_decoder(model, golden):
    from dc_vic_amd import ops
    pq = model.vq_model.post_quant_conv
    logits = torch.nn.functional.one_hot(dev(golden["a17_idx"]), 256).permute(0, 3, 1, 2).float().contiguous()
    idx, lat = ops.argmax_lut(logits, model.vq_model.quantize.embedding.weight, pq.weight.reshape(4, 4).contiguous(), pq.bias)
    assert np.array_equal(idx.cpu().numpy(), golden["a17_idx"])
    close(lat, golden["a17_lat"], rtol=1e-5, atol=1e-7)
    cf = {k: dev(golden[f"a17_{k}"]) for k in ("block_1_8", "block_1_4", "block_1_2")}
    out = model.fusion_module(lat, cf, model.vq_model.decoder, w=1.0)
    close(out[:, :, 16:48, 30:62], golden["a17_out_crop"], rtol=0, atol=2e-4, tag="a17_out")
    close(out[:, :, ::4, ::4], golden["a17_out_ds"], rtol=0, atol=2e-4, tag="a17_out")
    plain = model.vq_model.decoder(lat)
    close(plain[:, :, ::4, ::4], golden["a17p_out_ds"], rtol=0, atol=1e-4, tag="a17p_out")


# ------------------------------------------------------------------------------ a10 CHARM vs the reference module
@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_stage_charm_vs_reference_module(model, charm_golden, tag):
    """context_model.run vs the reference's own Minnen20CharmContextModel.forward (tests/golden/charm.npz, fixture
    docstring in oracle/gen_golden.py).  Teacher-forced with the reference's symbols round(y - mu_ref), so every
    slice sees the reference's support; the HIP rounding itself is checked against the same symbols with
    near-ties (|frac(y - mu) - 1/2| <= |mu_hip - mu_ref| at that element) itemised."""
    from dc_vic_amd import ops
    from parity_util import Report, round_flips
    G = charm_golden
    y, ho = dev(G[f"{tag}_y"]), dev(G[f"{tag}_hyper_out"])
    sym_ref = torch.from_numpy(np.round(G[f"{tag}_y"] - G[f"{tag}_mu"]).astype(np.int32)).to("cuda:0")
    sc = model.context_model.slice_ch
    r = model.context_model.run(None, ho, model.entropy_model_y, symbols_in=lambda i, ix: sym_ref[:, i * sc:(i + 1) * sc].contiguous(),
                                want_likelihood=False)
    close(r["mu"], G[f"{tag}_mu"], rtol=0, atol=1e-5, tag="charm_mu")
    close(r["sigma"], G[f"{tag}_sigma"], rtol=0, atol=6e-5, tag="charm_sigma")
    close(r["y_hat"], G[f"{tag}_y_hat"], rtol=0, atol=1e-5, tag="charm_y_hat")
    # free-running encode side: the HIP path rounds by itself
    rep = Report(f"charm_{tag}")
    f = model.context_model.run(y, ho, model.entropy_model_y, want_likelihood=True, want_symbols=True)
    first = None
    for i in range(model.context_model.num_slices):
        sl = slice(i * sc, (i + 1) * sc)
        if not torch.equal(f["symbols"][:, sl], sym_ref[:, sl]):
            first = i
            break
    if first is None:
        close(f["y_hat"], G[f"{tag}_y_hat"], rtol=0, atol=1e-4)
    else:   # the first differing slice still has the reference's support: its flips must be rounding near-ties
        sl = slice(first * sc, (first + 1) * sc)
        round_flips(rep, f"charm slice {first}", f["symbols"][:, sl], sym_ref[:, sl], torch.from_numpy(G[f"{tag}_y"] - G[f"{tag}_mu"])[:, sl],
                    f["mu"][:, sl].cpu().numpy() - G[f"{tag}_mu"][:, sl])
    rep.dump()


# ------------------------------------------------------------------------------ end to end vs oracle (teacher-forced)
from conftest import demo_image as _demo  # noqa: E402


def full_parity(model, oracle, oracle_compress, tag, key, x, q):
    from parity_util import Report, decode_parity, encode_parity, free_running_compress
    rep = Report(tag)
    try:
        ro = oracle_compress(key, x, q)
        encode_parity(model, ro, x, q, rep)
        rg = free_running_compress(model, ro, x, q, rep)
        d = decode_parity(model, oracle, ro, q, rep)
        # free-running decompress of the product's own stream reproduces its encoder-side latents bit for bit
        img_g, zh_g, yh_g = model.decompress(rg["string_list"])
        assert torch.equal(yh_g, rg["y_hat"]) and torch.equal(zh_g, rg["z_hat"])
        if rg["string_list"] == ro["string_list"] and "img" in d and torch.equal(d["out_idx"].cpu(), d["oracle"]["out_idx"]):
            from oracle.dcvic_oracle import postprocess
            H, W = x.shape[2:]
            rep.close("img(compress->decompress)", img_g, postprocess(d["oracle"]["img"], H, W), key="img")
    finally:
        rep.dump()
    return rep


@pytest.mark.parametrize("shape,seed,q", [((1, 3, 64, 96), 101, 0), ((1, 3, 64, 64), 102, 2), ((1, 3, 100, 70), 105, 4)])
def test_parity_small_and_ragged(model, oracle, oracle_compress, shape, seed, q):
    """Ragged sizes (reflect pad to x64 + crop): every stage teacher-forced against the oracle, integer decisions exact up
    to itemised near-ties, bytes identical, bpp to 4 decimals, reconstruction <= 1e-3."""
    full_parity(model, oracle, oracle_compress, f"small_{shape[2]}x{shape[3]}_q{q}", ("rand", shape, seed), img(shape, seed), q)


@pytest.mark.parametrize("seed,q", [(201, 0), (202, 1), (203, 2), (204, 3), (201, 4)])
def test_parity_256(model, oracle, oracle_compress, seed, q):
    """BASELINE config 2's image size, four different images, q = 0..4."""
    full_parity(model, oracle, oracle_compress, f"256_s{seed}_q{q}", ("rand", (1, 3, 256, 256), seed), img((1, 3, 256, 256), seed), q)


@pytest.mark.parametrize("name", ["kodim03.png", "kodim15.png", "kodim23.png"])
@pytest.mark.parametrize("q", [0, 2, 4])
def test_parity_kodak(model, oracle, oracle_compress, name, q):
    """BASELINE config 3: real Kodak images (the reference's demo_images, 768x512; data fixtures under tests/golden/), EVERY
    image at EVERY q in {0, 2, 4} (the three of the 24 the reference ships x the three qualities of rd_results/kodak.csv:7,9,11):
    real-bytes and predicted bpp to 4 decimals, reconstruction <= 1e-3."""
    x = _demo(name)
    assert x.shape == (1, 3, 512, 768)
    full_parity(model, oracle, oracle_compress, f"kodak_{name[:-4]}_q{q}", ("demo", name), x, q)


def test_run_model_vs_oracle(model, oracle):
    """Batched rate-estimation forward (hyperprior_dc_vic_model.py:112-118) on a batch of two 256x256 images: stage by stage
    against the oracle's run_model with per-element near-tie bounds and caps (parity_util.run_model_parity) -- bpp / qbpp to 4
    decimals, fake_images <= TOL["img"], no rate-only fallback."""
    from parity_util import Report, run_model_parity
    x = img((2, 3, 256, 256), 103)
    ro = oracle.run_model(x, 1.51, 2.25)
    rep = Report("run_model_2x256")
    try:
        rg = run_model_parity(model, ro, x, 1.51, 2.25, rep)
    finally:
        rep.dump()
    close(rg["real_images"], ro["real_images"], rtol=0, atol=0)


# ------------------------------------------------------------------------------ a18 tiling (> 1024 px), config 4
def test_tiling_vs_oracle(model, oracle, oracle_compress):
    """hyperprior_vic_model.py:190-246 (_vq_encode_split) and 413-473 (decode_split) on a 1088x576 image: 4 x 2 windows on
    both sides.  Encode: the stitched z_e and everything after it, teacher-forced (encode_parity takes the split branch).
    Decode: every 32x32-latent window of the oracle's y_hat goes through the teacher-forced decode stages, and the
    product's stitched image must equal, bit for bit, the test's own stitching of the product's per-window outputs
    (window starts / centre-crop rectangles restated here from the reference loop)."""
    from oracle import dcvic_oracle as O
    from parity_util import Report, decode_parity, encode_parity, free_running_compress, dev as pdev
    q = 1
    x = img((1, 3, 1088, 576), 301)
    rep = Report("tiling_1088x576_q1")
    try:
        ro = oracle_compress(("rand", (1, 3, 1088, 576), 301), x, q)
        assert ro["x_pad"].shape[2:] == (1088, 576)
        encode_parity(model, ro, x, q, rep)
        rg = free_running_compress(model, ro, x, q, rep)
        b1, b2 = model.selected_beta_rate[q], model.selected_beta_vq[q]
        y_hat = ro["y_hat"]
        yH, yW = y_hat.shape[2:]
        tops, lefts = O._split_starts(yH, 16, 32), O._split_starts(yW, 16, 32)
        assert tops == [0, 16, 32, 36] and lefts == [0, 4]
        stitched = torch.full((1, 3, yH * 16, yW * 16), -100.0)
        flips_before = rep.n_flips()
        for y0 in tops:
            for x0 in lefts:
                crop = y_hat[:, :, y0:y0 + 32, x0:x0 + 32].contiguous()
                sub = {**ro, "y_hat": crop}
                yh = pdev(crop)
                o, _ = model._decode(yh, 1.0, b1, b2)
                wrep = Report(f"tiling_win_{y0}_{x0}")
                # teacher-forced decode stages of this window (argmax near-ties itemised per window)
                do = O.decode_trace(oracle.sd, crop, b1, b2)
                _window_decode_parity(model, do, yh, b1, b2, wrep)
                rep.flips.update({f"win({y0},{x0}) {k}": v for k, v in wrep.flips.items()})
                rep.err.update({f"win({y0},{x0}) {k}": v for k, v in wrep.err.items()})
                rep.caps.update({f"win({y0},{x0}) {k}": v for k, v in wrep.caps.items()})
                off = 8 * 16
                _x0, _y0 = x0 * 16, y0 * 16
                l = _x0 + off if x0 > 0 else 0
                t = _y0 + off if y0 > 0 else 0
                r = _x0 + off + 256 if x0 < lefts[-1] else yW * 16
                b = _y0 + off + 256 if y0 < tops[-1] else yH * 16
                stitched[:, :, t:b, l:r] = o.cpu()[:, :, t - _y0:b - _y0, l - _x0:r - _x0]
        # decode_split decodes the 8 windows as ONE batch (comp_model.TILE_BATCH); `stitched` was built window by window at N = 1
        out = model.decode_split(pdev(y_hat), 1.0, beta_rate=b1, beta_vq=b2)
        assert torch.equal(out.cpu(), stitched), "decode_split (batched windows) differs from the reference loop's window-by-window rectangles"
        # same for the encoder side: batched windows == one window per launch, bit for bit
        from dc_vic_amd import comp_model as cm
        xp = model.img_preprocess(x, is_train=False)
        z_b = model._vq_encode_split(xp)
        old = cm.TILE_BATCH
        cm.TILE_BATCH = 1
        try:
            z_1 = model._vq_encode_split(xp)
            out_1 = model.decode_split(pdev(y_hat), 1.0, beta_rate=b1, beta_vq=b2)
        finally:
            cm.TILE_BATCH = old
        assert torch.equal(z_b, z_1) and torch.equal(out_1, out), "tiling windows as a batch change bits"
        assert float(out.min()) > -99.0                                   # every pixel was written
        # the product's own stream round-trips through the tiled decoder
        img_g, zh_g, yh_g = model.decompress(rg["string_list"])
        assert torch.equal(yh_g, rg["y_hat"]) and img_g.shape == x.shape
        if rep.n_flips() == 0:
            img_o, _, _, _ = oracle.decompress(ro["string_list"])
            rep.close("img(tiled compress->decompress)", img_g, img_o, key="img")
    finally:
        rep.dump()


def _window_decode_parity(model, do, yh, b1, b2, rep):
    from dc_vic_amd import ops
    from parity_util import argmax_flips, dev as pdev
    f1, fd = model.decoder.get_feats(yh, beta_1=b1, beta_2=b2)
    rep.close("feat_1", f1, do["feat_1"], key="feat")
    _, lg = model.vq_estimator(pdev(do["feat_1"]))
    rep.close("logits", lg, do["logits"])
    pq = model.vq_model.post_quant_conv
    cbw = model.vq_model.quantize.embedding.weight
    idx_g, _ = ops.argmax_lut(lg, cbw, pq.weight.reshape(pq.out_channels, -1).contiguous(), pq.bias)
    argmax_flips(rep, "out_idx", idx_g, lg, do["logits"])
    cf = {k: pdev(v) for k, v in do["feats"].items()}
    out = model.fusion_module(pdev(do["lat"]), cf, model.vq_model.decoder, w=1.0)
    rep.close("img", out, do["img"])


def test_tiling_window_starts_and_guards(model):
    """Window starts of both tiling loops for sizes around the thresholds, and the short-side guard: an image with
    max(H, W) > 1024 whose other side is < 512 cannot be tiled by the reference loop (negative start) -> clear error."""
    from dc_vic_amd.comp_model import _starts
    assert _starts(1088, 256, 512, True) == [0, 256, 512, 576]
    assert _starts(576, 256, 512, True) == [0, 64]
    assert _starts(512, 256, 512, True) == [0]
    assert _starts(68, 16, 32, False) == [0, 16, 32, 36] and _starts(36, 16, 32, False) == [0, 4]
    with pytest.raises(ValueError, match="512"):
        model.compress(img((1, 3, 1088, 300), 302), 0)


# ------------------------------------------------------------------------------ properties at full size
def test_roundtrip_bit_exact_256(model):
    """encode -> bytes -> decode at the benchmark shape: the decoder reproduces the encoder's y_hat / z_hat
    bit for bit (GPU-resident CHARM on both sides), and two identical calls give identical bytes."""
    x = img((4, 3, 256, 256), 104)
    r = model.compress_batch(x, 0)
    r2 = model.compress_batch(x, 0)
    assert r["string_lists"] == r2["string_lists"]
    imgs, z_hat, y_hat = model.decompress_batch(r["string_lists"])
    assert torch.equal(y_hat, r["y_hat"]) and torch.equal(z_hat, r["z_hat"])
    assert imgs.shape == (4, 3, 256, 256) and float(imgs.abs().max()) <= 1.0
    # batch invariance: image 2 alone gives the same bytes and the same reconstruction
    r1 = model.compress(x[2:3], 0)
    assert r1["string_list"] == r["string_lists"][2]
    i1, _, _ = model.decompress(r1["string_list"])
    assert torch.equal(i1[0], imgs[2])
    # real bytes vs predicted bits: rANS overhead is small
    for i in range(4):
        real_bits = 8 * (len(r["string_lists"][i][1]) + len(r["string_lists"][i][2]))
        pred = float(r["pred_y_bit"][i] + r["pred_z_bit"][i])
        # rANS adds <= 2 flush words per stream + 16-bit probability quantisation to the estimate;
        # escape-coded outliers may undercut the 1e-9 likelihood floor, so the band is two-sided
        assert 0.85 * pred - 256 < real_bits < 1.10 * pred + 256, (real_bits, pred)


def test_batch_invariance_at_32(model):
    """The benchmark's batch size, graph path included (default policy: eager, capture, replay): the bytes do not depend on which of the
    three ran, an image coded alone gives the bytes and the reconstruction it gives inside the batch of 32 -- what lets a decoder in one
    batch read a stream written in another -- and the decoder reproduces the encoder's latents bit for bit."""
    assert not model._graphs.disabled and model._graphs.capture_after == 2
    x = img((32, 3, 256, 256), 110)
    r = model.compress_batch(x, 0)
    for _ in range(2):
        assert model.compress_batch(x, 0)["string_lists"] == r["string_lists"]
    assert ("enc", (32, 3, 256, 256)) in {k[:2] for k in model._graphs.entries}
    imgs = None
    for _ in range(3):
        out, z_hat, y_hat = model.decompress_batch(r["string_lists"])
        assert torch.equal(y_hat, r["y_hat"]) and torch.equal(z_hat, r["z_hat"])
        assert imgs is None or torch.equal(out, imgs)
        imgs = out.clone()
    assert "dec" in {k[0] for k in model._graphs.entries} and not model._graphs.disabled
    assert imgs.shape == (32, 3, 256, 256)
    for k in (0, 13, 31):
        r1 = model.compress(x[k:k + 1], 0)
        assert r1["string_list"] == r["string_lists"][k], k
        i1, _, _ = model.decompress(r["string_lists"][k])
        assert torch.equal(i1[0], imgs[k]), k


def test_ragged_and_kodak_shape(model):
    """Non-multiple-of-64 image (reflect pad + crop) and the Kodak shape 512x768 round-trip."""
    for shape, q in (((1, 3, 100, 70), 4), ((1, 3, 512, 768), 2)):
        x = img(shape, 105)
        r = model.compress(x, q)
        out, z_hat, y_hat = model.decompress(r["string_list"])
        assert out.shape == shape
        assert torch.equal(y_hat, r["y_hat"])
        from dc_vic_amd.codec_utils import HeaderHandler
        hd = HeaderHandler().decode(r["string_list"][0])
        assert hd["img_size"] == shape[2:] and hd["quality_ind"] == q


def test_charm_split_and_streams_bit_identical(model, monkeypatch):
    """The stacked hyperprior partial convs (accumulator hand-over through `init`) and the two-stream schedule are
    pure re-schedulings: symbols, cdf indexes and y_hat are bit-identical to the plain sequential CHARM."""
    x = img((3, 3, 128, 192), 106)
    monkeypatch.setenv("DCVIC_CHARM_SPLIT", "0"); monkeypatch.setenv("DCVIC_CHARM_STREAMS", "0")
    a = model.compress_batch(x, 1)
    monkeypatch.setenv("DCVIC_CHARM_SPLIT", "1"); monkeypatch.setenv("DCVIC_CHARM_STREAMS", "1")
    b = model.compress_batch(x, 1)
    assert torch.equal(a["y_symbols"], b["y_symbols"]) and torch.equal(a["y_indexes"], b["y_indexes"])
    assert torch.equal(a["y_hat"], b["y_hat"])
    assert a["string_lists"] == b["string_lists"]


def test_hipgraph_replay_identical_to_eager(model):
    """The encoder / decoder networks replay as captured hipGraphs (default since round 3, DCVIC_GRAPHS=0 switches it off).  Same
    kernels, same arguments: bytes and reconstructions equal the eager path's, across repeated replays and a second shape; a shape is
    captured the SECOND time it is seen (capture_after = 2)."""
    g = model._graphs
    was, was_after = g.disabled, g.capture_after
    assert was_after == 2 and not was
    g.clear()
    x0 = img((1, 3, 64, 64), 109)
    model.compress_batch(x0, 0)
    assert not g.entries                               # first sighting: eager
    model.compress_batch(x0, 0)
    assert [k[0] for k in g.entries] == ["enc"]        # second: captured and replayed
    g.capture_after = 1
    try:
        for shape, q in (((1, 3, 256, 256), 0), ((2, 3, 128, 192), 3)):
            x1, x2 = img(shape, 107), img(shape, 108)
            g.disabled = True
            e1, e2 = model.compress_batch(x1, q), model.compress_batch(x2, q)
            ei1 = model.decompress_batch(e1["string_lists"])[0].clone()
            ei2 = model.decompress_batch(e2["string_lists"])[0].clone()
            g.disabled = False
            g.clear()
            for _ in range(2):      # first pass captures, second replays
                r1, r2 = model.compress_batch(x1, q), model.compress_batch(x2, q)
                assert r1["string_lists"] == e1["string_lists"] and r2["string_lists"] == e2["string_lists"]
                assert torch.equal(r1["y"], e1["y"]) and torch.equal(r2["vq_indices"], e2["vq_indices"])
                i1 = model.decompress_batch(r1["string_lists"])[0].clone()
                i2 = model.decompress_batch(r2["string_lists"])[0].clone()
                assert torch.equal(i1, ei1) and torch.equal(i2, ei2)
            assert not g.disabled, "hipGraph capture failed and fell back to eager"
            kinds = sorted(k[0] for k in g.entries)
            assert "dec" in kinds and "enc" in kinds, kinds
    finally:
        g.disabled, g.capture_after = was, was_after
        g.clear()


def test_fused_groupnorm_statistics_change_only_the_decoder_at_1e6(model):
    """GroupNorm statistics from the F(4x4) epilogue (decoder side only): the bitstream, the latents and the decoded VQ indices are
    untouched bit for bit, the reconstruction moves by < 5e-5 (measured 1.4e-5) against the two-pass GroupNorm (ops.GN_FUSED_STATS = False)."""
    from dc_vic_amd import ops
    x = img((2, 3, 256, 256), 120)
    g_was = model._graphs.disabled
    model._graphs.disabled = True                      # (a captured decoder graph would freeze whichever variant it recorded)
    old = ops.GN_FUSED_STATS
    try:
        r1 = model.compress_batch(x, 1)
        i1, z1, y1 = model.decompress_batch(r1["string_lists"])
        ops.GN_FUSED_STATS = False
        r0 = model.compress_batch(x, 1)
        i0, z0, y0 = model.decompress_batch(r0["string_lists"])
    finally:
        ops.GN_FUSED_STATS = old
        model._graphs.disabled = g_was
    assert r0["string_lists"] == r1["string_lists"] and torch.equal(y0, y1) and torch.equal(z0, z1)
    d = float((i0 - i1).abs().max())
    assert 0.0 < d < 5e-5, d              # measured 1.4e-5 (24 GroupNorms with fp32 tile sums); > 0: the fused path really ran
