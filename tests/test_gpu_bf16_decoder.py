"""Opt-in bf16 reconstruction (model.set_decoder_precision("bf16"), csrc/conv_bf16.hip) on a real MI355X.

 * the kernel against a float64 convolution of the bf16-rounded operands (what remains is fp32 accumulation error);
 * the pack equals weight.to(torch.bfloat16) bit for bit;
 * nothing upstream of the reconstruction moves: bitstreams, latents, estimator logits and indices are bit-identical to fp32 mode;
 * fidelity against the fp32 reconstruction (>= 50 dB PSNR on [0, 1], max |diff| <= 0.1 on [-1, 1]), tiled images included;
 * determinism, batch invariance, the hipGraph cache across precision switches, the default, training, and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CFG = os.path.join(ROOT, "config", "dc_vic_synthetic.yaml")
DEMO = os.path.join(ROOT, "tests", "golden", "demo_images")


def _new_model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    opt = BaseConfig.fromfile(CFG, {"device": DEV})
    m = build_comp_model(opt)
    load_synth_weights(m, 1234)
    m.codec_setup()
    return m


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available()
    m = _new_model()
    yield m
    m.set_decoder_precision("fp32")


def psnr01(a, b):
    """PSNR on [0, 1] of two [-1, 1] images."""
    mse = float((((a.double() - b.double()) / 2) ** 2).mean())
    return float("inf") if mse == 0 else 10 * np.log10(1.0 / mse)


def _png(path):
    from PIL import Image
    x = torch.from_numpy(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)
    return ((x - 0.5) / 0.5).unsqueeze(0)


# ------------------------------------------------------------------------------ kernel vs fp64 of the bf16-rounded operands
def _bf(t):
    return t.to(torch.bfloat16).double()


def _ref(srcs, w, b, ups, act, res, aff):
    x = torch.cat([_bf(s.cpu()) for s in srcs], 1)
    wd = _bf(w.cpu())
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, wd, None, padding=1)
    mag = F.conv2d(x.abs(), wd.abs(), None, padding=1)
    if b is not None:
        y = y + b.cpu().double().view(1, -1, 1, 1)
        mag = mag + b.cpu().double().abs().view(1, -1, 1, 1)
    if act == "lrelu":
        y = torch.where(y > 0, y, 0.2 * y)
    if res is not None:
        y = y + res.cpu().double()
        mag = mag + res.cpu().double().abs()
    if aff is not None:
        s, t = (v.cpu().double().view(v.shape[0], -1, 1, 1) for v in aff)
        y = y * (1 + s) + t
        mag = mag * (1 + s).abs() + t.abs()
    return y, mag


def _run(Cin_list, Cout, N, H, W, ups=False, bias=True, act=None, res=False, aff=False, seed=0, views=False):
    """views: the sources are channel slices of one buffer, with NaN channels around each (a read outside a source poisons the
    result), and the output is a channel slice of a larger buffer whose other channels must keep their sentinel."""
    from dc_vic_amd import ops
    g = torch.Generator().manual_seed(seed)
    Cin = sum(Cin_list)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / np.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    srcs = [torch.randn((N, c, H, W), generator=g).to(DEV) for c in Cin_list]
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    r = torch.randn((N, Cout, Ho, Wo), generator=g).to(DEV) if res else None
    a = (torch.randn((N, Cout), generator=g).mul(0.3).to(DEV), torch.randn((N, Cout), generator=g).mul(0.3).to(DEV)) if aff else None
    out = None
    if views:
        gap = 8
        buf = torch.full((N, Cin + gap * (len(Cin_list) + 1), H, W), float("nan"), device=DEV)
        o = gap
        for k, s in enumerate(srcs):
            buf[:, o:o + s.shape[1]] = s
            srcs[k] = buf[:, o:o + s.shape[1]]
            o += s.shape[1] + gap
        out_buf = torch.full((N, Cout + 24, Ho, Wo), -12345.0, device=DEV)
        out = out_buf[:, 16:16 + Cout]
    plan = ops.ConvPlan(w.to(DEV), b.to(DEV) if b is not None else None, "conv", pad=(1, 1), upsample=ups)
    plan.bf16 = True
    y = plan(srcs if len(srcs) > 1 else srcs[0], out=out, act=ops.ACT_LRELU02 if act == "lrelu" else ops.ACT_NONE, res=r, affine=a)
    torch.cuda.synchronize()
    if views:
        assert y.data_ptr() == out.data_ptr()
        assert bool((out_buf[:, :16] == -12345.0).all()) and bool((out_buf[:, 16 + Cout:] == -12345.0).all()), \
            "the output was written outside its channel slice"
    assert plan.last_bf16 and plan.bf16_launches == 1, "the launch did not run on the bf16 kernel"
    ref, mag = _ref(srcs, w, b, ups, act, r, a)
    err = (y.cpu().double() - ref).abs()
    bound = 1e-5 * mag + 1e-6
    worst = float((err / bound).max())
    print(f"bf16 conv Cin={Cin_list} Cout={Cout} N={N} {H}x{W} ups={ups}: max err / bound {worst:.3f}, max err {float(err.max()):.2e}")
    assert worst <= 1.0
    return plan, y


def _decoder_shapes(model):
    """(Cin, Cout, upsample) of every marked 3x3 layer the bf16 kernel takes."""
    from dc_vic_amd.layers import Conv2d
    shapes = set()
    for mod in (model.vq_model.decoder, model.fusion_module):
        for m in mod.modules():
            if isinstance(m, Conv2d) and m.kernel_size == 3 and m.padding == 1 and m.stride == 1 and m.in_channels % 8 == 0 and m.out_channels >= 16:
                shapes.add((m.in_channels, m.out_channels, bool(m.upsample)))
    return sorted(shapes)


def test_kernel_every_decoder_shape(model):
    shapes = _decoder_shapes(model)
    assert any(s[2] for s in shapes) and len(shapes) >= 6
    for i, (cin, cout, ups) in enumerate(shapes):
        _run([cin], cout, 2, 12 if ups else 24, 20 if ups else 40, ups=ups, seed=i)


def test_kernel_two_source_concat_and_full_epilogue():
    _run([192, 256], 256, 2, 24, 40, act="lrelu", res=True, aff=True, seed=11)
    _run([16, 48], 64, 1, 9, 13, ups=True, act="lrelu", res=True, aff=True, seed=12)


def test_kernel_ragged_and_batch_sizes():
    _run([64], 96, 1, 72, 136, seed=21)
    _run([64], 96, 3, 72, 136, res=True, seed=22)
    _run([40], 48, 3, 5, 7, ups=True, seed=23)
    _run([128], 128, 1, 1, 1, seed=24)


def test_kernel_three_sources_through_views():
    """The fusion buffers' layout: up to three sources read as channel slices of one buffer (each with its own offset and the buffer's
    batch stride), the output written into a channel slice, N = 3; with and without the fused upsample."""
    _run([192, 64, 256], 128, 3, 12, 20, seed=31, views=True)
    _run([192, 64, 256], 64, 3, 6, 10, ups=True, seed=32, views=True)
    _run([192, 64, 256], 96, 1, 7, 9, act="lrelu", res=True, aff=True, seed=33, views=True)
    _run([16, 48], 64, 3, 9, 13, ups=True, act="lrelu", res=True, aff=True, seed=34, views=True)
    _run([64], 96, 3, 17, 29, res=True, seed=35, views=True)


def test_kernel_batch_invariant():
    """Image k of a batch of 3 equals the same image launched alone, bit for bit."""
    from dc_vic_amd import ops
    g = torch.Generator().manual_seed(5)
    w = torch.randn((128, 256, 3, 3), generator=g).mul(0.02).to(DEV)
    x = torch.randn((3, 256, 40, 56), generator=g).to(DEV)
    plan = ops.ConvPlan(w, None, "conv", pad=(1, 1))
    plan.bf16 = True
    yb = plan(x)
    for k in range(3):
        assert torch.equal(plan(x[k:k + 1].contiguous()), yb[k:k + 1])


def test_pack_is_rne_bf16_of_the_weights():
    from dc_vic_amd import _lib, ops
    L = _lib.lib()
    shape = int(L.dcvic_conv3x3_bf16_mfma_shape())
    for cin, cout in ((704, 512), (40, 96)):
        w = torch.randn((cout, cin, 3, 3), generator=torch.Generator().manual_seed(cin)).to(DEV)
        nb = L.dcvic_conv3x3_bf16_packed_bytes(cin, cout)
        assert nb == -(-cout // 128) * 128 * -(-cin // 32) * 32 * 9 * 2
        p = torch.empty(nb // 2, dtype=torch.bfloat16, device=DEV)
        _lib.check(L.dcvic_conv3x3_bf16_pack_f32(ops._p(w), ops._p(p), cin, cout, ops._stream()), "pack")
        torch.cuda.synchronize()
        cp, kp = -(-cout // 128) * 128, -(-cin // 32)
        u = p.view(torch.int16).cpu()
        if shape == 32:    # [block32][chunk][tap][kstep][lane][8]: co = 32 block + lane % 32, ci = 32 chunk + 16 kstep + 8 (lane // 32) + j
            u = u.view(cp // 32, kp, 9, 2, 2, 32, 8).permute(0, 5, 1, 3, 4, 6, 2)
        else:              # [block16][chunk][tap][lane][8]: co = 16 block + lane % 16, ci = 32 chunk + 8 (lane // 16) + j
            u = u.view(cp // 16, kp, 9, 4, 16, 8).permute(0, 4, 1, 3, 5, 2)
        u = u.reshape(cp, kp * 32, 9)
        want = torch.zeros((cp, kp * 32, 9), dtype=torch.int16)
        want[:cout, :cin] = w.cpu().to(torch.bfloat16).view(torch.int16).reshape(cout, cin, 9)
        assert torch.equal(u, want)


# ------------------------------------------------------------------------------ the model in bf16 mode
def _cases():
    out = []
    for q in range(5):
        g = torch.Generator().manual_seed(100 + q)
        out.append((f"synth_q{q}", torch.rand((1, 3, 256, 256), generator=g) * 2 - 1, q))
    for n in sorted(os.listdir(DEMO)):
        out.append((n, _png(os.path.join(DEMO, n)), 2))
    return out


def test_nothing_upstream_moves_and_fidelity(model):
    from dc_vic_amd.layers import Conv2d
    psnrs = []
    for name, x, q in _cases():
        model.set_decoder_precision("fp32")
        r32 = model.compress(x, q)
        img32, z32, y32 = model.decompress(r32["string_list"])
        br, bv = model.selected_beta_rate[q], model.selected_beta_vq[q]
        _, idx32, log32 = model._decode(y32, 1.0, br, bv, want_logits=True)
        model.set_decoder_precision("bf16")
        assert model.decoder_precision == "bf16"
        r16 = model.compress(x, q)
        assert r16["string_list"] == r32["string_list"], name
        img16, z16, y16 = model.decompress(r16["string_list"])
        assert torch.equal(y16, y32) and torch.equal(z16, z32), name
        _, idx16, log16 = model._decode(y16, 1.0, br, bv, want_logits=True)
        assert torch.equal(log16, log32) and torch.equal(idx16, idx32), name
        p = psnr01(img16, img32)
        mx = float((img16 - img32).abs().max())
        psnrs.append(p)
        print(f"{name}: bf16 vs fp32 PSNR {p:.2f} dB, max |diff| {mx:.4f}")
        assert p >= 50.0 and mx <= 0.1, name
    # coverage: every marked layer the kernel takes ran on it, except the measured fp32 exemptions (comp_model.BF16_KEEP_FP32)
    from dc_vic_amd.comp_model import BF16_KEEP_FP32
    convs = [m for m in model.modules() if isinstance(m, Conv2d) and m._plan is not None]
    for m in convs:
        m._plan.bf16_launches = m._plan.fp32_launches = 0
    model._graphs.clear()                       # (an eager decode: the counters are host-side)
    model._decode(r16["y_hat"], 1.0, br, bv)
    ran16 = ran32 = 0
    for n, m in model.named_modules():
        if isinstance(m, Conv2d) and m.bf16 and m._plan is not None:
            ran16 += m._plan.bf16_launches
            ran32 += m._plan.fp32_launches
            if n in BF16_KEEP_FP32 or m.in_channels % 8 or m.out_channels < 16:
                assert m._plan.bf16_launches == 0, n
            else:
                assert m._plan.fp32_launches == 0 and m._plan.bf16_launches > 0, n
    print(f"PSNR range {min(psnrs):.2f} .. {max(psnrs):.2f} dB; marked launches on bf16: {ran16} of {ran16 + ran32}")
    model.set_decoder_precision("fp32")


def test_tiled_decode_split(model):
    g = torch.Generator().manual_seed(77)
    x = torch.rand((1, 3, 576, 1088), generator=g) * 2 - 1
    model.set_decoder_precision("fp32")
    r = model.compress(x, 1)
    i32, _, _ = model.decompress(r["string_list"])
    model.set_decoder_precision("bf16")
    i16, _, _ = model.decompress(r["string_list"])
    model.set_decoder_precision("fp32")
    p, mx = psnr01(i16, i32), float((i16 - i32).abs().max())
    print(f"tiled 1088x576: bf16 vs fp32 PSNR {p:.2f} dB, max |diff| {mx:.4f}")
    assert p >= 50.0 and mx <= 0.1


def test_determinism_batch_invariance_and_graph_cache(model):
    g = torch.Generator().manual_seed(9)
    xs = torch.rand((4, 3, 256, 256), generator=g) * 2 - 1
    model.set_decoder_precision("fp32")
    rb = model.compress_batch(xs, 0)
    streams = rb["string_lists"]
    # fp32 twice: the second call replays the captured graph
    a32, _, _ = model.decompress_batch(streams)
    b32, _, _ = model.decompress_batch(streams)
    assert torch.equal(a32, b32)
    model.set_decoder_precision("bf16")
    a16, _, _ = model.decompress_batch(streams)
    b16, _, _ = model.decompress_batch(streams)
    assert torch.equal(a16, b16)
    assert not torch.equal(a16, a32), "bf16 mode replayed the fp32 graph"
    # the eager bf16 decode (no graph) of the same latents
    _, _, y_hat = model.decompress_batch(streams)
    q = 0
    eager, _ = model._decode(y_hat, 1.0, model.selected_beta_rate[q], model.selected_beta_vq[q])
    from dc_vic_amd import ops
    assert torch.equal(ops.crop_clamp(eager, 256, 256), a16)
    # alone vs inside the batch of 4
    one, _, _ = model.decompress(streams[2])
    assert torch.equal(one, a16[2:3])
    model.set_decoder_precision("fp32")
    c32, _, _ = model.decompress_batch(streams)
    assert torch.equal(c32, a32)


def test_precision_switch_after_a_weight_change(model):
    """Graphs of both precisions captured, then one decoder convolution (a layer that does run on the bf16 kernel) updated in place: the
    switch to bf16 and back must not replay either graph, which hold the fp32 route packs and the bf16 pack of the OLD weights.  Both
    results equal their eager decode on the new weights, and both moved."""
    from dc_vic_amd.comp_model import BF16_KEEP_FP32
    name = "vq_model.decoder.up.1.block.0.conv1"
    assert name not in BF16_KEEP_FP32
    conv = model.get_submodule(name)
    g = model._graphs
    was = g.disabled
    xs = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(10)) * 2 - 1
    w_before = conv.weight.detach().clone()
    try:
        model.set_decoder_precision("fp32")
        streams = model.compress_batch(xs, 0)["string_lists"]
        old = {}
        for prec in ("fp32", "bf16"):
            model.set_decoder_precision(prec)
            for _ in range(3):                                 # eager, capture, replay
                old[prec] = model.decompress_batch(streams)[0].clone()
        assert {k[-1] for k in g.entries if k[0] == "dec"} == {"fp32", "bf16"}, list(g.entries)
        model.set_decoder_precision("fp32")
        with torch.no_grad():
            noise = torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(11)) * float(conv.weight.std())
            conv.weight.add_(noise.to(DEV))
        new = {}
        for prec in ("bf16", "fp32"):                          # to bf16 and back
            model.set_decoder_precision(prec)
            new[prec] = model.decompress_batch(streams)[0].clone()
        g.disabled = True
        for prec in ("bf16", "fp32"):
            model.set_decoder_precision(prec)
            eager = model.decompress_batch(streams)[0]
            assert torch.equal(new[prec], eager), f"{prec}: a graph captured with the old weights was replayed"
            assert not torch.equal(new[prec], old[prec]), prec
        assert not torch.equal(new["bf16"], new["fp32"])
    finally:
        g.disabled = was
        with torch.no_grad():
            conv.weight.copy_(w_before)
        model.set_decoder_precision("fp32")


def test_default_is_fp32_and_unknown_precision_raises(model):
    fresh = _new_model()
    assert fresh.decoder_precision == "fp32"
    g = torch.Generator().manual_seed(31)
    x = torch.rand((1, 3, 256, 256), generator=g) * 2 - 1
    r = fresh.compress(x, 3)
    a, _, _ = fresh.decompress(r["string_list"])
    fresh.set_decoder_precision("bf16")
    fresh.set_decoder_precision("fp32")
    b, _, _ = fresh.decompress(r["string_list"])
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        fresh.set_decoder_precision("fp16")


def test_training_ignores_decoder_precision():
    from dc_vic_amd.train import DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondTamingNLayerDiscriminator
    from dc_vic_amd.train import autograd as A
    m = _new_model()
    torch.manual_seed(5)
    D = DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, L=10, cond_ch=8,
                                              use_pi=False, include_x=True).to(DEV)
    tr = DualBetaCondGanDistortionVqCodeTrainer(m, D, seed=3)
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(90)) * 2 - 1
    b1, b2 = torch.tensor([2.29, 0.62]), torch.tensor([3.0, 1.5])
    fakes = []
    for prec in ("fp32", "bf16"):
        m.set_decoder_precision(prec)
        tr.g_group.zero_grad()
        o = tr.generator_forward(A.Ctx([tr.g_group]), x, None, b1, b2)
        fakes.append(o["fake"].data.clone())
    assert torch.equal(fakes[0], fakes[1])


def test_cli_decoder_precision(tmp_path):
    from PIL import Image
    outs = {}
    for prec in ("fp32", "bf16"):
        save = tmp_path / prec
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "compress.py"), "--config_path", CFG, "--model_path", "unused.pth.tar",
               "--img_dir", DEMO, "--save_dir", str(save), "-q", "1", "--decompress", "-d", "cuda:0", "--synthetic_weights",
               "--decoder_precision", prec]
        subprocess.check_call(cmd, cwd=ROOT, timeout=600)
        outs[prec] = save
    a, b = outs["fp32"], outs["bf16"]
    assert (a / "_bitrates.csv").read_bytes() == (b / "_bitrates.csv").read_bytes()
    assert json.load(open(a / "_avg_bitrate.json")) == json.load(open(b / "_avg_bitrate.json"))
    for n in sorted(os.listdir(DEMO)):
        assert (a / n.replace(".png", ".bin")).read_bytes() == (b / n.replace(".png", ".bin")).read_bytes()
        pa = np.asarray(Image.open(a / n), dtype=np.float64)
        pb = np.asarray(Image.open(b / n), dtype=np.float64)
        mse = ((pa - pb) / 255.0) ** 2
        p = float("inf") if mse.mean() == 0 else 10 * np.log10(1.0 / mse.mean())
        print(f"CLI {n}: bf16 vs fp32 PNG PSNR {p:.2f} dB")
        assert p >= 50.0
