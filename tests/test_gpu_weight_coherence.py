"""The state between the weights and the kernels -- packed convolution plans, fused q/k/v packs, cached beta vectors, captured
hipGraphs -- against every way of changing weights, on a real MI355X.

Every case: restore weights A, run compress + decompress three times (eager, capture, replay), change weights by the route under test,
run ONCE on the default (graph) path and compare bytes, y, VQ indices and image, bit for bit, with a second model that received the
live model's state dict through the top-level load_state_dict and runs eagerly; check that the observable the changed weights feed
really moved; run twice more and check that both segments were captured again and still agree.

Routes: top-level load_state_dict (control), load_state_dict of each child that owns parameters, an in-place op on one parameter per cache
site, a replaced parameter, and `p.data` writes followed by invalidate_weight_caches().  Without that call a `p.data` write is
unsupported (torch does not version it): the last test only runs it.  Nothing here releases memory a live graph points at: no
empty_cache(), and the first call after a change is the graph-path call."""
import os

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
Q = 0
CHILDREN = ("encoder", "decoder", "hyperencoder", "hyperdecoder", "entropy_model_z", "vq_estimator", "vq_model", "fusion_module",
            "context_model")


def _new_model(seed):
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV})
    m = build_comp_model(opt)
    load_synth_weights(m, seed)
    m.codec_setup()
    return m


@pytest.fixture(scope="module")
def x():
    return torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(2024)) * 2 - 1


def _run(m, x):
    r = m.compress_batch(x, Q)
    img = m.decompress_batch(r["string_lists"])[0]
    return dict(bytes=r["string_lists"], y=r["y"].clone(), vq_indices=r["vq_indices"].clone(), image=img.clone())


def _same(a, b):
    return {k: (a[k] == b[k] if k == "bytes" else torch.equal(a[k], b[k])) for k in ("bytes", "y", "vq_indices", "image")}


@pytest.fixture(scope="module")
def live():
    assert torch.cuda.is_available()
    m = _new_model(1234)
    assert not m._graphs.disabled and m._graphs.capture_after == 2
    return m


@pytest.fixture(scope="module")
def sd_a(live):
    return {k: v.detach().clone() for k, v in live.state_dict().items()}


@pytest.fixture(scope="module")
def sd_b(sd_a):
    """Seed-4321 weights under A's keys (the integer CDF tables stay A's: rebuilding them is codec_setup()'s job)."""
    from dc_vic_amd.synth import full_synth_state_dict
    b = full_synth_state_dict(4321)
    assert set(b) <= set(sd_a)
    return {k: (b[k].to(DEV) if k in b else v) for k, v in sd_a.items()}


@pytest.fixture(scope="module")
def expected(x):
    """expected(state_dict): what a model that got these weights by the one route known to be good computes, eagerly."""
    ref = _new_model(1234)
    ref._graphs.disabled = True

    def f(state_dict):
        ref.load_state_dict(state_dict)
        ref.codec_setup()
        assert ref._graphs.disabled and not ref._graphs.entries
        return _run(ref, x)
    return f


def _coherent_after(live, sd_a, expected, x, change, moved):
    """Steps 1-7 of the module docstring.  `moved`: the observables that must differ from weights A's."""
    g = live._graphs
    was = g.disabled, g.capture_after
    try:
        live.load_state_dict(sd_a)
        for _ in range(3):                                             # eager, capture, replay
            before = _run(live, x)
        assert {k[0] for k in g.entries} == {"enc", "dec"}, list(g.entries)
        change(live)
        after = _run(live, x)                                          # the graph path
        want = expected(live.state_dict())
        same = _same(after, want)
        still = _same(after, before)
        print("equal to the reference on the new weights:", same, "| equal to weights A's:", still)
        assert all(same.values()), f"stale after the change: {[k for k, v in same.items() if not v]}"
        for k in moved:
            assert not still[k], f"{k} did not move: the case proves nothing"
        for _ in range(2):                                             # capture, replay
            again = _run(live, x)
            assert all(_same(again, want).values())
        assert not g.disabled, "hipGraph capture failed and fell back to eager"
        assert {k[0] for k in g.entries} == {"enc", "dec"}, list(g.entries)
    finally:
        g.disabled, g.capture_after = was
        live.load_state_dict(sd_a)


def _sub(sd, name):
    return {k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}


# ------------------------------------------------------------------------------ load_state_dict
def test_control_top_level_load_state_dict(live, sd_a, sd_b, expected, x):
    def change(m):
        m.load_state_dict(sd_b)
        m.codec_setup()
    _coherent_after(live, sd_a, expected, x, change, moved=("bytes", "y", "vq_indices", "image"))


# what each child feeds: the encoder side shows in the latent or the bytes, the entropy side in the bytes, the decoder side in the image
_CHILD_MOVES = {"encoder": ("y", "bytes"), "decoder": ("image",), "hyperencoder": ("bytes",), "hyperdecoder": ("bytes",),
                "entropy_model_z": ("bytes",), "vq_estimator": ("image",), "vq_model": ("vq_indices", "y", "image"),
                "fusion_module": ("image",), "context_model": ("bytes",)}


@pytest.mark.parametrize("child", CHILDREN)
def test_child_load_state_dict(live, sd_a, sd_b, expected, x, child):
    def change(m):
        getattr(m, child).load_state_dict(_sub(sd_b, child))
        if child == "entropy_model_z":
            m.codec_setup()                                            # its integer tables are the caller's to rebuild
    _coherent_after(live, sd_a, expected, x, change, moved=_CHILD_MOVES[child])


# ------------------------------------------------------------------------------ in place, one parameter per cache site
def _bump(p, std=None):
    """A bias-like vector times 1.25; a matrix / kernel plus noise of its own scale (or of `std`)."""
    with torch.no_grad():
        if p.dim() == 1:
            p.mul_(1.25)
        else:
            noise = torch.randn(p.shape, generator=torch.Generator().manual_seed(77)) * (float(p.std()) if std is None else std)
            p.add_(noise.to(p.device))


_LAST_SWIN = "vq_estimator.swin_blks.2.residual_group.blocks.2"       # (the synthetic config: 3 RSTBs of 3 blocks)
# The reconstruction sees the estimator only through its argmax over 256 logits at the 2 x 8 x 8 latent positions.  The synthetic bias
# table has std 0.02 against attention logits of order 1: noise of the table's own scale moves the logits by ~1e-3 of their spread and
# flips no index, so the image would not show it.  This one parameter gets noise of the scale of the attention logits it is added to.
_NOISE_STD = {_LAST_SWIN + ".attn.relative_position_bias_table": 1.0}
IN_PLACE = [
    # (parameter, what it feeds, the copy of it that the path reads)
    ("encoder.conv1.weight", ("y", "bytes"), "packed plan, enc graph"),
    ("encoder.beta_ft_list.0.scale.weight", ("y", "bytes"), "_vec_cache, encode side"),
    ("encoder.mlp.0.weight", ("y", "bytes"), "_vec_cache, encode side"),
    ("decoder.init_fuse.shift.weight", ("image",), "_vec_cache, decode side"),
    ("vq_model.encoder.mid.attn_1.q.weight", ("y",), "fused qkv pack, enc graph"),
    ("vq_model.encoder.mid.attn_1.v.bias", ("y",), "fused qkv pack, enc graph"),
    ("vq_model.decoder.mid.attn_1.q.weight", ("image",), "fused qkv pack, dec graph"),
    ("vq_model.decoder.mid.attn_1.v.bias", ("image",), "fused qkv pack, dec graph"),
    ("vq_model.quantize.embedding.weight", ("y", "image"), "the codebook, both graphs"),
    ("vq_model.post_quant_conv.weight", ("image",), "the index -> latent LUT's matrix"),
    ("vq_model.decoder.up.1.upsample.conv.weight", ("image",), "sub-pixel phase packs, Winograd route packs"),
    ("context_model.mean_slice_transforms.1.model.0.weight", ("bytes",), "_rest_plan, _hyper_partials"),
    ("context_model.mean_slice_transforms.1.model.0.bias", ("bytes",), "_rest_plan reads it in place"),
    ("context_model.mean_slice_transforms.1.model.2.weight", ("bytes",), "packed plan, eager"),
    ("hyperdecoder.hd_mu.conv2.weight", ("bytes",), "packed plan, eager"),
    ("fusion_module.fusion_modules.block_1_4.scale.0.weight", ("image",), "packed plan, dec graph"),
    (_LAST_SWIN + ".attn.relative_position_bias_table", ("image",), "read in place, dec graph"),
    (_LAST_SWIN + ".norm2.weight", ("image",), "read in place, dec graph"),
]


def _param(m, name):
    mod_name, leaf = name.rsplit(".", 1)
    return m.get_submodule(mod_name), leaf


@pytest.mark.parametrize("name,moved,site", IN_PLACE, ids=[c[0] for c in IN_PLACE])
def test_in_place_update(live, sd_a, expected, x, name, moved, site):
    def change(m):
        mod, leaf = _param(m, name)
        _bump(getattr(mod, leaf), _NOISE_STD.get(name))
    _coherent_after(live, sd_a, expected, x, change, moved=moved)


@pytest.mark.parametrize("name", ["encoder.beta_ft_list.0.scale.weight", "encoder.mlp.0.weight", "decoder.init_fuse.shift.weight"])
def test_beta_vector_cache_on_the_eager_path(live, sd_a, expected, x, name):
    """The beta vectors are cached on the eager path too (DCVIC_GRAPHS=0): the same three updates with the graphs off."""
    g = live._graphs
    was = g.disabled
    try:
        live.load_state_dict(sd_a)
        g.disabled = True
        before = _run(live, x)
        mod, leaf = _param(live, name)
        _bump(getattr(mod, leaf))
        after = _run(live, x)
        assert all(_same(after, expected(live.state_dict())).values())
        assert not _same(after, before)["image" if name.startswith("decoder") else "y"]
    finally:
        g.disabled = was
        live.load_state_dict(sd_a)


# ------------------------------------------------------------------------------ a parameter replaced by a new one
@pytest.mark.parametrize("name,moved", [("encoder.conv2.weight", ("y", "bytes")), ("encoder.beta_ft_list.2.shift.weight", ("y", "bytes"))])
def test_parameter_replacement(live, sd_a, expected, x, name, moved):
    """`mod.weight = nn.Parameter(new)`: a new storage whose version starts at 0 again."""
    def change(m):
        mod, leaf = _param(m, name)
        old = getattr(mod, leaf)
        noise = torch.randn(old.shape, generator=torch.Generator().manual_seed(78)) * float(old.std())
        setattr(mod, leaf, nn.Parameter(old.detach() + noise.to(DEV), requires_grad=False))
        assert getattr(mod, leaf)._version == 0 and getattr(mod, leaf).data_ptr() != old.data_ptr()
    _coherent_after(live, sd_a, expected, x, change, moved=moved)


# ------------------------------------------------------------------------------ writes torch does not version
def _raw_write(m):
    for sub in (m.decoder, m.context_model):
        for p in sub.parameters():
            v = p._version
            p.data.mul_(1.02)
            assert p._version == v


def test_data_write_then_invalidate(live, sd_a, expected, x):
    """`p.data.mul_()` on every parameter of the ELIC decoder and of CHARM: no (storage, version) key moves, so the one public call is
    needed, and after it everything is rebuilt from the new values."""
    def change(m):
        _raw_write(m)
        m.invalidate_weight_caches()
    _coherent_after(live, sd_a, expected, x, change, moved=("bytes", "image"))


def test_data_write_without_the_call_is_unsupported(live, sd_a, x):
    """The same write WITHOUT invalidate_weight_caches(), on a model whose graphs are off: UNSUPPORTED.  `p._version` does not move under
    `p.data` (nor under a kernel writing through the raw pointer), so the packed plans and cached beta vectors keep their keys and the
    result mixes old copies with new values.  Nothing is asserted about the values: the call runs, and the documented remedy brings the
    model back."""
    g = live._graphs
    was = g.disabled
    try:
        live.load_state_dict(sd_a)
        g.disabled = True
        _run(live, x)
        _raw_write(live)
        out = _run(live, x)
        assert out["image"].shape == (2, 3, 64, 64)
        live.invalidate_weight_caches()
    finally:
        g.disabled = was
        live.load_state_dict(sd_a)
