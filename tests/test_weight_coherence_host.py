"""Weight coherence, host side (no GPU): the Python logic that decides whether a copy of the weights -- a packed plan, a cached beta
vector, a captured hipGraph -- may still be used.  The model is built on the CPU; nothing here launches a kernel.

 * layers.WeightFingerprint moves under every route torch versions and stays put under reads -- and under `p.data` writes, the
   documented limitation that invalidate_weight_caches() exists for;
 * invalidate_weight_caches() empties every weight-derived cache of the package;
 * _GraphCache.run drops an entry whose weights moved and sends its key back through the sighting / capture policy;
 * _BetaCond empties its vector cache when mlp or a scale/shift module moved, and keeps the per-beta-pair reuse otherwise;
 * one validity check costs less than 2 % of the recorded N = 1 latencies."""
import json
import os
import time

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILDREN = ("encoder", "decoder", "hyperencoder", "hyperdecoder", "entropy_model_z", "vq_estimator", "vq_model", "fusion_module",
            "context_model")


@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": "cpu"})
    return build_comp_model(opt)


def _fp(*modules):
    from dc_vic_amd.layers import WeightFingerprint
    return WeightFingerprint(modules)


def test_segments_cover_every_parameter_their_code_reads(model):
    """The two graph segments' module lists, against the model's children: everything but the entropy side (hyperprior, CHARM, the two
    entropy models), which runs eagerly around the graphs, and split over "enc" / "dec" as compress_batch / decompress_batch use them."""
    own = lambda mods: {id(p) for m in mods for p in m.parameters()}
    enc, dec = own(model._segment_modules("enc")), own(model._segment_modules("dec"))
    eager = own([model.hyperencoder, model.hyperdecoder, model.entropy_model_z, model.entropy_model_y, model.context_model])
    assert enc | dec | eager == own([model])
    assert not (enc & eager) and not (dec & eager)
    assert enc & dec == own([model.vq_model.quantize])            # the codebook: VQ argmin on one side, the index -> latent LUT on the other
    assert own([model.encoder, model.vq_model.encoder, model.vq_model.quant_conv]) <= enc
    assert own([model.decoder, model.vq_estimator, model.fusion_module, model.vq_model.decoder, model.vq_model.post_quant_conv]) <= dec


def test_fingerprint_moves_under_every_versioned_route(model):
    w = _fp(model)
    # top-level load_state_dict
    a = w()
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    b = w()
    assert a != b
    # per child: its own fingerprint moves, a sibling's does not
    for name in CHILDREN:
        child = getattr(model, name)
        other = getattr(model, CHILDREN[(CHILDREN.index(name) + 1) % len(CHILDREN)])
        wc, wo = _fp(child), _fp(other)
        a, o = wc(), wo()
        child.load_state_dict({k: v.clone() for k, v in child.state_dict().items()})
        assert wc() != a, name
        assert wo() == o, name
    # in-place ops on one parameter
    p = model.encoder.conv1.weight
    we = _fp(model.encoder)
    with torch.no_grad():
        a = we()
        p.copy_(torch.zeros_like(p))
        b = we()
        p.add_(1.0)
        c = we()
        p.mul_(1.25)
        d = we()
    assert len({a, b, c, d}) == 4
    # replacement: a new storage at version 0
    old = model.encoder.conv1.weight
    try:
        model.encoder.conv1.weight = nn.Parameter(old.detach().clone(), requires_grad=False)
        assert model.encoder.conv1.weight._version == 0
        e = we()
        assert e != d
        # a buffer replaced by assignment (the entropy models' tables are)
        wz, off = _fp(model.entropy_model_z), model.entropy_model_z._offset
        a = wz()
        model.entropy_model_z._offset = torch.zeros(3, dtype=torch.int32)
        assert wz() != a
    finally:
        model.encoder.conv1.weight = old
        model.entropy_model_z._offset = off
    # `p.data = other`: same Parameter, same version, another storage (what train.ParamGroup does)
    a = we()
    keep = p.data
    p.data = keep.clone()
    assert we() != a
    p.data = keep
    assert we() == a


def test_fingerprint_stays_put_under_reads_and_under_data_writes(model):
    w = _fp(model)
    a = w()
    model.state_dict()
    list(model.parameters())
    list(model.named_modules())
    list(model.buffers())
    {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert w() == a and w() == a
    # THE LIMITATION: torch does not version a write through .data (nor one through the raw pointer, which looks the same from here), so
    # no (storage, version) key can see it.  This route needs invalidate_weight_caches(); the trainer's fused Adam step is one.
    p = model.decoder.conv1.weight
    v = p._version
    p.data.copy_(torch.ones_like(p))
    p.data.mul_(0.5)
    assert p._version == v
    assert w() == a
    assert float(p.detach().flatten()[0]) == 0.5               # ... although the values did change


def _cache_sites(model):
    """(module, attribute) of every weight-derived cache the package keeps on a module, by the issue's list.  `_plain_plan` and `_dgrad`
    are set lazily by train/autograd.conv on convolution layers, `_rest*` / `_hp*` lazily by charm.py: seeded where they would appear."""
    from dc_vic_amd.charm import Minnen20CharmContextModel, SliceTransform
    from dc_vic_amd.elic import _BetaCond
    from dc_vic_amd.entropy import EntropyBottleneck
    from dc_vic_amd.layers import _Packed
    from dc_vic_amd.vqgan import AttnBlock
    sites = []
    for m in model.modules():
        if isinstance(m, _Packed):
            sites += [(m, "_plan"), (m, "_plain_plan"), (m, "_dgrad")]
        if isinstance(m, AttnBlock):
            sites.append((m, "_qkv_plan"))
        if isinstance(m, SliceTransform):
            sites += [(m, "_rest_key"), (m, "_rest")]
        if isinstance(m, Minnen20CharmContextModel):
            sites += [(m, "_hp_key"), (m, "_hp_mean"), (m, "_hp_scale")]
        if isinstance(m, EntropyBottleneck):
            sites.append((m, "_packs"))
        if isinstance(m, _BetaCond):
            sites.append((m, "_vec_cache"))
    return sites


@pytest.mark.parametrize("caller", ["invalidate_weight_caches", "load_state_dict", "refresh_plans", "function_on_child"])
def test_invalidation_empties_every_cache(model, caller):
    """Every cache attribute seeded with a sentinel reads as empty after the one entry point -- called directly, through the top-level
    load_state_dict, through ParamGroup.refresh_plans, and as the module-level function on a child.  A cache added to the package without
    a line in layers.WEIGHT_CACHE_ATTRS fails the last assertions (every `*_key`-guarded, `*_plan`, `*_cache` or `*_packs` attribute of the
    model's modules must be listed)."""
    from dc_vic_amd.layers import WEIGHT_CACHE_ATTRS, invalidate_weight_caches
    sentinel = object()
    sites = _cache_sites(model)
    kinds = {a for _, a in sites}
    assert kinds == {"_plan", "_plain_plan", "_dgrad", "_qkv_plan", "_vec_cache", "_rest_key", "_rest", "_hp_key", "_hp_mean", "_hp_scale",
                     "_packs"}
    assert kinds - {"_vec_cache"} == set(WEIGHT_CACHE_ATTRS)
    scope = model.vq_model if caller == "function_on_child" else model
    inside = {id(m) for m in scope.modules()}
    try:
        for m, a in sites:
            if a == "_vec_cache":
                m._vec_cache[(1.0, 2.0, "cpu")] = sentinel
            else:
                setattr(m, a, sentinel)
        model._graphs.entries["k"] = sentinel
        model._graphs.seen["k"] = 1
        if caller == "invalidate_weight_caches":
            model.invalidate_weight_caches()
        elif caller == "load_state_dict":
            model.load_state_dict(model.state_dict())
        elif caller == "refresh_plans":
            from dc_vic_amd.train.autograd import ParamGroup
            grp = ParamGroup.__new__(ParamGroup)          # (the constructor moves the parameters into a flat device buffer: not needed here)
            grp.modules = [model]
            grp.refresh_plans()
        else:
            invalidate_weight_caches(model.vq_model)
        for m, a in sites:
            v = getattr(m, a)
            if id(m) not in inside:
                assert v is sentinel or v == {(1.0, 2.0, "cpu"): sentinel}, (type(m).__name__, a)      # out of scope: untouched
            elif a == "_vec_cache":
                assert v == {}, type(m).__name__
            else:
                assert v is None, (type(m).__name__, a)
        if scope is model:
            assert not model._graphs.entries and not model._graphs.seen
        else:
            assert model._graphs.entries["k"] is sentinel
    finally:
        for m, a in sites:
            if a == "_vec_cache":
                m._vec_cache.clear()
            else:
                setattr(m, a, None)
        model._graphs.clear()
    # no module of the model keeps a key-guarded cache under a name the entry point does not know
    guards = {"_plan_key": "_plan", "_qkv_key": "_qkv_plan", "_packs_key": "_packs", "_rest_key": "_rest_key", "_hp_key": "_hp_key"}
    for m in model.modules():
        for a in m.__dict__:
            if a.endswith("_key"):
                assert guards.get(a) in WEIGHT_CACHE_ATTRS, (type(m).__name__, a)
            elif a.endswith(("_plan", "_cache", "_packs")):
                assert a in WEIGHT_CACHE_ATTRS or a == "_vec_cache", (type(m).__name__, a)


class _FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


def test_graph_cache_drops_an_entry_whose_weights_moved(model):
    """_GraphCache.run with a stand-in for the captured graph: replayed while the segment's fingerprint matches, dropped when it does not,
    and the key then starts again at its first sighting (eager) instead of ending in `disabled`."""
    from dc_vic_amd.comp_model import _GraphCache
    from dc_vic_amd.layers import WeightFingerprint
    g = _GraphCache()
    g.disabled = False
    assert g.capture_after == 2
    mods = model._segment_modules("dec")
    calls = []

    def eager(x):
        calls.append(1)
        return x + 1

    def seed(key):
        fake, watch = _FakeGraph(), WeightFingerprint(mods)
        g.entries[key] = (fake, [torch.zeros(2)], "replayed", None, watch, watch())
        g.seen[key] = 2
        return fake

    x = torch.ones(2)
    fake = seed("k")
    other = seed("other")
    assert g.run("k", eager, [x], modules=mods) == "replayed" and fake.replays == 1 and not calls
    assert torch.equal(g.entries["k"][1][0], x)                   # the input went into the static buffer
    model.state_dict(); list(model.parameters())
    assert g.run("k", eager, [x], modules=mods) == "replayed" and fake.replays == 2
    p = model.fusion_module.fusion_modules["block_1_4"].scale[0].weight
    with torch.no_grad():
        p.add_(0.0)                                                # same values, new version: torch cannot tell, so neither do we
    out = g.run("k", eager, [x], modules=mods)
    assert torch.equal(out, x + 1) and calls == [1] and fake.replays == 2
    assert "k" not in g.entries and g.seen["k"] == 1 and not g.disabled
    assert "other" in g.entries                                    # dropped when it is next asked for, not before
    assert torch.equal(g.run("other", eager, [x], modules=mods), x + 1) and other.replays == 0 and "other" not in g.entries
    # a weight of the OTHER segment does not drop this one
    fake = seed("k2")
    with torch.no_grad():
        model.encoder.conv1.weight.add_(0.0)
        model.context_model.mean_slice_transforms[0].model[0].weight.add_(0.0)
    assert g.run("k2", eager, [x], modules=mods) == "replayed" and fake.replays == 1


def test_beta_vector_cache_follows_its_weights(model):
    """_BetaCond._vec_cache_current (called by beta_vectors before the lookup): the cache survives calls while mlp and the scale/shift
    modules passed in are unchanged -- the per-beta-pair reuse -- and is emptied when any of them moved."""
    sentinel = object()
    key = (1.0, 2.0, "cpu")
    for net, mods in ((model.encoder, list(model.encoder.beta_ft_list)),
                      (model.decoder, [model.decoder.init_fuse] + list(model.decoder.beta_ft_list))):
        net._vec_cache_current(mods)
        net._vec_cache[key] = sentinel
        for _ in range(3):
            net._vec_cache_current(mods)
            net.state_dict()
            assert net._vec_cache.get(key) is sentinel
        targets = [net.mlp[0].weight, net.mlp[2].bias, mods[0].scale.weight, mods[0].shift.bias, mods[-1].shared[0].weight]
        for p in targets:
            with torch.no_grad():
                p.mul_(1.0)
            net._vec_cache_current(mods)
            assert not net._vec_cache
            net._vec_cache[key] = sentinel
            net._vec_cache_current(mods)
            assert net._vec_cache.get(key) is sentinel
        # a child's load_state_dict, and a replaced parameter
        net.load_state_dict(net.state_dict())
        net._vec_cache_current(mods)
        assert not net._vec_cache
        net._vec_cache[key] = sentinel
        old = mods[1].scale.weight
        try:
            mods[1].scale.weight = nn.Parameter(old.detach().clone(), requires_grad=False)
            net._vec_cache_current(mods)
            assert not net._vec_cache
        finally:
            mods[1].scale.weight = old
        # a conv of the network that is NOT a conditioning weight leaves the vectors alone
        net._vec_cache_current(mods)
        net._vec_cache[key] = sentinel
        with torch.no_grad():
            net.conv1.weight.mul_(1.0)
        net._vec_cache_current(mods)
        assert net._vec_cache.get(key) is sentinel
        net._vec_cache.clear()


def test_validity_check_costs_under_two_percent_of_the_n1_latency(model):
    """Host cost of one graph validity check (WeightFingerprint over the segment's modules + the tuple comparison), per segment of the
    synthetic model, against 2 % of the recorded N = 1 256x256 latencies (profiles/r3_latency_n1.json: compress 10.41 ms -> 0.21 ms,
    decompress 19.26 ms -> 0.39 ms) -- the graphs exist to save launch overhead, the check must not hand it back.  Timed with
    perf_counter over 1 000 calls, best of three such runs (the cost of the check, not of whatever else the machine was doing).
    Measured on the development host (CPU tensors): enc 327 tensors 100 us, dec 594 tensors 190 us per check."""
    from dc_vic_amd.layers import WeightFingerprint
    with open(os.path.join(ROOT, "profiles", "r3_latency_n1.json")) as f:
        rec = json.load(f)["256x256"]
    assert abs(rec["compress_ms"] - 10.41) < 0.01 and abs(rec["decompress_ms"] - 19.26) < 0.01
    for seg, total_ms, bound_ms in (("enc", rec["compress_ms"], 0.21), ("dec", rec["decompress_ms"], 0.39)):
        assert abs(0.02 * total_ms - bound_ms) < 0.005
        watch = WeightFingerprint(model._segment_modules(seg))
        then = watch()
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(1000):
                ok = watch() == then
            best = min(best, (time.perf_counter() - t0) / 1000)
        assert ok
        print(f"{seg}: {len(then[0])} tensors, {best * 1e6:.1f} us per validity check (bound {bound_ms * 1e3:.0f} us)")
        assert best * 1e3 < bound_ms, (seg, best * 1e3)
