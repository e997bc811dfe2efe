"""The VQ search kernels and the argmax -> codebook LUT kernel (csrc/vq.hip) on a real MI355X against tests/vq_ref.py, bit for bit.

Every operation of these kernels is one IEEE fp32 operation in an order the source fixes, so the CPU restatement is equal to the kernel and
every comparison here is torch.equal: zero mismatches, no tolerance.  Each search case of vq_ref.CASES
  * calls dcvic_vq_argmin_f32 directly, its outputs inside sentinel-filled buffers with 64 guard elements on either side, a codebook view
    that is 16-byte aligned or one float off as the case says, and DCVIC_VQ_KERNEL as the case says;
  * asserts through dcvic_vq_last_variant() that it reached the kernel the table names (vq_ref.variant_of restates the dispatcher);
  * compares idx, zq and feat = cat[zq, one_hot] with the restatement, checks the guards, and reruns for equal bits;
  * runs every other variant that accepts the same input (forced shard / lds) for the same bits, and for the 4-vectors-per-lane kernel
    the last image alone (2 vectors per lane) against the last image of the batch.
The regimes (model, grid, cancel, hits, zeros) and the duplicated rows that put a tied minimum across every structural boundary of the
kernels are vq_ref's; tests/test_vq_host.py shows that the table notices a last-minimum rule, a group resolved to its offset 0 and a
merge of the lane groups by distance alone.

Out of scope, and deliberately not pinned: NaN or Inf in z, and NaN logits.  torch.argmin / argmax return the NaN's index; the kernels'
`<` / `>` scans skip NaNs.

With DCVIC_TEST_RATIOS=<file> the variant, the vector count, the mismatch count and the share of tied vectors of every search case are
written there (profiles/vq_exact.json)."""
import os

import pytest
import torch
import torch.nn.functional as F

import vq_ref as R
from kernel_bounds import DEV, ratios_mark, write_ratios

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = {"cases": {}, "argmax_lut": {}}
GUARD = 64
SENT_F, SENT_I = -12345.0, -7


@pytest.fixture(scope="module", autouse=True)
def _report():
    mark = ratios_mark()
    yield
    write_ratios(EXTRA, since=mark)


def Lib():
    from dc_vic_amd._lib import lib
    return lib()


def t(a):
    """A torch copy of a (read-only, shared) numpy array."""
    return torch.tensor(a)


def guarded(n, dtype):
    """A device buffer of GUARD + n + GUARD sentinels; the kernel gets the address of element GUARD."""
    return torch.full((n + 2 * GUARD,), SENT_I if dtype == torch.int64 else SENT_F, dtype=dtype, device=DEV)


def ptr(buf):
    return None if buf is None else buf.data_ptr() + GUARD * buf.element_size()


def body(buf, shape):
    return buf[GUARD:buf.numel() - GUARD].reshape(shape)


def guards_intact(buf):
    s = SENT_I if buf.dtype == torch.int64 else SENT_F
    return bool((buf[:GUARD] == s).all()) and bool((buf[buf.numel() - GUARD:] == s).all())


def untouched(buf):
    return bool((buf == (SENT_I if buf.dtype == torch.int64 else SENT_F)).all())


def codebook_on_device(cb, aligned):
    """The codebook as a device view whose base is 16-byte aligned, or one float past such an address."""
    flat = torch.empty(cb.size + 4, dtype=torch.float32, device=DEV)
    off = 0 if aligned else 1
    v = flat[off:off + cb.size]
    v.copy_(t(cb).reshape(-1))
    assert (v.data_ptr() % 16 == 0) == aligned
    return v


def search(z_d, cb_d, N, D, HW, n_e, want_zq=True, want_feat=True, force=None):
    """One call of the C entry point -> (rc, idx, zq, feat buffers with their guards, the variant reached)."""
    idx = guarded(N * HW, torch.int64)
    zq = guarded(N * D * HW, torch.float32) if want_zq else None
    feat = guarded(N * (D + n_e) * HW, torch.float32) if want_feat else None
    old = os.environ.pop("DCVIC_VQ_KERNEL", None)
    if force:
        os.environ["DCVIC_VQ_KERNEL"] = force
    try:
        rc = Lib().dcvic_vq_argmin_f32(z_d.data_ptr(), cb_d.data_ptr(), ptr(idx), ptr(zq), ptr(feat), N, D, HW, n_e,
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("DCVIC_VQ_KERNEL", None)
        if old is not None:
            os.environ["DCVIC_VQ_KERNEL"] = old
    return rc, idx, zq, feat, int(Lib().dcvic_vq_last_variant())


def same_input_variants(c):
    """(force, variant) of every other kernel that accepts the case's input."""
    out = []
    for force in (None, "shard", "lds"):
        v = R.variant_of(c["N"], c["D"], c["HW"], c["n_e"], c["aligned"], force)
        if v not in ("EINVAL", c["variant"]) and v not in [o[1] for o in out]:
            out.append((force, v))
    return out


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_vq_search_bit_exact(c):
    N, D, HW, n_e = c["N"], c["D"], c["HW"], c["n_e"]
    ref = R.case_reference(c)
    z_d = t(ref["z"]).to(DEV)
    cb_d = codebook_on_device(ref["cb"], c["aligned"])
    want = {k: t(ref[k]) for k in ("idx", "zq", "feat")}
    rc, idx, zq, feat, v = search(z_d, cb_d, N, D, HW, n_e, force=c["force"])
    assert rc == 0, Lib().dcvic_last_error()
    assert v == R.VARIANT_CODE[c["variant"]], f"{c['id']}: reached variant {v}, the table says {c['variant']}"
    got = {"idx": body(idx, (N, HW)).cpu(), "zq": body(zq, (N, D, HW)).cpu(), "feat": body(feat, (N, D + n_e, HW)).cpu()}
    mism = int((got["idx"] != want["idx"]).sum())
    EXTRA["cases"][c["id"]] = {"variant": c["variant"], "vectors": N * HW, "mismatches": mism, "tied": round(ref["tied"], 4)}
    print(f"{c['id']}: variant {v}, {N * HW} vectors, {mism} mismatches, tied share {ref['tied']:.4f}")
    assert mism == 0, f"{c['id']}: {mism} of {N * HW} indices differ from the restatement, first at {(got['idx'] != want['idx']).nonzero()[0].tolist()}"
    for k in ("idx", "zq", "feat"):
        assert torch.equal(got[k], want[k]), f"{c['id']}: {k} differs from the restatement"
    for b in (idx, zq, feat):
        assert guards_intact(b), f"{c['id']}: wrote outside its output"
    rc2, idx2, zq2, feat2, _ = search(z_d, cb_d, N, D, HW, n_e, force=c["force"])
    assert rc2 == 0 and torch.equal(idx2, idx) and torch.equal(zq2, zq) and torch.equal(feat2, feat), f"{c['id']}: a rerun differs"
    for force, other in same_input_variants(c):
        rc3, idx3, zq3, feat3, v3 = search(z_d, cb_d, N, D, HW, n_e, force=force)
        assert rc3 == 0 and v3 == R.VARIANT_CODE[other], (c["id"], force, v3)
        assert torch.equal(idx3, idx) and torch.equal(zq3, zq) and torch.equal(feat3, feat), f"{c['id']}: {other} differs from {c['variant']}"
    if c["variant"] == "packed2":                                       # the same image alone: 2 vectors per lane
        one = z_d[N - 1:].contiguous()
        rc4, idx4, zq4, feat4, v4 = search(one, cb_d, 1, D, HW, n_e)
        assert rc4 == 0 and v4 == R.VARIANT_CODE["packed1"]
        assert torch.equal(body(idx4, (1, HW))[0], body(idx, (N, HW))[N - 1]) and torch.equal(body(zq4, (1, D, HW))[0], body(zq, (N, D, HW))[N - 1])
        assert torch.equal(body(feat4, (1, D + n_e, HW))[0], body(feat, (N, D + n_e, HW))[N - 1]), f"{c['id']}: packed1 differs from packed2"


def _first(variant):
    """The first case of a variant with three images and a ragged pixel count (packed2: its smallest)."""
    for c in R.CASES:
        if c["variant"] == variant and (variant == "packed2" or (c["N"] == 3 and c["HW"] > 16 and c["HW"] % 16 and c["n_e"] > 1)):
            return c
    raise KeyError(variant)


@pytest.mark.parametrize("variant", ["lds4", "lds8", "packed1", "packed2", "shard"])
def test_vq_nullable_outputs_and_guards(variant):
    """All four zq / feat combinations: what is asked for equals the restatement, and nothing else is written -- neither the guards
    around each output nor, with an output absent, anything at all for it."""
    c = _first(variant)
    N, D, HW, n_e = c["N"], c["D"], c["HW"], c["n_e"]
    ref = R.case_reference(c)
    z_d = t(ref["z"]).to(DEV)
    cb_d = codebook_on_device(ref["cb"], c["aligned"])
    for want_zq in (False, True):
        for want_feat in (False, True):
            rc, idx, zq, feat, v = search(z_d, cb_d, N, D, HW, n_e, want_zq, want_feat, force=c["force"])
            what = f"{c['id']} zq={want_zq} feat={want_feat}"
            assert rc == 0 and v == R.VARIANT_CODE[variant], what
            assert guards_intact(idx) and torch.equal(body(idx, (N, HW)).cpu(), t(ref["idx"])), what
            assert (zq is None) == (not want_zq) and (feat is None) == (not want_feat)
            if want_zq:
                assert guards_intact(zq) and torch.equal(body(zq, (N, D, HW)).cpu(), t(ref["zq"])), what
            if want_feat:
                assert guards_intact(feat) and torch.equal(body(feat, (N, D + n_e, HW)).cpu(), t(ref["feat"])), what


def test_vq_refusals_write_nothing():
    """Each refused call returns the error, launches nothing and leaves every output as it was."""
    L = Lib()
    for what, N, D, HW, n_e in R.REFUSED:
        z_d = torch.zeros(N * D * HW, dtype=torch.float32, device=DEV)
        cb_d = torch.zeros(n_e * D, dtype=torch.float32, device=DEV)
        rc, idx, zq, feat, v = search(z_d, cb_d, N, D, HW, n_e, want_feat=n_e * HW < 10 ** 6)
        assert rc == -1 and b"vq_argmin" in L.dcvic_last_error(), what
        assert v == 0 and untouched(idx) and untouched(zq) and (feat is None or untouched(feat)), what
        assert R.variant_of(N, D, HW, n_e) == "EINVAL"
    lg = torch.zeros(2 * 256 * 16, dtype=torch.float32, device=DEV)
    cb, w, b = (torch.zeros(n, dtype=torch.float32, device=DEV) for n in (1024, 16, 4))
    idx, lat = guarded(32, torch.int64), guarded(2 * 4 * 16, torch.float32)
    s = torch.cuda.current_stream().cuda_stream
    assert L.dcvic_argmax_lut_f32(lg.data_ptr(), None, None, cb.data_ptr(), w.data_ptr(), b.data_ptr(), 2, 256, 4, 16, s) == -1
    assert b"argmax_lut" in L.dcvic_last_error()
    assert L.dcvic_argmax_lut_f32(lg.data_ptr(), ptr(idx), ptr(lat), None, w.data_ptr(), b.data_ptr(), 2, 256, 4, 16, s) == -1
    assert b"argmax_lut" in L.dcvic_last_error() and b"codebook" in L.dcvic_last_error()
    torch.cuda.synchronize()
    assert untouched(idx) and untouched(lat)


@pytest.mark.parametrize("c", R.LUT_CASES, ids=[c["id"] for c in R.LUT_CASES])
def test_argmax_lut_bit_exact(c):
    """Every input kind (plateaus of equal maxima, all logits equal, all -inf, one +inf, +0.0 against -0.0) x every output combination
    (idx only, latent only, both) x with and without the bias: the index is the first maximum, the latent the restated fma chain."""
    L = Lib()
    N, HW, n_e, D = c["N"], c["HW"], c["n_e"], c["D"]
    cb, w, bias = R.lut_weights(c)
    cb_d, w_d, b_d = (torch.from_numpy(a).to(DEV) for a in (cb, w, bias))
    s = torch.cuda.current_stream().cuda_stream
    for kind in R.LUT_KINDS:
        x = R.lut_logits(c, kind)
        x_d = torch.from_numpy(x).to(DEV)
        ref_idx, ref_b = R.argmax_lut_ref(x, cb, w, bias)
        _, ref_nb = R.argmax_lut_ref(x, cb, w, None)
        plateau = float(((x == x.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean())
        EXTRA["argmax_lut"][f"{c['id']}/{kind}"] = {"vectors": N * HW, "tied": round(plateau, 4)}
        for want_idx, want_lat in ((True, False), (False, True), (True, True)):
            for with_bias in (True, False):
                what = f"{c['id']} {kind} idx={want_idx} latent={want_lat} bias={with_bias}"
                idx = guarded(N * HW, torch.int64) if want_idx else None
                lat = guarded(N * D * HW, torch.float32) if want_lat else None
                rc = L.dcvic_argmax_lut_f32(x_d.data_ptr(), ptr(idx), ptr(lat), cb_d.data_ptr(), w_d.data_ptr(),
                                            b_d.data_ptr() if with_bias else None, N, n_e, D, HW, s)
                torch.cuda.synchronize()
                assert rc == 0, (what, L.dcvic_last_error())
                if want_idx:
                    assert guards_intact(idx) and torch.equal(body(idx, (N, HW)).cpu(), torch.from_numpy(ref_idx)), what
                if want_lat:
                    assert guards_intact(lat), what
                    assert torch.equal(body(lat, (N, D, HW)).cpu(), torch.from_numpy(ref_b if with_bias else ref_nb)), what


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    opt = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV})
    m = build_comp_model(opt)
    load_synth_weights(m, 1234)
    m.codec_setup()
    return m


class _Capture(torch.nn.Module):
    """Stands in for the analysis transform: hands back the feature it was given."""

    def forward(self, x, feat, **kw):
        return feat


@pytest.mark.parametrize("duplicate_row", [False, True], ids=["synthetic", "row200_is_row7"])
def test_given_indices_make_the_one_hot_feature(model, monkeypatch, duplicate_row):
    """The encoder's one-hot feature is F.one_hot of the indices it was GIVEN (the reference's hyperprior_vic_model.py:268-271), for
    every code j, through vq_encode(x, vq_indices=idx) and comp_encode(..., feat=None) -- also where a later codebook row equals an
    earlier one, where a search of the gathered latent would return the earlier row."""
    w = model.vq_model.quantize.embedding.weight
    n_e, D = w.shape
    saved = w.data.clone()
    try:
        if duplicate_row:
            w.data[200] = w.data[7]
            model.invalidate_weight_caches()
        idx = torch.arange(n_e, device=DEV).reshape(1, 16, n_e // 16)
        x = torch.zeros((1, 3, 256, 16 * (n_e // 16)), device=DEV)
        want = F.one_hot(idx, n_e).permute(0, 3, 1, 2).float()
        zq, idx_out, feat = model.vq_encode(x, vq_indices=idx, want_feat=True)
        assert torch.equal(idx_out, idx) and torch.equal(zq, w.data[idx].permute(0, 3, 1, 2))
        wrong = (feat[:, D:] != want).any(dim=1).nonzero()
        assert wrong.numel() == 0, f"vq_encode: the one-hot feature differs from the given indices at codes {idx[0][wrong[:, 1], wrong[:, 2]].tolist()}"
        assert torch.equal(feat[:, :D], zq)
        monkeypatch.setattr(model, "encoder", _Capture())
        feat2 = model.comp_encode(x, zq, idx, feat=None)
        wrong = (feat2[:, D:] != want).any(dim=1).nonzero()
        assert wrong.numel() == 0, f"comp_encode: the one-hot feature differs from the given indices at codes {idx[0][wrong[:, 1], wrong[:, 2]].tolist()}"
        assert torch.equal(feat2[:, :D], zq)
    finally:
        monkeypatch.undo()
        w.data.copy_(saved)
        model.invalidate_weight_caches()
