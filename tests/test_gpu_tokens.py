"""The two kernels of csrc/tokens.hip on a real MI355X against tests/tokens_ref.py, bit for bit, and vq_encode's token route.

Both kernels move bytes (a table lookup, a codebook row, a one-hot): every comparison is torch.equal.  The entry points are called
directly with their outputs inside sentinel-filled buffers (64 guard elements on either side, as tests/test_gpu_vq.py does), then
through dc_vic_amd.ops, and vq_encode(x, tokens) against vq_indices_to_latent plus _index_feat."""
import os

import pytest
import torch

import tokens_ref as R
from kernel_bounds import DEV

pytestmark = pytest.mark.gpu
GUARD, SENT_F, SENT_I = R.GUARD, R.SENT_F, R.SENT_I


def Lib():
    from dc_vic_amd._lib import lib
    return lib()


def guarded(n, dtype=torch.float32):
    return torch.full((n + 2 * GUARD,), SENT_I if dtype == torch.int64 else SENT_F, dtype=dtype, device=DEV)


def ptr(buf):
    return None if buf is None else buf.data_ptr() + GUARD * buf.element_size()


def body(buf, shape):
    return buf[GUARD:buf.numel() - GUARD].reshape(shape)


def guards_intact(buf):
    s = SENT_I if buf.dtype == torch.int64 else SENT_F
    return bool((buf[:GUARD] == s).all()) and bool((buf[buf.numel() - GUARD:] == s).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------- kernel A
def run_a(src_view):
    """dcvic_u8_hwc_to_f32_nchw on a dense device view [N, H, W, 3], the output between guards; returns it on the host."""
    N, H, W, _ = src_view.shape
    assert src_view.is_contiguous()
    tab = R.table().to(DEV)
    out = guarded(N * 3 * H * W)
    assert Lib().dcvic_u8_hwc_to_f32_nchw(src_view.data_ptr(), N, H, W, tab.data_ptr(), ptr(out), stream()) == 0, Lib().dcvic_last_error()
    torch.cuda.synchronize()
    assert guards_intact(out)
    return body(out, (N, 3, H, W)).cpu()


@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 24, 40), (2, 7, 13), (2, 33, 64)])
def test_u8_hwc_to_f32_nchw_equals_the_table_expression(shape):
    """(2, 7, 13): items of 273 bytes, the second one starts on an odd address and ends in a group of 3 pixels.  (2, 33, 64): more than
    one workgroup per item."""
    src = R.u8_case(*shape, seed=sum(shape))
    dev = src.to(DEV)
    assert dev.data_ptr() % 4 == 0
    got = run_a(dev)
    assert torch.equal(got, R.table_expression(src)) and torch.equal(got, R.u8_hwc_to_f32_nchw_ref(src, R.table()))
    assert torch.equal(run_a(dev), got)                                          # two runs, equal bits
    assert torch.equal(run_a(dev[1:] if shape[0] > 1 else dev)[-1], got[-1])     # the last item alone


@pytest.mark.parametrize("shape", [(4, 12, 20), (4, 7, 13), (4, 9, 10)])
def test_u8_hwc_to_f32_nchw_on_a_slice_of_a_resident_array(shape):
    """[1:3] of a 4-item array: the slice starts at byte 720 (aligned), 273 (odd) and 270 (even, not a multiple of 4)."""
    src = R.u8_case(*shape, seed=3)
    dev = src.to(DEV)
    assert torch.equal(run_a(dev[1:3]), R.table_expression(src[1:3]))
    from dc_vic_amd import ops
    assert torch.equal(ops.u8_hwc_to_f32_nchw(dev[1:3], R.table().to(DEV)).cpu(), R.table_expression(src[1:3]))


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_u8_hwc_to_f32_nchw_on_a_view_inside_its_allocation(shift):
    """The source starts `shift` bytes into its allocation and ends with it: a load past the slice would leave the allocation."""
    src = R.u8_case(2, 8, 12, seed=shift)
    flat = torch.zeros(shift + src.numel(), dtype=torch.uint8, device=DEV)
    flat[shift:] = src.to(DEV).reshape(-1)
    view = flat[shift:].reshape(src.shape)
    assert view.data_ptr() % 4 == shift
    assert torch.equal(run_a(view), R.table_expression(src))


# ---------------------------------------------------------------------------------------------------- kernel B
def run_b(tokens, cb, want=(True, True, True), shift=0):
    """dcvic_vq_token_feat_f32 on device tokens / codebook with the wanted outputs between guards; the others null.  `shift`: every
    output starts that many elements past its 16-byte aligned place (the guards grow by as much)."""
    N, h, w = tokens.shape
    n_e, D = cb.shape
    sizes = (N * h * w, N * D * h * w, N * (D + n_e) * h * w)
    bufs = [guarded(n + shift, torch.int64 if k == 0 else torch.float32) if want[k] else None for k, n in enumerate(sizes)]
    at = [None if b is None else ptr(b) + shift * b.element_size() for b in bufs]
    rc = Lib().dcvic_vq_token_feat_f32(tokens.data_ptr(), tokens.element_size(), cb.data_ptr(), N, h, w, D, n_e, at[0], at[1], at[2], stream())
    assert rc == 0, Lib().dcvic_last_error()
    torch.cuda.synchronize()
    shapes = ((N, h, w), (N, D, h, w), (N, D + n_e, h, w))
    out = []
    for b, n, shape in zip(bufs, sizes, shapes):
        if b is None:
            out.append(None)
            continue
        sent = SENT_I if b.dtype == torch.int64 else SENT_F
        assert bool((b[:GUARD + shift] == sent).all()) and bool((b[GUARD + shift + n:] == sent).all()), "a guard was written"
        out.append(b[GUARD + shift:GUARD + shift + n].reshape(shape).cpu())
    return out


B_CASES = [(1, 1, 1, 4, 256), (2, 3, 5, 4, 256), (3, 32, 32, 4, 256), (3, 17, 19, 8, 16)]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["uint8", "int64"])
@pytest.mark.parametrize("case", B_CASES, ids=lambda c: "x".join(map(str, c)))
def test_vq_token_feat_equals_the_torch_chain(case, dtype):
    """(3, 17, 19): 323 positions, two workgroups per image with a partial one; D + n_e = 24 channels, two channel chunks with a partial one."""
    N, h, w, D, n_e = case
    cb = R.codebook_case(n_e, D, seed=5)
    tok = R.token_case(N, h, w, n_e, seed=9, dtype=dtype)
    want = R.torch_chain(tok, cb)
    cb_d, tok_d = cb.to(DEV), tok.to(DEV)
    got = run_b(tok_d, cb_d)
    for g, r, name in zip(got, want, ("idx", "zq", "feat")):
        assert g.dtype == r.dtype and torch.equal(g, r), name
    for g, r in zip(run_b(tok_d, cb_d), got):                                   # two runs, equal bits
        assert torch.equal(g, r)
    for k in range(3):                                                          # each output alone, the others null
        only = run_b(tok_d, cb_d, want=tuple(j == k for j in range(3)))
        assert torch.equal(only[k], want[k]) and all(only[j] is None for j in range(3) if j != k)
    if N == 3:                                                                  # image 1 of 3 equals the same image run alone
        for g, r in zip(run_b(tok_d[1:2].contiguous(), cb_d), got):
            assert torch.equal(g[0], r[1])
    from dc_vic_amd import ops
    for g, r in zip(ops.vq_token_feat(tok_d, cb_d, want_feat=True), want):
        assert torch.equal(g.cpu(), r)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["uint8", "int64"])
@pytest.mark.parametrize("case", [(2, 4, 6, 4, 256), (3, 32, 32, 4, 256), (2, 2, 2, 8, 16)], ids=lambda c: "x".join(map(str, c)))
def test_vq_token_feat_on_views_off_their_alignment(case, dtype):
    """Outputs one and three elements past a 16-byte address, and tokens one element into their allocation (an odd address for uint8,
    8 bytes off 16 for int64): the bits of the aligned call, with the guards around the shifted outputs intact."""
    N, h, w, D, n_e = case
    cb = R.codebook_case(n_e, D, seed=6)
    tok = R.token_case(N, h, w, n_e, seed=10, dtype=dtype)
    want = R.torch_chain(tok, cb)
    cb_d, tok_d = cb.to(DEV), tok.to(DEV)
    flat = torch.zeros(tok.numel() + 1, dtype=dtype, device=DEV)
    flat[1:] = tok_d.reshape(-1)
    off = flat[1:].reshape(tok.shape)
    assert tok_d.data_ptr() % 16 == 0 and off.data_ptr() % 16 == tok.element_size()
    for name, got in (("aligned", run_b(tok_d, cb_d)), ("outputs off", run_b(tok_d, cb_d, shift=1)), ("tokens off", run_b(off, cb_d)),
                      ("zq alone, off", run_b(tok_d, cb_d, want=(False, True, False), shift=3))):
        for g, r in zip(got, want):
            assert g is None or torch.equal(g, r), name
    bad = tok.long().clone()
    bad.view(-1)[1], bad.view(-1)[6] = n_e, -1                                   # the rule for tokens outside the codebook, here too
    idx, zq, feat = run_b(bad.to(DEV), cb_d)
    ridx, rzq, rfeat = R.vq_token_feat_ref(bad, cb)
    assert torch.equal(idx, ridx) and torch.equal(zq.isnan(), rzq.isnan()) and torch.equal(zq.nan_to_num(7.0), rzq.nan_to_num(7.0))
    assert torch.equal(feat.nan_to_num(7.0), rfeat.nan_to_num(7.0)) and int(zq.isnan().sum()) == 2 * D


def test_vq_token_feat_tokens_outside_the_codebook():
    """n_e and -1 among valid int64 tokens: NaN zq and an all-zero one-hot at those positions only, idx carried through."""
    N, h, w, D, n_e = 2, 3, 5, 4, 256
    cb = R.codebook_case(n_e, D, seed=5)
    tok = R.token_case(N, h, w, n_e, seed=9)
    bad = tok.clone()
    bad[0, 1, 2], bad[1, 2, 4], bad[1, 0, 0] = n_e, -1, 1 << 40
    idx, zq, feat = run_b(bad.to(DEV), cb.to(DEV))
    _, zq0, feat0 = R.torch_chain(tok, cb)
    hit = (bad != tok).unsqueeze(1)
    assert int(hit.sum()) == 3 and torch.equal(idx, bad)
    assert torch.isnan(zq[hit.expand_as(zq)]).all() and torch.equal(torch.where(hit, zq0, zq), zq0)
    assert torch.isnan(feat[:, :D][hit.expand(-1, D, -1, -1)]).all() and not feat[:, D:][hit.expand(-1, n_e, -1, -1)].any()
    assert torch.equal(torch.where(hit, feat0, feat), feat0)
    ridx, rzq, rfeat = R.vq_token_feat_ref(bad, cb)
    assert torch.equal(ridx, idx) and torch.equal(rzq.isnan(), zq.isnan()) and torch.equal(rfeat.nan_to_num(7.0), feat.nan_to_num(7.0))


def test_argument_refusals_on_the_gpu():
    assert R.check_refusals() == 26


# ---------------------------------------------------------------------------------------------------- vq_encode
@pytest.fixture(scope="module")
def model():
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    m = build_comp_model(BaseConfig.fromfile(os.path.join(R.ROOT, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
    load_synth_weights(m, 1234)
    return m


@pytest.mark.parametrize("want_feat", [False, True])
@pytest.mark.parametrize("how", ["uint8_device", "int64_device", "int64_host", "int32_host"])
def test_vq_encode_with_tokens_equals_the_torch_route(model, how, want_feat):
    n_e = model.vq_model.quantize.embedding.weight.shape[0]
    tok = R.token_case(2, 8, 16, n_e, seed=4)
    x = torch.zeros((2, 3, 64, 128), device=DEV)
    given = {"uint8_device": tok.to(torch.uint8).to(DEV), "int64_device": tok.to(DEV), "int64_host": tok, "int32_host": tok.int()}[how]
    with torch.no_grad():
        out = model.vq_encode(x, given, want_feat=want_feat)
        idx = tok.to(DEV)
        zq = model.vq_indices_to_latent(idx)
        want = (zq, idx, model._index_feat(zq, idx)) if want_feat else (zq, idx)
    assert len(out) == len(want)
    for g, r in zip(out, want):
        assert g.dtype == r.dtype and g.device == r.device and g.is_contiguous() and torch.equal(g, r)
