"""tests/vq_ref.py, host side (no GPU): the exact fp32 fma against rationals, the distance chain against integers, the dispatcher's
restatement, the tie quota of the regimes, the structural boundaries the duplicated rows span, and the sensitivity of the case table to
three index rules gone wrong.  Also the fifth public header include/dcvic_vq.h against _lib.VQ_SIGNATURES."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import test_cabi
import vq_ref as R
from dc_vic_amd import _lib
from test_focal_host import loss_header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HOST_CASES = R.CASES


def test_fma32_is_exact():
    """fma32 against a rational evaluation rounded once: 12 000 seeded triples over a wide exponent range, a third of them with
    c near -a * b (cancellation) and a third with |c| far below |a * b|; then constructed triples whose exact sum lies just off an
    fp32 midpoint that the fp64 sum lands on, where the plain fp64 route is wrong -- asserted, so the construction is known to bite."""
    rng = np.random.default_rng(11)
    n = 12000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)
    k = n // 3
    c[:k] = (-(a[:k].astype(np.float64) * b[:k]) * (1 + rng.integers(-4, 5, k) * 2.0 ** -23)).astype(F32)
    c[k:2 * k] = (a[k:2 * k].astype(np.float64) * b[k:2 * k] * 2.0 ** -rng.integers(24, 60, k)).astype(F32)
    want = np.array([R.fma32_exact(x, y, w) for x, y, w in zip(a, b, c)], F32)
    got = R.fma32(a, b, c)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))

    # (1 + k 2^-12)(1 + m 2^-12) = 1 + (k + m) 2^-12 + k m 2^-24 with k m odd: an fp32 midpoint (ulp 2^-23); c = +-2^-60 is lost by the
    # fp64 sum (ulp 2^-52), which then ties to even, while the exact sum lies strictly on one side
    ks, ms = 2 * rng.integers(0, 512, 200) + 1, 2 * rng.integers(0, 512, 200) + 1        # odd, below 1024: the product stays below 2
    a2 = np.repeat((1 + ks * 2.0 ** -12).astype(F32), 2)
    b2 = np.repeat((1 + ms * 2.0 ** -12).astype(F32), 2)
    c2 = np.tile(np.array([2.0 ** -60, -2.0 ** -60], F32), 200)
    want2 = np.array([R.fma32_exact(x, y, w) for x, y, w in zip(a2, b2, c2)], F32)
    assert np.array_equal(R.fma32(a2, b2, c2), want2)
    plain_wrong = (R.fma32_plain(a2, b2, c2) != want2).reshape(200, 2)
    assert (plain_wrong.sum(axis=1) == 1).all(), "every constructed pair must defeat the plain fp64 route for exactly one sign of c"
    # the same below the normal range, where the midpoints are those of the denormal grid: 3 * 2^-150 + 2^-149 * 2^-30
    tiny = R.fma32(F32(3.0), F32(2.0 ** -149), F32(0.0))
    assert tiny == F32(3 * 2.0 ** -149)
    assert R.fma32(F32(2.0 ** -75), F32(1.5 * 2.0 ** -75), F32(2.0 ** -149)) == R.fma32_exact(F32(2.0 ** -75), F32(1.5 * 2.0 ** -75), F32(2.0 ** -149))
    assert R.f32_from_fraction(Fraction(3, 2 ** 150)) == F32(2.0 ** -148) and R.f32_from_fraction(Fraction(1, 2 ** 150)) == F32(0.0)
    assert R.f32_from_fraction(Fraction(2 ** 25 + 1, 2 ** 25)) == F32(1.0) and R.f32_from_fraction(Fraction(-(2 ** 24 + 3), 2 ** 24)) == F32(-(1 + 2.0 ** -22))


def test_dist32_is_exact_on_the_grid_and_its_two_forms_agree():
    """grid: z and codes in {-3..3} 2^-8, so the distance is the integer |z - e|^2 2^-16 and every fp32 step is exact.  On every
    regime the fma form (packed, shard) and the subtract form (generic) are the same bits, since 2 * dot is exact."""
    n_grid = 0
    for c in HOST_CASES:
        if c["N"] * c["HW"] * c["n_e"] > 3 * 10 ** 5:
            continue
        z, cb, _, _ = R.make_inputs(c)
        zf = z.transpose(0, 2, 1).reshape(-1, c["D"])
        d = R.dist32(zf, cb, "fma")
        assert np.array_equal(d.view(np.uint32), R.dist32(zf, cb, "sub").view(np.uint32)), c["id"]
        if c["regime"] == "grid":
            zi, ei = np.rint(zf.astype(np.float64) * 256).astype(np.int64), np.rint(cb.astype(np.float64) * 256).astype(np.int64)
            di = ((zi[:, None, :] - ei[None, :, :]) ** 2).sum(axis=2)
            assert np.array_equal(d.astype(np.float64) * 65536, di.astype(np.float64)), c["id"]
            assert np.array_equal(R.argmin_first(d), np.argmin(di, axis=1)), c["id"]
            n_grid += 1
    assert n_grid >= 10


def test_variant_of_reaches_every_variant_and_every_refusal():
    reached = {c["variant"] for c in R.CASES}
    assert reached == {"shard", "packed2", "packed1", "lds4", "lds8"}
    for what, N, D, HW, n_e in R.REFUSED:
        assert R.variant_of(N, D, HW, n_e) == "EINVAL", what
    for args in ((0, 4, 16, 256), (1, 4, 0, 256), (1, 4, 16, 0)):
        assert R.variant_of(*args) == "EINVAL"
    # the thresholds, each from both sides
    assert R.variant_of(65535, 4, 1, 256) == "packed2" and R.variant_of(2047, 4, 1, 256) == "packed1"
    assert R.variant_of(1024, 4, 1025, 8) == "packed2" and R.variant_of(1024, 4, 1024, 8) == "packed1"
    assert R.variant_of(1, 4, 16, 1024) == "packed1" and R.variant_of(1, 4, 16, 1032) == "lds4" and R.variant_of(1, 4, 16, 1280) == "shard"
    assert R.variant_of(1, 4, 16, 1280, cb_aligned16=False) == "lds4" and R.variant_of(1, 4, 16, 256, force="shard") == "shard"
    assert R.variant_of(1, 4, 16, 256, cb_aligned16=False, force="shard") == "packed1" and R.variant_of(1, 4, 16, 256, force="lds") == "lds4"
    assert R.variant_of(1, 4, 16, 8190) == "lds4" and R.variant_of(1, 4, 16, 8192) == "shard" and R.variant_of(1, 4, 16, 8193) == "EINVAL"
    assert R.variant_of(1, 4, 16, 8192, cb_aligned16=False) == "lds4" and R.variant_of(1, 4, 16, 8448, cb_aligned16=False) == "EINVAL"
    assert R.variant_of(1, 8, 16, 4551) == "lds8" and R.variant_of(1, 8, 16, 256, force="shard") == "lds8"
    # every variant meets every regime, with the duplicated rows in place
    for v in reached:
        assert {c["regime"] for c in R.CASES if c["variant"] == v} == set(R.REGIMES), v
    assert set(R.VARIANT_CODE.values()) == {_lib.VQ_SHARD, _lib.VQ_PACKED2, _lib.VQ_PACKED1, _lib.VQ_LDS4, _lib.VQ_LDS8}
    assert R.VARIANT_CODE["shard"] == _lib.VQ_SHARD and R.VARIANT_CODE["lds8"] == _lib.VQ_LDS8 and R.VARIANT_CODE["packed1"] == _lib.VQ_PACKED1


def test_regimes_tie_and_duplicates_span_every_boundary():
    """Every grid and cancel case has a tied restated minimum on at least a quarter of its vectors; every boundary dup_pairs names is
    spanned, per variant, by a vector whose minimum is attained at both rows of the pair and resolved to the first; and the structural
    models, unchanged, are argmin_first."""
    spanned = {}
    for c in HOST_CASES:
        ref = R.case_reference(c)
        if c["regime"] in ("grid", "cancel"):
            assert ref["tied"] >= 0.25, (c["id"], ref["tied"])
        zf = ref["z"].transpose(0, 2, 1).reshape(-1, c["D"])
        idx = ref["idx"].reshape(-1)
        first = {a: (b, what) for a, b, what in ref["pairs"]}
        for m, a in ref["hit"].items():
            b, what = first[a]
            d = R.dist32(zf[m:m + 1], ref["cb"], R.FORM[c["variant"]])[0]
            if d[a] == d[b] == d.min() and idx[m] == a:
                spanned.setdefault((R.RESOLVE[c["variant"]].__name__, what), c["id"])
        if c["N"] * c["HW"] * c["n_e"] <= 3 * 10 ** 5:
            d = R.dist32(zf, ref["cb"], R.FORM[c["variant"]])
            assert np.array_equal(R.RESOLVE[c["variant"]](d), idx), c["id"]
    for variant, n_e in (("packed1", 256), ("shard", 2048), ("lds4", 255)):
        for _, _, what in R.dup_pairs(variant, n_e):
            assert (R.RESOLVE[variant].__name__, what) in spanned, (variant, what)
    assert len(R.dup_pairs("shard", 2048)) == 6 and len(R.dup_pairs("packed1", 256)) == 3


# the first case of the table that fails under each change, pinned so that a change of the table shows
EXPECT_FIRST = {"last": "lds4-n255x4-N1-HW1-zeros", "offset0": "packed1-n8x4-N1-HW1-model", "dist": "shard-n256x4-N1-HW15-cancel-forced"}


@pytest.mark.parametrize("change", ["last", "offset0", "dist"])
def test_cases_are_sensitive_to_a_wrong_index_rule(change):
    """A copy of the restatement with one index rule changed (vq_ref.resolve_*): the last minimum for the first, a group resolved to its
    offset 0, the lane groups merged by distance alone.  At least one case of every variant the change applies to must differ."""
    failing = {}
    for c in HOST_CASES:
        if c["variant"] not in R.CHANGES[change]:
            continue
        ref = R.case_reference(c)
        zf = ref["z"].transpose(0, 2, 1).reshape(-1, c["D"])
        rows = max(1, R.CHUNK // c["n_e"])
        for m0 in range(0, zf.shape[0], rows):
            d = R.dist32(zf[m0:m0 + rows], ref["cb"], R.FORM[c["variant"]])
            if not np.array_equal(R.RESOLVE[c["variant"]](d, change), ref["idx"].reshape(-1)[m0:m0 + rows]):
                failing.setdefault(c["variant"], c["id"])
                break
    print(f"change {change!r}: first failing case per variant {failing}")
    for v in R.CHANGES[change]:
        assert v in failing, (change, v)
    first = next(c["id"] for c in R.CASES if c["id"] in failing.values())
    assert first == EXPECT_FIRST[change], (change, first)



def test_argmax_lut_ref_first_maximum_and_chain():
    for case in R.LUT_CASES[:12]:
        cb, w, bias = R.lut_weights(case)
        for kind in R.LUT_KINDS:
            x = R.lut_logits(case, kind)
            idx, lat = R.argmax_lut_ref(x, cb, w, bias)
            mx = x.max(axis=1, keepdims=True)
            firsts = np.argmax(x == mx, axis=1)
            assert np.array_equal(idx, firsts), (case["id"], kind)
            if kind == "all_neg_inf" or kind == "all_equal":
                assert (idx == 0).all()
            if case["n_e"] >= 256 and kind in ("plateaus", "signed_zeros"):
                assert ((x == mx).sum(axis=1) > 1).mean() > 0.5, (case["id"], kind)
            # one pixel by rationals
            n, p = case["N"] - 1, case["HW"] // 2
            for ch in range(case["D"]):
                a = F32(0.0)
                for d in range(case["D"]):
                    a = R.fma32_exact(w[ch, d], cb[idx[n, p], d], a)
                assert lat[n, ch, p] == F32(a + bias[ch]), (case["id"], kind)
    assert {c["D"] for c in R.LUT_CASES} == {3, 4, 8}
    assert R.argmax_lut_ref(np.zeros((1, 2, 3), F32))[1] is None


def test_vq_header_matches_its_signature_table():
    protos = loss_header_prototypes(os.path.join(ROOT, "include", "dcvic_vq.h"))
    assert protos == {"dcvic_vq_last_variant": (C.c_int, [])}
    assert test_cabi.signature_mismatches(_lib.VQ_SIGNATURES, protos) == []
    others = set()
    for h in ("dcvic.h", "dcvic_loss.h", "dcvic_rate.h", "dcvic_train.h"):
        others |= set(loss_header_prototypes(os.path.join(ROOT, "include", h)))
    assert not set(protos) & others
    assert not set(_lib.VQ_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.RATE_SIGNATURES) | set(_lib.TRAIN_SIGNATURES))
    L = _lib.lib()
    fn = L.dcvic_vq_last_variant
    assert fn.restype is C.c_int and list(fn.argtypes) == []
    assert test_cabi.signature_mismatches(dict(_lib.VQ_SIGNATURES, dcvic_vq_last_variant="q:"), protos) != []
    # the header's codes are the binding's
    txt = open(os.path.join(ROOT, "include", "dcvic_vq.h")).read()
    import re
    codes = {k: int(v) for k, v in re.findall(r"#define DCVIC_VQ_(\w+)\s+(\d+)", txt)}
    assert codes == {"NONE": _lib.VQ_NONE, "SHARD": _lib.VQ_SHARD, "PACKED2": _lib.VQ_PACKED2, "PACKED1": _lib.VQ_PACKED1,
                     "LDS4": _lib.VQ_LDS4, "LDS8": _lib.VQ_LDS8}


def test_search_refusals_without_gpu():
    """dcvic_vq_argmin_f32 and dcvic_argmax_lut_f32 refuse what their contracts exclude before any launch (every GPU hidden)."""
    lines = [f"err(L.dcvic_vq_argmin_f32(P, P, P, P, P, {N}, {D}, {HW}, {n_e}, None), 'vq_argmin')" for _, N, D, HW, n_e in R.REFUSED]
    lines += ["assert L.dcvic_vq_last_variant() == 0",
              "err(L.dcvic_argmax_lut_f32(P, None, None, P, P, P, 1, 256, 4, 16, None), 'argmax_lut')",
              "err(L.dcvic_argmax_lut_f32(P, P, P, None, P, P, 1, 256, 4, 16, None), 'argmax_lut', 'codebook')",
              "print('CHECKS_OK')"]
    test_cabi._run_without_gpu("\n".join(lines) + "\n")
