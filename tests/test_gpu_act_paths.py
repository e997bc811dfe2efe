"""Every kernel path that applies dcvic_act (csrc/common.h) gives the bits it gave before the activation switch was hoisted out of the
per-value code: the GroupNorm apply pass (float4, scalar and handed-over-statistics paths, out of place and in place), the epilogue of
every convolution family ConvPlan can route to (direct, async, async16, 1x1 DMA 64 / 96 / 128, 3x3 DMA, F(2x2) Winograd, thin cin / cout)
and the elementwise kernel's default arm -- each under every activation, with and without bias, residual and affine where the family
takes them.

A case is the SHA-256 of its output bytes against tests/golden/act_paths.json, which tools/record_act_golden.py wrote on the parent
build (tests/act_paths_cases.py holds the cases and says what the inputs contain).  On a mismatch the failure also reports the largest
absolute difference against a float64 torch evaluation of the same case, so that a moved bit can be told from a wrong result.  Every
convolution case asserts the kernel it reached through the launch statistics (ops.kernel_events_*), so a case cannot test a neighbour."""
import pytest
import torch

import act_paths_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return A.load_golden()["hashes"]


def check(golden, cid, y, ref64):
    got = A.sha(y)
    if got != golden[cid]:
        diff = float((y.detach().cpu().double() - ref64().double()).abs().nan_to_num(nan=float("inf")).max())
        raise AssertionError(f"{cid}: output bytes differ from the recorded ones (sha256 {got[:16]}.. != {golden[cid][:16]}..); "
                             f"max |y - float64 evaluation| = {diff:.3e}")


@pytest.mark.parametrize("name", list(A.GN_SHAPES))
@pytest.mark.parametrize("a", A.ACTS, ids=A.ACT_NAMES)
def test_groupnorm_apply(golden, name, a):
    dev = tuple(None if t is None else t.to(A.DEV) for t in A.gn_inputs(name))
    for inplace in (False, True):
        y = A.gn_run(name, a, inplace, dev)
        check(golden, f"gn/{name}/{A.ACT_NAMES[a]}/{'inplace' if inplace else 'out'}", y, lambda: A.gn_ref64(name, a))


@pytest.fixture(scope="module")
def runners():
    cache = {}

    def get(c):
        if c["id"] not in cache:
            cache.clear()                 # one family's maps on the device at a time
            cache[c["id"]] = A.ConvRunner(c)
        return cache[c["id"]]
    return get


@pytest.mark.parametrize("a", A.ACTS, ids=A.ACT_NAMES)
@pytest.mark.parametrize("c", A.CONV_CASES, ids=[c["id"] for c in A.CONV_CASES])
def test_conv_epilogue(golden, runners, c, a):
    rn = runners(c)
    want = A.conv_expected_kernel(c)
    for cb in A.conv_combos(c):
        y, names = rn.run(a, cb)
        assert names == [want], f"{A.conv_id(c, a, cb)}: ran {names}, the case is about {want}"
        check(golden, A.conv_id(c, a, cb), y, lambda: A.conv_ref64(c, a, cb))


@pytest.mark.parametrize("op", A.EW_DEFAULT_OPS)
@pytest.mark.parametrize("a", A.ACTS, ids=A.ACT_NAMES)
def test_ew_default_arm(golden, op, a):
    x = A.ew_inputs()
    y = A.ew_run(op, a, x.to(A.DEV))
    check(golden, f"ew/op{op}/{A.ACT_NAMES[a]}", y, lambda: A.act_fn(a, x.double()))
