"""Host-side checks of the activation-path cases (tests/act_paths_cases.py), no GPU: the recorded hashes cover exactly the cases the GPU
test replays, the convolution cases route to the kernel family they name under dcvic_conv2d_f32's host rules at 256 CUs
(conv_direct_ref.launch_plan), and the seeded inputs carry the values the cases are about."""
import torch

import act_paths_cases as A
import conv_direct_ref as R


def test_golden_covers_every_case():
    doc = A.load_golden()
    assert list(doc["hashes"]) == A.all_ids()
    assert all(len(h) == 64 and set(h) <= set("0123456789abcdef") for h in doc["hashes"].values())
    assert "compiler" in doc["header"] and "clang" in doc["header"]["compiler"]
    commit = doc["header"]["recorded_on_commit"]                    # the build the bits were taken from: the parent of the hoist
    assert len(commit) == 40 and set(commit) <= set("0123456789abcdef")
    # in place and out of place are the same computation
    for k, h in doc["hashes"].items():
        if k.endswith("/inplace"):
            assert h == doc["hashes"][k[:-len("inplace")] + "out"], k


def test_conv_cases_route_to_their_family():
    for c in A.CONV_CASES:
        assert c["N"] == 2
        if c["wino"]:
            assert c["expect"] == 9100 and c["W"] % 4 == 0 and all(ci % 8 == 0 for ci in c["cins"])
            assert c["cout"] % 64 and (c["H"] % 8 or c["W"] % 32)
            continue
        p = R.case_plan(c)
        assert p["variant"] == c["expect"], (c["id"], p)
        if not c["thin"]:
            assert c["cout"] % R.CLASS_TC[p["cls"]], c["id"]        # the last co-tile is partial
            assert p["blocks"] > 1


def test_inputs_carry_the_edge_values():
    def has_edges(t):
        f = t.reshape(-1)
        z = f[f == 0]
        sub = f[(f != 0) & (f.abs() < 2.0 ** -126)]
        return bool((torch.signbit(z)).any() and (~torch.signbit(z)).any() and (sub > 0).any() and (sub < 0).any())

    for name in A.GN_SHAPES:
        x, gamma, beta, part = A.gn_inputs(name)
        assert has_edges(x)
        assert bool((gamma == 0).any()) and bool(torch.signbit(beta[gamma == 0]).any())          # act(-0) is reached
        assert bool(((gamma != 0) & (gamma.abs() < 2.0 ** -126)).any())                           # subnormal products
        xh = (x - x.mean()) / x.std()
        assert float(xh.max()) * 40.0 - 3.0 > 88.73 and float(xh.min()) * 40.0 - 3.0 < -103.5 and float(gamma[1]) == 40.0   # |v| past 88
        assert (part is not None) == A.GN_SHAPES[name]["part"]
    for c in A.CONV_CASES:
        x, w, bias, res, aff = A.conv_inputs(c)
        assert has_edges(x) and has_edges(res)
        assert float(bias[0]) == float(torch.tensor(A.EDGE[0])) and not w[0].any()               # the activation sees fp32(88.6) exactly
        if c["cout"] >= 12:
            assert bias[:len(A.EDGE)].tolist() == torch.tensor(A.EDGE).tolist() and not w[:len(A.EDGE)].any()
    x = A.ew_inputs()
    assert has_edges(x) and float(x.abs().max()) > 88.73 and x.reshape(-1)[5:5 + len(A.EDGE)].tolist() == torch.tensor(A.EDGE).tolist()
