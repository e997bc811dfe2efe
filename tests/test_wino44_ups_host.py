"""Host-side checks of the upsample-structured F(4x4, 3x3) convolution (csrc/wino44_ups.hip): its transform constants, its packed
size and its argument checks.  No GPU needed."""
import ctypes as C
from fractions import Fraction as Fr

import numpy as np

from dc_vic_amd import _lib

# the constants as the kernel writes them: S in the header comment / U4_S_THIRD, A^T in u4_at, G in u4_u; rows of S and G in the
# order of the kept interpolation points 0, 1, 3/2, -3/2, inf (the point -1 is the dropped one)
S = [[Fr(9, 4), Fr(-13, 4), 1, 0],
     [0, Fr(-9, 2), 2, 0],
     [0, Fr(-5, 2), Fr(5, 2), 0],
     [0, Fr(1, 2), Fr(-1, 2), 0],
     [0, Fr(9, 4), Fr(-13, 4), 1]]
AT = [[1, 1, 1, 1, 0],
      [0, 1, Fr(3, 2), Fr(-3, 2), 0],
      [0, 1, Fr(9, 4), Fr(9, 4), 0],
      [0, 1, Fr(27, 8), Fr(-27, 8), 1]]
G = [[Fr(4, 9), 0, 0], [Fr(-2, 5), Fr(-2, 5), Fr(-2, 5)], [Fr(8, 45), Fr(4, 15), Fr(2, 5)], [Fr(8, 45), Fr(-4, 15), Fr(2, 5)], [0, 0, 1]]


def _mm(A, B):
    return [[sum(Fr(A[i][k]) * Fr(B[k][j]) for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _t(A):
    return [list(r) for r in zip(*A)]


def test_wino44_ups_transform_is_an_exact_upsample_convolution():
    """Y = A^T [(G g G^T) . (S d S^T)] A on a 4x4 low-resolution patch d equals, in rational arithmetic, the 3x3 correlation of the
    nearest-x2 upsampled rows / columns [a, b, b, c, c, d] for the 4x4 output tile whose origin is a multiple of 4; every constant of
    S and A^T is a dyadic rational (exact in fp32)."""
    for row in S + AT:
        for v in row:
            d = Fr(v).denominator
            assert d & (d - 1) == 0, v
    rng = np.random.RandomState(0)
    for _ in range(3):
        d = [[Fr(int(v)) for v in r] for r in rng.randint(-9, 10, (4, 4))]
        g = [[Fr(int(v)) for v in r] for r in rng.randint(-9, 10, (3, 3))]
        U = _mm(_mm(G, g), _t(G))
        V = _mm(_mm(S, d), _t(S))
        M = [[U[a][b] * V[a][b] for b in range(5)] for a in range(5)]
        Y = _mm(_mm(AT, M), _t(AT))
        rep = [0, 1, 1, 2, 2, 3]                      # upsampled row / column u of the 6x6 window -> low-resolution index
        up = [[d[rep[i]][rep[j]] for j in range(6)] for i in range(6)]
        ref = [[sum(up[i + r][j + c] * g[r][c] for r in range(3) for c in range(3)) for j in range(4)] for i in range(4)]
        assert Y == ref


def test_wino44_ups_transform_is_the_textbook_f44_on_the_structure():
    """S is B^T P of the textbook F(4x4, 3x3) at the points 0, 1, -1, 3/2, -3/2, inf (P the 6x4 row replication [a, b, b, c, c, d]) with
    the row of the point -1 removed because it is zero there, and A^T / G are the textbook matrices restricted to the kept points."""
    pts = [Fr(0), Fr(1), Fr(-1), Fr(3, 2), Fr(-3, 2)]

    def poly(roots):
        c = [Fr(1)]
        for r in roots:
            c = [(c[k - 1] if k > 0 else 0) - r * (c[k] if k < len(c) else 0) for k in range(len(c) + 1)]
        return c
    BT = [poly([q for q in pts if q != p]) + [Fr(0)] for p in pts] + [poly(pts)]
    P = [[1 if rep == c else 0 for c in range(4)] for rep in (0, 1, 1, 2, 2, 3)]
    BP = _mm(BT, P)
    assert BP[2] == [0, 0, 0, 0]
    assert [BP[j] for j in (0, 1, 3, 4, 5)] == [[Fr(v) for v in r] for r in S]
    AT6 = [[p ** i for p in pts] + [Fr(int(i == 3))] for i in range(4)]
    assert [[AT6[i][j] for j in (0, 1, 3, 4, 5)] for i in range(4)] == [[Fr(v) for v in r] for r in AT]


def test_wino44_ups_kernel_forms_equal_the_matrices():
    """The three-thirds form of S x the kernel executes (U4_S_THIRD) and the form of A^T m in u4_at equal the matrices."""
    rng = np.random.RandomState(1)
    x = [Fr(int(v)) for v in rng.randint(-9, 10, 4)]
    t0, t1, q = x[2] - Fr(13, 4) * x[1], x[3] - Fr(13, 4) * x[2], x[2] - x[1]
    y0, y4, e = Fr(9, 4) * x[0] + t0, Fr(9, 4) * x[1] + t1, x[2] + x[2]
    y = [y0, e - Fr(9, 2) * x[1], Fr(5, 2) * q, Fr(-1, 2) * q, y4]
    assert y == [sum(Fr(S[i][k]) * x[k] for k in range(4)) for i in range(5)]
    m = [Fr(int(v)) for v in rng.randint(-9, 10, 5)]
    s, dd = m[2] + m[3], m[2] - m[3]
    ya = [(m[0] + m[1]) + s, m[1] + Fr(3, 2) * dd, m[1] + Fr(9, 4) * s, Fr(27, 8) * dd + (m[1] + m[4])]
    assert ya == [sum(Fr(AT[i][k]) * m[k] for k in range(5)) for i in range(4)]


def test_wino44_ups_fp32_error_level():
    """fp32 error of one 256 -> 256 layer through these transforms (torch emulation, fp64 reference) stays at the 1e-6 level of the
    plain F(4x4) kernel's points."""
    import torch
    f = lambda Mx: torch.tensor([[float(v) for v in r] for r in Mx], dtype=torch.float64)
    St, ATt, Gt = f(S), f(AT), f(G)
    torch.manual_seed(0)
    Cin = Cout = 256
    H = 8                                            # low resolution: output 16 x 16
    x = torch.randn(Cin, H, H)
    w = torch.randn(Cout, Cin, 3, 3) / (3 * Cin ** 0.5)
    ref = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x[None].double(), scale_factor=2), w.double(), padding=1)[0]
    U = torch.einsum("ar,kcrs,bs->abkc", Gt, w.double(), Gt).float()
    Pt = torch.nn.functional.pad(x, (1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2)          # [c, 4, 4 tiles, 4, 4]
    V = torch.einsum("ar,cijrs,bs->abcij", St.float(), Pt, St.float())
    M = torch.einsum("abkc,abcij->abkij", U, V)
    Y = torch.einsum("ia,abkxy,jb->kxiyj", ATt.float(), M, ATt.float()).reshape(Cout, 4 * Pt.shape[1], 4 * Pt.shape[2])
    err = float((Y.double() - ref).abs().max()) / float(ref.abs().max())
    assert err < 1e-5, err


def test_wino44_ups_packed_bytes_and_argument_checks():
    """dcvic_wino44_ups_packed_bytes: one 50 KiB slab (2 k-steps x 25 positions x 4 channels x 64 output channels, fp32) per (64-channel
    tile, 8-channel chunk).  The entry points check their arguments before any HIP call (the shared convolution io check plus their
    own: 8-channel sources, W % 4, activation, statistics buffer)."""
    L = _lib.lib()
    for cin, cout in ((256, 256), (512, 512), (8, 64), (128, 200)):
        assert L.dcvic_wino44_ups_packed_bytes(cin, cout) == ((cout + 63) // 64) * ((cin + 7) // 8) * 2 * 25 * 4 * 64 * 4
    assert L.dcvic_wino44_ups_packed_bytes(0, 64) == 0
    assert L.dcvic_wino44_ups_pack_f32(None, None, 8, 8, None) == -1
    N, CIN, H, W = 2, 16, 8, 8

    def make_io(srcs=(CIN,), w=W, act=0):
        io = _lib.ConvIO()
        io.N, io.H, io.W = N, H, w
        io.Hout, io.Wout, io.Hfull, io.Wfull = 2 * H, 2 * w, 2 * H, 2 * w
        io.osy = io.osx = 1
        io.n_src = len(srcs)
        for i, c in enumerate(srcs):
            io.src[i].ptr = 64; io.src[i].C = c; io.src[i].batch_stride = c * H * w
        io.out = 64; io.out_batch_stride = 16 * 4 * H * w
        io.act = act
        return io
    P = C.c_void_p(64)

    def rejects(rc, prefixes=("conv3x3_wino44_ups", "conv3x3_wino44_ups_stats")):
        assert rc == -1
        assert L.dcvic_last_error().decode().split(":")[0] in prefixes, L.dcvic_last_error()
    plain = lambda io, cin=CIN: L.dcvic_conv3x3_wino44_ups_f32(cin, 16, P, None if io is None else C.byref(io), None)
    stats = lambda io, cin=CIN, part=P: L.dcvic_conv3x3_wino44_ups_stats_f32(cin, 16, P, None if io is None else C.byref(io), part, None)
    for call in (plain, stats):
        rejects(call(None))
        rejects(call(make_io(srcs=(12,)), cin=12))                  # 8-channel sources
        rejects(call(make_io(w=6)))                                  # W % 4
        rejects(call(make_io(act=3)))                                # transcendental epilogue
        io = make_io()
        io.Hout = H                                                  # not the x2 output
        rejects(call(io))
    rejects(stats(make_io(), part=None))
