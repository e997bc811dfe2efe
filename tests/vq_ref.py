"""The VQ search and argmax -> codebook LUT kernels (csrc/vq.hip) restated on the CPU, bit for bit, with the case tables and the input
regimes that tests/test_vq_host.py and tests/test_gpu_vq.py share.

Every operation of these kernels is one IEEE fp32 operation in an order the source fixes (__fmul_rn, __fadd_rn, fmaf; the fp32 MFMA is a
k-ordered fma chain), so the restatement is EQUAL to the kernel, not close to it.  numpy's fp32 multiply, add and subtract are those
operations; the fused multiply-add is fma32 below, exact with one rounding.

A plain module: numpy only, nothing that needs a GPU at import."""
from fractions import Fraction

import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ exact fp32 arithmetic
def f32_from_fraction(q):
    """The fp32 nearest to the rational q, ties to even, denormals included (|q| below the fp32 maximum)."""
    q = Fraction(q)
    if q == 0:
        return F32(0.0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()        # 2^(e-1) <= q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1
    ulp = max(e - 23, -149)
    scaled = q / Fraction(2) ** ulp
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    assert n <= 1 << 24 and ulp + 24 <= 128, "fp32 overflow is out of scope"
    return F32(sign * float(n) * 2.0 ** ulp)                         # n <= 2^24 and a power of two: exact in fp64, then exact in fp32


def fma32_exact(a, b, c):
    """fma(a, b, c) of three fp32 scalars through rationals: the yardstick for fma32."""
    return f32_from_fraction(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma32_plain(a, b, c):
    """The fp64-then-fp32 route: a * b is exact in fp64, the sum is rounded to fp64 and then to fp32.  Wrong where the fp64 sum is
    inexact and lands on an fp32 rounding midpoint (tests/test_vq_host.py constructs such triples)."""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64) + np.asarray(c, F32).astype(np.float64)).astype(F32)


def fma32(a, b, c):
    """fp32 fma with a single rounding, element by element on broadcastable arrays.  The product of two fp32 is exact in fp64.  The
    fp64 sum p + c then rounds to fp32 as the exact sum does unless it is inexact AND lies exactly on an fp32 rounding midpoint (or below
    the fp32 normal range, where the midpoints sit elsewhere); those few elements are redone with rationals."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    r = s.astype(F32)
    bits = s.view(np.uint64)
    cand = (bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)             # the 29 bits fp32 drops are 1000...0
    cand |= (np.abs(s) < 2.0 ** -126) & (s != 0)
    if cand.any():
        i = np.flatnonzero(cand)
        pi, ci, si = p.ravel()[i], c64.ravel()[i], s.ravel()[i]
        bb = si - pi                                                            # TwoSum: the error of the fp64 sum, exactly
        err = (pi - (si - bb)) + (ci - bb)
        i = i[err != 0]
        if i.size:
            r = r.copy()
            af, bf, cf, rf = a.ravel(), b.ravel(), c.ravel(), r.reshape(-1)
            for k in i:
                rf[k] = fma32_exact(af[k], bf[k], cf[k])
    return r


# ------------------------------------------------------------------------------------------------ the search, restated
def sq32(x):
    """[K, D] -> [K]: rounded squares summed left to right (z2 and e2 of every kernel)."""
    x = np.asarray(x, F32)
    s = x[:, 0] * x[:, 0]
    for d in range(1, x.shape[1]):
        s = s + x[:, d] * x[:, d]
    return s


def dot32(z, cb):
    """[M, D], [n_e, D] -> [M, n_e]: fma(z_{D-1}, e_{D-1}, ... fma(z1, e1, z0 * e0))."""
    z, cb = np.asarray(z, F32), np.asarray(cb, F32)
    dot = z[:, :1] * cb[None, :, 0]
    for d in range(1, z.shape[1]):
        dot = fma32(z[:, d:d + 1], cb[None, :, d], dot)
    return dot


def dist32(z, cb, form="fma"):
    """The kernels' distance of every vector z [M, D] to every code cb [n_e, D], fp32 [M, n_e].
      form "fma": d = fma(-2, dot, z2 + e2)      the packed and the shard kernel
      form "sub": d = (z2 + e2) - 2 * dot        the generic kernel
    The two are equal: 2 * dot is exact, so both round the same exact value once (tests/test_vq_host.py asserts it)."""
    t = sq32(z)[:, None] + sq32(cb)[None, :]
    dot = dot32(z, cb)
    if form == "fma":
        return fma32(F32(-2.0), dot, t)
    assert form == "sub", form
    return t - F32(2.0) * dot


def argmin_first(d):
    return np.argmin(d, axis=1).astype(np.int64)


def tied(d):
    """[M] bool: the minimum of the row is attained more than once."""
    return (d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1


FORM = {"shard": "fma", "packed2": "fma", "packed1": "fma", "lds4": "sub", "lds8": "sub"}
CHUNK = 1 << 21                        # distances per chunk of vectors: bounds the fp64 temporaries of fma32


def search_ref(z, cb, variant, want_feat=True, resolve=None):
    """z [N, D, HW], cb [n_e, D] -> dict(idx [N, HW] int64, zq [N, D, HW], feat [N, D + n_e, HW] = cat[zq, one_hot], tied = the share
    of vectors whose restated minimum is attained twice or more).  resolve: the index rule, argmin_first unless a test passes one of
    the structural models below."""
    z, cb = np.asarray(z, F32), np.asarray(cb, F32)
    N, D, HW = z.shape
    n_e = cb.shape[0]
    zf = np.ascontiguousarray(z.transpose(0, 2, 1)).reshape(N * HW, D)
    idx = np.empty(N * HW, np.int64)
    n_tied = 0
    rows = max(1, CHUNK // n_e)
    for m0 in range(0, N * HW, rows):
        d = dist32(zf[m0:m0 + rows], cb, FORM[variant])
        idx[m0:m0 + rows] = (resolve or argmin_first)(d)
        n_tied += int(tied(d).sum())
    e = cb[idx]
    zq = zf + (e - zf)
    out = {"idx": idx.reshape(N, HW), "zq": np.ascontiguousarray(zq.reshape(N, HW, D).transpose(0, 2, 1)), "tied": n_tied / (N * HW)}
    if want_feat:
        feat = np.zeros((N, D + n_e, HW), F32)
        feat[:, :D] = out["zq"]
        nn, pp = np.divmod(np.arange(N * HW), HW)
        feat[nn, D + idx, pp] = 1.0
        out["feat"] = feat
    return out


# Structural models of how each kernel reaches its index from the distances, with the three changes the host test shows the cases to be
# sensitive to.  Unchanged, each equals argmin_first.
#   change "last":    the last minimum instead of the first (a `<=` for the `<`, the larger index in a merge)
#   change "offset0": a group resolved to its offset 0 (the packed kernel's found = -1 fallback taken always)
#   change "dist":    the shard kernel's lane groups merged by distance alone
def resolve_generic(d, change=None):
    if change == "last":
        return (d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)).astype(np.int64)
    return argmin_first(d)


def resolve_packed(d, change=None):
    """vq_argmin4_kernel: the minimum of every 8-code group, the first group whose minimum is strictly below the running one, then the
    first code of that group whose distance equals the minimum."""
    M, n_e = d.shape
    assert n_e % 8 == 0
    g = d.reshape(M, n_e // 8, 8)
    gm = g.min(axis=2)
    last = change == "last"
    grp = (gm.shape[1] - 1 - np.argmin(gm[:, ::-1], axis=1)) if last else np.argmin(gm, axis=1)
    if change == "offset0":
        return (grp * 8).astype(np.int64)
    win = g[np.arange(M), grp]
    eq = win == win.min(axis=1, keepdims=True)
    found = (7 - np.argmax(eq[:, ::-1], axis=1)) if last else np.argmax(eq, axis=1)
    return (grp * 8 + found).astype(np.int64)


def resolve_shard(d, change=None):
    """vq_shard_mfma_kernel: lane group g owns the codes j with (j % 16) // 4 == g in ascending order under a strict `<`; the four
    (d, idx) pairs are merged by xor 16 (g0 with g1, g2 with g3), then xor 32 (g0 with g2): the smaller distance, at equal distances
    the smaller index.  Lane group 0 stores."""
    M, n_e = d.shape
    assert n_e % 256 == 0
    codes = np.arange(n_e)
    best, bi = [], []
    for g in range(4):
        own = codes[(codes % 16) // 4 == g]
        sub = d[:, own]
        k = (sub.shape[1] - 1 - np.argmin(sub[:, ::-1], axis=1)) if change == "last" else np.argmin(sub, axis=1)
        best.append(sub[np.arange(M), k])
        bi.append(own[k])

    def merge(b0, i0, b1, i1):            # what the lane holding (b0, i0) keeps after it has seen (b1, i1)
        if change == "dist":
            take = b1 < b0
        elif change == "last":
            take = (b1 < b0) | ((b1 == b0) & (i1 > i0))
        else:
            take = (b1 < b0) | ((b1 == b0) & (i1 < i0))
        return np.where(take, b1, b0), np.where(take, i1, i0)
    b01, i01 = merge(best[0], bi[0], best[1], bi[1])
    b23, i23 = merge(best[2], bi[2], best[3], bi[3])
    return merge(b01, i01, b23, i23)[1].astype(np.int64)


RESOLVE = {"shard": resolve_shard, "packed2": resolve_packed, "packed1": resolve_packed, "lds4": resolve_generic, "lds8": resolve_generic}
CHANGES = {"last": ("shard", "packed2", "packed1", "lds4", "lds8"), "offset0": ("packed2", "packed1"), "dist": ("shard",)}


# ------------------------------------------------------------------------------------------------ argmax -> LUT, restated
def argmax_lut_ref(logits, cb=None, w=None, bias=None):
    """logits [N, n_e, HW] -> (idx [N, HW] = the first maximum, latent [N, D, HW] or None without a codebook):
    a = 0; a = fma(w[c][d], cb[idx][d], a) for d ascending; then + bias[c]."""
    idx = np.argmax(np.asarray(logits, F32), axis=1).astype(np.int64)
    if cb is None:
        return idx, None
    cb, w = np.asarray(cb, F32), np.asarray(w, F32)
    D = cb.shape[1]
    e = cb[idx]                                                   # [N, HW, D]
    lat = np.empty((idx.shape[0], D, idx.shape[1]), F32)
    for c in range(D):
        a = np.zeros(idx.shape, F32)
        for d in range(D):
            a = fma32(w[c, d], e[:, :, d], a)
        lat[:, c] = a + F32(bias[c]) if bias is not None else a
    return idx, lat


# ------------------------------------------------------------------------------------------------ the dispatcher, restated
LDS_LIMIT = 160 * 1024


def cdiv(a, b):
    return (a + b - 1) // b


def variant_of(N, D, HW, n_e, cb_aligned16=True, force=None):
    """dcvic_vq_argmin_f32's dispatcher: 'shard', 'packed2', 'packed1', 'lds4', 'lds8' or 'EINVAL'.  force: DCVIC_VQ_KERNEL."""
    force = force or ""
    if not (N > 0 and HW > 0 and n_e > 0) or D not in (4, 8) or N > 65535:
        return "EINVAL"
    shard_ok = D == 4 and n_e % 256 == 0 and cb_aligned16
    if shard_ok and (n_e > 1024 or force.startswith("sh")):
        return "shard"
    if n_e * (D + 1) * 4 > LDS_LIMIT:
        return "EINVAL"
    if D == 4 and n_e % 8 == 0 and n_e <= 1024 and not force.startswith("l"):
        return "packed2" if N * cdiv(HW, 1024) >= 2048 else "packed1"
    return "lds4" if D == 4 else "lds8"


VARIANT_CODE = {"shard": 1, "packed2": 2, "packed1": 3, "lds4": 4, "lds8": 5}     # include/dcvic_vq.h

# (what, N, D, HW, n_e): refused by the argument checks, nothing written
REFUSED = [
    ("D = 5", 1, 5, 16, 256),
    ("N = 65536", 65536, 4, 1, 256),
    ("D = 4, n_e = 8200: no LDS image, no shards", 1, 4, 16, 8200),
    ("D = 8, n_e = 4552: no LDS image", 1, 8, 16, 4552),
]


# ------------------------------------------------------------------------------------------------ input regimes
REGIMES = ("model", "grid", "cancel", "hits", "zeros")


def _signs(pattern, D):
    return np.array([1.0 if (pattern >> (d % 4)) & 1 else -1.0 for d in range(D)], F32)


def dup_pairs(variant, n_e):
    """(first, copy, boundary) rows: cb[copy] = cb[first], so that a vector equal to cb[first] has a tied minimum that spans the named
    structural boundary; the first must win."""
    if variant in ("packed1", "packed2"):
        want = [(1, 5, "within one 8-code group"), (3, 10, "across two 8-code groups"), (n_e - 16 + 6, n_e - 8 + 0, "across the last two groups")]
    elif variant == "shard":
        want = [(1, 9, "across lane groups 0 and 2 of one tile"), (6, 12, "across lane groups 1 and 3 of one tile"),
                (21, 32 + 2, "across two tiles, the copy in a lower lane group"), (17, 49, "across two tiles, one lane group"),
                (7 + 64, 256 + 2, "across two shards, the copy in a lower lane group"), (256 + 45, n_e - 256 + 44, "across two shards, one lane group")]
    else:
        want = [(2, n_e - 1, "first against last code"), (n_e // 2, n_e // 2 + 1, "neighbours")]
    used, out = set(), []
    for a, b, what in want:
        if 0 <= a < b < n_e and not {a, b} & used:
            used |= {a, b}
            out.append((a, b, what))
    return out


def make_inputs(case):
    """-> z [N, D, HW], cb [n_e, D] (fp32 numpy, seeded by the case), pairs = dup_pairs placed in cb, and hit = {vector m: row} for the
    vectors set equal to a duplicated row (none in `cancel`, whose vectors are far from every code)."""
    N, D, HW, n_e, regime, variant = (case[k] for k in ("N", "D", "HW", "n_e", "regime", "variant"))
    rng = np.random.default_rng(case["seed"])
    M = N * HW
    if regime == "grid":
        # every product, square and sum is a multiple of 2^-16 below 2^8: all arithmetic is exact, true ties abound
        cb = rng.integers(-3, 4, (n_e, D)).astype(F32) * F32(2.0 ** -8)
        z = rng.integers(-3, 4, (M, D)).astype(F32) * F32(2.0 ** -8)
        # few codes, or 8 dimensions (where equidistant codes are rarer): a block of rows repeats the first rows in another order
        h = n_e // 2 if n_e < 64 else n_e // 3 if D == 8 else 0
        if h:
            cb[n_e - h:] = cb[rng.permutation(h)]
    elif regime == "cancel":
        # |z_d| about 1e3, |e_d| about 1e-2: z2 + e2 rounds to z2 (ulp 0.25 .. 0.5), and the codes that share the sign pattern of z
        # have dots within 1e-3 of each other, so their distances collide
        P = min(16, max(1, n_e // 2))
        cb = np.stack([_signs(j % P, D) for j in range(n_e)]) * (F32(0.01) * (1 + 1e-5 * rng.uniform(-1, 1, (n_e, D)))).astype(F32)
        z = np.stack([_signs(p, D) for p in rng.integers(0, P, M)]) * (1000.0 * (1 + 0.05 * rng.uniform(-1, 1, (M, D)))).astype(F32)
    else:
        cb = (rng.uniform(-1, 1, (n_e, D)) / n_e).astype(F32)
        z = (rng.standard_normal((M, D)) * (0.6 / n_e)).astype(F32)
    cb, z = cb.astype(F32), z.astype(F32)
    if regime == "zeros":
        for r, v in ((n_e // 3, 0.0), (n_e - 1, -0.0), (0, 0.0)):   # all-zero rows, one of them -0.0; they tie for z = 0
            if n_e > 3 or r == 0:
                cb[r] = v
        z[::2] = 0.0
        z[1::4] = -0.0
        z[3::8, 1] = -0.0
    pairs = dup_pairs(variant, n_e) if regime != "zeros" else []
    for a, b, _ in pairs:
        cb[b] = cb[a]
    if regime == "hits":                                            # z = cb[j] for every j (as many as there are vectors), spread over the image
        j = (np.arange(M) * (n_e // M if M < n_e else 1)) % n_e
        z = cb[j].copy()
    hit = {}
    if regime != "cancel":
        for k, (a, b, _) in enumerate(pairs):                       # the duplicated rows are hit at both ends of the image (the ragged tail)
            for m in (k, M - 1 - k):
                if 0 <= m < M and m not in hit:
                    z[m] = cb[a]
                    hit[m] = a
    z = np.ascontiguousarray(z.reshape(N, HW, D).transpose(0, 2, 1))
    return z, cb, pairs, hit


# ------------------------------------------------------------------------------------------------ case tables
def _cases():
    table = {
        # variant: (HW set, N set, [(n_e, D, force, aligned)])
        # n_e = 1000 is a multiple of 8 and would go to the packed kernel: like 256 it reaches the LDS kernel forced
        "lds4": ((1, 255, 256, 257), (1, 3), [(1, 4, None, True), (255, 4, None, True), (1000, 4, "lds", True), (256, 4, "lds", True),
                                                (2048, 4, None, False), (8190, 4, None, True)]),
        "lds8": ((1, 255, 256, 257), (1, 3), [(8, 8, None, True), (256, 8, None, True), (1001, 8, None, True)]),
        "packed1": ((1, 257, 511, 512, 513), (1, 3), [(8, 4, None, True), (256, 4, None, True), (1024, 4, None, True), (256, 4, None, False)]),
        "shard": ((1, 15, 17, 63, 65, 255, 257), (1, 3), [(256, 4, "shard", True), (512, 4, "shard", True), (2048, 4, None, True),
                                                            (16384, 4, None, True)]),
    }
    out = []
    for variant, (hws, ns, params) in table.items():
        k = 0
        for p, (n_e, D, force, aligned) in enumerate(params):
            for HW in hws:
                for N in ns:
                    out.append(dict(variant=variant, N=N, D=D, HW=HW, n_e=n_e, force=force, aligned=aligned, k=k + p))
                    k += 1
    for k, ((N, HW), n_e) in enumerate(((s, n) for s in ((2048, 1), (2048, 769), (1024, 1025)) for n in (8, 16))):
        out.append(dict(variant="packed2", N=N, D=4, HW=HW, n_e=n_e, force=None, aligned=True, k=k))
    for i, c in enumerate(out):
        # the regimes rotate through a variant's cases, shifted by one per parameter row, so that every shape and every parameter
        # meets several regimes; a single code can tie with nothing, so n_e = 1 keeps to the regimes without a tie quota
        regimes = ("model", "hits", "zeros") if c["n_e"] == 1 else REGIMES
        c["regime"] = regimes[c["k"] % len(regimes)]
        if c["variant"] == "packed2":
            c["regime"] = ("cancel", "hits", "model", "grid", "zeros", "grid")[i - (len(out) - 6)]
        c["seed"] = 1000 + i
        c["id"] = "{variant}-n{n_e}x{D}-N{N}-HW{HW}-{regime}".format(**c) + ("-forced" if c["force"] else "") + ("" if c["aligned"] else "-misaligned")
        # vectors x codes stay at or below 2e7, except the one shape the packed2 threshold needs (2048 x 769 vectors x 16 codes = 2.5e7)
        assert c["N"] * c["HW"] * c["n_e"] <= (2 * 10 ** 7 if (c["N"], c["HW"], c["n_e"]) != (2048, 769, 16) else 2.6 * 10 ** 7), c["id"]
        assert variant_of(c["N"], c["D"], c["HW"], c["n_e"], c["aligned"], c["force"]) == c["variant"], c["id"]
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]

_REF_CACHE = {}


def case_reference(case):
    """Inputs and restated outputs of one case, computed once and shared (read-only) by the tests that need them."""
    if case["id"] not in _REF_CACHE:
        z, cb, pairs, hit = make_inputs(case)
        ref = search_ref(z, cb, case["variant"])
        ref.update(z=z, cb=cb, pairs=pairs, hit=hit)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF_CACHE[case["id"]] = ref
    return _REF_CACHE[case["id"]]


# argmax_lut: (N, HW, n_e, D), D and the bias rotating; every case runs every input kind and every output combination
LUT_KINDS = ("plateaus", "all_equal", "all_neg_inf", "one_pos_inf", "signed_zeros")


def _lut_cases():
    out = []
    shapes = [(N, HW, n_e) for n_e in (1, 2, 256, 1001) for HW in (1, 255, 256, 257, 1000) for N in (1, 3)] + [(1, 257, 16384), (3, 257, 16384)]
    for i, (N, HW, n_e) in enumerate(shapes):
        D = (3, 4, 8)[i % 3]
        out.append(dict(N=N, HW=HW, n_e=n_e, D=D, seed=5000 + i, id=f"n{n_e}-N{N}-HW{HW}-D{D}"))
    return out


LUT_CASES = _lut_cases()


def lut_logits(case, kind):
    """[N, n_e, HW] fp32 logits of one named kind."""
    N, HW, n_e = case["N"], case["HW"], case["n_e"]
    rng = np.random.default_rng(case["seed"] + LUT_KINDS.index(kind))
    x = rng.standard_normal((N, n_e, HW)).astype(F32)
    if kind == "plateaus":                 # quantised to a few levels: the maximum is attained by many channels
        x = np.round(x * F32(1.5)).astype(F32)
    elif kind == "all_equal":
        x[:] = F32(0.75)
    elif kind == "all_neg_inf":
        x[:] = -np.inf
    elif kind == "one_pos_inf":            # one +inf per pixel, and the plateau of finite maxima around it
        x = np.round(x).astype(F32)
        j = rng.integers(0, n_e, (N, HW))
        nn, pp = np.divmod(np.arange(N * HW), HW)
        x[nn, j.reshape(-1), pp] = np.inf
    elif kind == "signed_zeros":           # nothing above zero; +0.0 and -0.0 are equal, the first of either sign wins
        x = -np.abs(np.round(x)).astype(F32)
        x[x == 0] = np.where(rng.integers(0, 2, int((x == 0).sum())) == 1, F32(-0.0), F32(0.0))
    else:
        raise ValueError(kind)
    return x


def lut_weights(case):
    """cb [n_e, D], w [D, D], bias [D]."""
    rng = np.random.default_rng(case["seed"] + 77)
    n_e, D = case["n_e"], case["D"]
    return ((rng.uniform(-1, 1, (n_e, D)) / max(n_e, 16)).astype(F32), (rng.standard_normal((D, D)) * 0.5).astype(F32),
            (rng.standard_normal(D) * 0.1).astype(F32))
