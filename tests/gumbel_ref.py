"""The reference expression of the hard Gumbel-softmax VQ sample for a GIVEN draw, in torch (any dtype, with autograd), and the seeded
inputs of the kernel tests.  F.gumbel_softmax(logits, tau, hard=True, dim=1) draws e = empty_like(logits).exponential_() and returns

    z = (logits - log(e)) / tau;  s = softmax(z, 1);  idx = s.max(1)[1];  ret = one_hot(idx) - s.detach() + s

(torch/nn/functional.py); hyperprior_dc_vic_model.py:254-260 multiplies `ret` with the detached codebook and applies post_quant_conv.
tests/test_gumbel_host.py holds `restate_ret` to F.gumbel_softmax bit for bit and its gradient to central differences."""
import numpy as np
import torch
import torch.nn.functional as F

FLT_MIN = float(np.finfo(np.float32).tiny)
TAUS = (0.5, 1.0, 2.0)
MIN_GAP = 1e-3          # of z = (logits - log e) / tau at the largest tau of TAUS, in fp64: an fp32 evaluation cannot move the argmax

# (N, C, H, W, D): the smallest shapes that reach each edge of csrc/gumbel.hip (64-position tiles, 16 waves over C, 272 classes in registers)
SHAPES = {
    "shipped_classes_half_tile": (2, 256, 4, 8, 4),
    "odd_classes_tile_plus_1": (3, 19, 5, 13, 4),
    "d8_129_positions": (2, 257, 3, 43, 8),
    "streaming_300_classes": (1, 300, 8, 8, 4),
    "one_class": (1, 1, 2, 2, 4),
}
REGIMES = ("normal", "saturated", "extreme_noise")


def restate_ret(logits, e, tau):
    """(idx, ret) of F.gumbel_softmax(logits, tau, hard=True, dim=1) for the draw e, op for op."""
    gumbels = -e.log()
    gumbels = (logits + gumbels) / tau
    y_soft = gumbels.softmax(1)
    index = y_soft.max(1, keepdim=True)[1]
    y_hard = torch.zeros_like(logits, memory_format=torch.legacy_contiguous_format).scatter_(1, index, 1.0)
    return index.squeeze(1), y_hard - y_soft.detach() + y_soft


def restate(logits, e, tau, codebook, pq_w, pq_b):
    """(idx, ret, lat): lat = post_quant_conv(ret @ codebook) as [N, D, H, W]; every tensor in logits' dtype."""
    idx, ret = restate_ret(logits, e, tau)
    zq = torch.einsum("nchw,cd->ndhw", ret, codebook)
    lat = F.conv2d(zq, pq_w.reshape(pq_w.shape[0], pq_w.shape[1], 1, 1), pq_b)
    return idx, ret, lat


def restate_grad(logits, e, tau, codebook, pq_w, pq_b, glatent, dtype):
    """(idx, lat, dlogits) of the restatement evaluated in `dtype`, dlogits by autograd for the gradient glatent on lat."""
    c = lambda t: None if t is None else t.detach().to(dtype)
    lg = c(logits).requires_grad_(True)
    idx, _, lat = restate(lg, c(e), tau, c(codebook), c(pq_w), c(pq_b))
    lat.backward(c(glatent))
    return idx, lat.detach(), lg.grad


def top2_gap(logits, e, tau):
    """Per position, the fp64 distance between the two largest z (inf with one class)."""
    z = (logits.double() - e.double().log()) / tau
    if z.shape[1] == 1:
        return torch.full_like(z[:, 0], float("inf"))
    top = z.topk(2, dim=1)[0]
    return top[:, 0] - top[:, 1]


def build_inputs(name, regime, seed=0):
    """Seeded fp32 inputs of one case: logits 3 * N(0, 1), e ~ Exp(1), codebook, post_quant weights and bias, and the gradient on the
    latent.  `saturated` raises one class per position by 30; `extreme_noise` plants FLT_MIN and 80 in the draw.  Where a position's
    top-2 gap of z falls below MIN_GAP at the largest tau, 1 is added to its winning logit; the gap is then asserted everywhere.
    -> dict, with `nudged` = the number of such positions."""
    N, C, H, W, D = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, name + regime)))
    logits = 3.0 * torch.randn((N, C, H, W), generator=g)
    e = torch.empty((N, C, H, W)).exponential_(generator=g)
    if regime == "saturated":
        cls = torch.randint(0, C, (N, 1, H, W), generator=g)
        logits.scatter_add_(1, cls, torch.full((N, 1, H, W), 30.0))
    elif regime == "extreme_noise":
        flat = e.view(-1)
        pick = torch.randperm(flat.numel(), generator=g)[:max(2, flat.numel() // 16)]
        flat[pick[0::2]] = FLT_MIN
        flat[pick[1::2]] = 80.0
    tau_max = max(TAUS)
    low = top2_gap(logits, e, tau_max) < MIN_GAP
    if bool(low.any()):
        win = ((logits.double() - e.double().log()).argmax(1, keepdim=True))
        logits.scatter_add_(1, win, low.unsqueeze(1).float())
    assert float(top2_gap(logits, e, tau_max).min()) >= MIN_GAP
    return dict(logits=logits, noise=e, codebook=torch.randn((C, D), generator=g), pq_w=torch.randn((D, D), generator=g) * 0.5,
                pq_b=torch.randn(D, generator=g) * 0.1, glatent=torch.randn((N, D, H, W), generator=g), nudged=int(low.sum()))
