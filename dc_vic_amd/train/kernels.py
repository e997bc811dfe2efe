"""ctypes wrappers of the training-step kernels (csrc/train.hip, include/dcvic.h "Training step"; csrc/chan_ce.hip; csrc/sample_loss.hip,
include/dcvic_sample_loss.h; csrc/rate_train.hip, include/dcvic_rate.h; csrc/gumbel.hip, include/dcvic_gumbel.h; csrc/msssim_loss.hip, include/dcvic_msssim_loss.h; csrc/data.hip, include/dcvic_data.h; csrc/bn_train.hip, include/dcvic_bn.h).  torch only supplies device memory; every computation is a HIP kernel launch on the current stream."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from .. import ops
from .._lib import check, lib
from ..ops import _bs, _chk4, _p, _stream

Tensor = torch.Tensor
_WS = {}
_WS_MIN = {torch.float32: 1 << 16, torch.float64: 1024}    # smallest allocation, in elements


def _workspace(n: int, device, tag: str = "f", dtype=torch.float32) -> Tensor:
    """Grow-only scratch buffers of at least n elements (one per tag and device), reused across launches on the same stream."""
    key = (tag, str(device))
    t = _WS.get(key)
    if t is None or t.numel() < n:
        t = _WS[key] = torch.empty(max(n, _WS_MIN[dtype]), dtype=dtype, device=device)
    return t


def conv_wgrad(G: Tensor, X: Tensor, dW: Tensor, KH: int, KW: int, stride: int, pad: int, accumulate: bool = True) -> None:
    """dW[m][c][ky][kx] (+)= sum G[n][m][oy][ox] * X[n][c][oy*s+ky-p][ox*s+kx-p]; dW contiguous [M, Cx, KH, KW]."""
    N, M, Hg, Wg = _chk4(G, "wgrad G")
    Nx, Cx, Hx, Wx = _chk4(X, "wgrad X")
    if N != Nx or not dW.is_contiguous() or dW.numel() != M * Cx * KH * KW:
        raise ValueError(f"conv_wgrad: shapes G{tuple(G.shape)} X{tuple(X.shape)} dW{tuple(dW.shape)}")
    need = int(lib().dcvic_conv_wgrad_workspace_floats(N, M, Cx, KH, KW, Hg, None))
    ws = _workspace(need, G.device, "wgrad")
    check(lib().dcvic_conv_wgrad_f32(_p(G), _bs(G), M, Hg, Wg, _p(X), _bs(X), Cx, Hx, Wx, N, KH, KW, stride, pad, pad, _p(dW),
                                     1 if accumulate else 0, _p(ws), _stream()), "conv_wgrad")


def conv_wgrad_src(G: Tensor, X: Tensor, dW: Tensor, c_off: int, KH: int, KW: int, stride: int, pad: int, accumulate: bool = True) -> None:
    """The weight gradient of ONE source X [N, Cs, Hx, Wx] (a channel-slice view with its own batch stride) of a multi-source
    convolution: dW[:, c_off:c_off + Cs] (+)= ..., dW contiguous [M, Cx_total, KH, KW].  One call per source gives the bits of
    conv_wgrad on the concatenated input (dcvic_conv_wgrad_src_f32)."""
    N, M, Hg, Wg = _chk4(G, "wgrad_src G")
    Nx, Cs, Hx, Wx = _chk4(X, "wgrad_src X")
    if N != Nx or dW.dim() != 4 or not dW.is_contiguous() or dW.dtype != torch.float32 or tuple(dW.shape[2:]) != (KH, KW) or dW.shape[0] != M:
        raise ValueError(f"conv_wgrad_src: shapes G{tuple(G.shape)} X{tuple(X.shape)} dW{tuple(dW.shape)}")
    Ct = int(dW.shape[1])
    need = int(lib().dcvic_conv_wgrad_workspace_floats(N, M, Ct, KH, KW, Hg, None))
    ws = _workspace(need, G.device, "wgrad")
    check(lib().dcvic_conv_wgrad_src_f32(_p(G), _bs(G), M, Hg, Wg, _p(X), _bs(X), Cs, Hx, Wx, N, KH, KW, stride, pad, pad, _p(dW), Ct, int(c_off),
                                         1 if accumulate else 0, _p(ws), _stream()), "conv_wgrad_src")


def chan_reduce(a: Tensor, b: Optional[Tensor] = None) -> Tensor:
    """[N, C, H, W] -> [N, C]: sum_p a (* b)."""
    N, Cc, H, W = _chk4(a, "chan_reduce a")
    if b is not None:
        _chk4(b, "chan_reduce b")
    out = torch.empty((N, Cc), dtype=torch.float32, device=a.device)
    check(lib().dcvic_chan_reduce_f32(_p(a), _bs(a), _p(b), _bs(b), _p(out), N, Cc, H * W, _stream()), "chan_reduce")
    return out


def sum_rows(x: Tensor, out: Tensor, accumulate: bool) -> None:
    """out[j] (+)= sum_i x[i][j]  (x: [rows, len] contiguous)."""
    rows = x.shape[0]
    ln = x.numel() // rows
    assert x.is_contiguous() and out.is_contiguous() and out.numel() == ln
    check(lib().dcvic_sum_rows_f32(_p(x), _p(out), rows, ln, 1 if accumulate else 0, _stream()), "sum_rows")


# The `op` of ew (dcvic_ew_bwd_f32); the table above ew_bwd_kernel in csrc/train.hip is the authority.
EW_ACT_GRAD = 0         # d = g * act'(a)              a: the OUTPUT for relu / lrelu02 / sigmoid / half_tanh, the INPUT for swish / gelu
EW_MUL = 1              # d = g * a
EW_MUL_SIGMOID = 2      # d = g * sigmoid(a)
EW_MUL_DSIGMOID = 3     # d = g * a * s (1 - s), s = sigmoid(b)
EW_SFT_DEC = 4          # d = g * (1 + w * a)
EW_SFT_SCALE = 5        # d = w * g * a
EW_SFT_SHIFT = 6        # d = w * g
EW_CHAN_SCALE = 7       # d = g * (1 + a[n][c])        a: a per-channel vector [N or 1][C], vec_bs = C or 0
EW_MSE_GRAD = 8         # d = 2 * w * (a - b)
EW_BCE_GRAD = 9         # d = w * (sigmoid(a) - act)   act: the target, 0 or 1
EW_ADD = 10             # d = a + b
EW_SCALE = 11           # d = a * w

# The `kind` of reduce_loss (dcvic_reduce_loss_f32, csrc/train.hip): out = scale * sum_i f.
SUM_SQ_ERR = 0          # f = (a - b)^2
SUM_BCE = 1             # f = BCE-with-logits(a, target)
SUM_SQ = 2              # f = a^2
SUM = 3                 # f = a


def ew(op: int, g: Optional[Tensor], a: Optional[Tensor] = None, b: Optional[Tensor] = None, w: float = 1.0, act: int = 0,
       out: Optional[Tensor] = None, vec_bs: int = 0) -> Tensor:
    ref = g if g is not None else a
    if out is None:
        out = torch.empty(ref.shape, dtype=torch.float32, device=ref.device)
    for t in (g, a if op != EW_CHAN_SCALE else None, b, out):
        if t is not None and not t.is_contiguous():
            raise ValueError("ew_bwd operands must be contiguous")
    Cc = ref.shape[1] if ref.dim() == 4 else 1
    HW = ref.shape[2] * ref.shape[3] if ref.dim() == 4 else 1
    check(lib().dcvic_ew_bwd_f32(op, _p(out), _p(g), _p(a), _p(b), ref.numel(), w, act, Cc, HW, vec_bs, _stream()), "ew_bwd")
    return out


def groupnorm_bwd(x: Tensor, dy: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float, act: int):
    N, Cc, H, W = _chk4(x, "gn_bwd x")
    _chk4(dy, "gn_bwd dy")
    dx = torch.empty((N, Cc, H, W), dtype=torch.float32, device=x.device)
    dg = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    db = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    check(lib().dcvic_groupnorm_bwd_f32(_p(x), _bs(x), _p(dy), _bs(dy), _p(dx), _bs(dx), _p(gamma), _p(beta), _p(dg), _p(db),
                                        N, Cc, H * W, groups, eps, act, _stream()), "groupnorm_bwd")
    return dx, dg, db


def layernorm_c_bwd(x: Tensor, dy: Tensor, gamma: Tensor, eps: float):
    N, Cc, H, W = _chk4(x, "ln_bwd x")
    if not (x.is_contiguous() and dy.is_contiguous()):
        raise ValueError("layernorm_c_bwd needs contiguous maps")
    dx = torch.empty_like(x)
    blocks = int(lib().dcvic_layernorm_c_bwd_blocks(N, H * W))
    part = torch.empty((blocks, 2 * Cc), dtype=torch.float32, device=x.device)
    check(lib().dcvic_layernorm_c_bwd_f32(_p(x), _p(dy), _p(dx), _p(gamma), _p(part), N, Cc, H * W, eps, _stream()), "layernorm_c_bwd")
    return dx, part


def softmax_c_bwd(P: Tensor, dP: Tensor, scale: float) -> Tensor:
    N, Cc, Pn = P.shape
    dS = torch.empty_like(P)
    check(lib().dcvic_softmax_c_bwd_f32(_p(P), _p(dP), _p(dS), N, Cc, Pn, scale, _stream()), "softmax_c_bwd")
    return dS


def swin_attn_bwd(qkv: Tensor, dout: Tensor, table: Tensor, dtable: Tensor, heads: int, ws: int, shift: int, accumulate: bool = True) -> Tensor:
    N, C3, H, W = _chk4(qkv, "swin_bwd qkv")
    Cc = C3 // 3
    dqkv = torch.empty_like(qkv)
    nwin = N * (H // ws) * (W // ws)
    wsb = _workspace(nwin * heads * ws ** 4, qkv.device, "swin")
    check(lib().dcvic_swin_attn_bwd_f32(_p(qkv), _p(dout.contiguous()), _p(dqkv), _p(table), _p(dtable), _p(wsb), N, Cc, H, W, heads, ws, shift,
                                        1 if accumulate else 0, _stream()), "swin_attn_bwd")
    return dqkv


def reduce_loss(kind: int, a: Tensor, b: Optional[Tensor], scale: float, target: int = 0) -> Tensor:
    """0-dim device tensor: scale * sum f(a, b)."""
    if not a.is_contiguous() or (b is not None and not b.is_contiguous()):
        raise ValueError("reduce_loss operands must be contiguous")
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    ws = _workspace(1024, a.device, "loss_ws", torch.float64)
    check(lib().dcvic_reduce_loss_f32(kind, _p(a), _p(b), a.numel(), target, scale, _p(out), _p(ws), _stream()), "reduce_loss")
    return out


def cross_entropy(logits: Tensor, target: Tensor, w: float, want_grad: bool = True):
    N, Cc, H, W = _chk4(logits, "ce logits")
    if not logits.is_contiguous() or target.dtype != torch.int64 or not target.is_contiguous():
        raise ValueError("cross_entropy: contiguous fp32 logits and int64 targets")
    nll = torch.empty((N, H, W), dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    check(lib().dcvic_cross_entropy_f32(_p(logits), _p(target), _p(nll), _p(dl), N, Cc, H * W, w, _stream()), "cross_entropy")
    return nll, dl


def _chan_ce_buffers(name: str, ws_doubles, logits: Tensor, target: Optional[Tensor], want_grad: bool):
    """What oasis_ce and focal_ce share: the operand checks, then (N, C, HW, workspace sized by the entry point's query `ws_doubles`,
    loss, dlogits or None)."""
    if logits.dim() != 4 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError(f"{name}: contiguous fp32 logits [N, C, H, W]")
    N, Cc, H, W = logits.shape
    if target is not None and (target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != N * H * W):
        raise ValueError(f"{name}: contiguous int64 targets with {N * H * W} elements")
    ws = _workspace(int(ws_doubles(N, H * W)), logits.device, name, torch.float64)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    return N, Cc, H * W, ws, loss, torch.empty_like(logits) if want_grad else None


def oasis_ce(logits: Tensor, target: Optional[Tensor], is_real: bool, scale: float, want_grad: bool = True, want_score: bool = False):
    """OASIS GAN loss (csrc/chan_ce.hip) in one pass over logits [N, C, H, W]: (loss, dlogits or None, score or None) with
    loss = scale * sum_positions CE(logits, index + 1 if is_real else 0), dlogits its gradient and score = mean(logits[:, 1:])."""
    N, Cc, HW, ws, loss, dl = _chan_ce_buffers("oasis_ce", lib().dcvic_oasis_ce_workspace_doubles, logits, target, want_grad)
    score = torch.empty(1, dtype=torch.float32, device=logits.device) if want_score else None
    check(lib().dcvic_oasis_ce_f32(_p(logits), _p(target), 1 if is_real else 0, scale, _p(loss), _p(dl), _p(score), _p(ws), N, Cc, HW,
                                   _stream()), "oasis_ce")
    return loss, dl, score


def focal_ce(logits: Tensor, target: Tensor, gamma: float, scale: float, want_grad: bool = True):
    """Focal cross entropy (csrc/chan_ce.hip) in one pass over logits [N, C, H, W]: (loss, dlogits or None) with
    loss = scale * sum_positions (1 - p_t)^gamma * CE(logits, target) and dlogits its gradient; gamma is 0 or >= 1."""
    N, Cc, HW, ws, loss, dl = _chan_ce_buffers("focal_ce", lib().dcvic_focal_ce_workspace_doubles, logits, target, want_grad)
    check(lib().dcvic_focal_ce_f32(_p(logits), _p(target), float(gamma), scale, _p(loss), _p(dl), _p(ws), N, Cc, HW, _stream()), "focal_ce")
    return loss, dl


# ------------------------------------------------------------------------------------------- per-image weights (csrc/sample_loss.hip)
def focal_ce_sample(logits: Tensor, target: Tensor, w: Tensor, gamma: float, want_grad: bool = True, want_per_sample: bool = False):
    """Focal cross entropy with one weight per image in one pass over logits [N, C, H, W]: (loss, dlogits or None, per_sample or None)
    with S[n] = sum_positions (1 - p_t)^gamma * CE of image n, loss = sum_n w[n] * S[n], dlogits its gradient and per_sample = S."""
    N, Cc, HW, ws, loss, dl = _chan_ce_buffers("focal_ce_sample", lib().dcvic_focal_ce_sample_workspace_doubles, logits, target, want_grad)
    per = torch.empty(N, dtype=torch.float32, device=logits.device) if want_per_sample else None
    check(lib().dcvic_focal_ce_sample_f32(_p(logits), _p(target), _p(_flat_f32(w, N, "focal_ce_sample: sample weights")), float(gamma), _p(loss),
                                          _p(dl), _p(per), _p(ws), N, Cc, HW, _stream()), "focal_ce_sample")
    return loss, dl, per


def sq_err_sample(a: Tensor, b: Tensor, w: Tensor, want_grad: bool = True, want_per_sample: bool = False):
    """Squared error with one weight per image, value and gradient in one pass: (loss, da or None, per_sample or None) with
    S[n] = sum (a[n] - b[n])^2, loss = sum_n w[n] * S[n] and da = 2 w[n] (a - b).  `a` [N, ...] is dense within an image and may have
    its own batch stride (a channel-slice view); `b` is contiguous."""
    N = a.shape[0]
    M = a.numel() // max(N, 1)
    if a.dtype != torch.float32 or not a.is_cuda or a.dim() < 2 or (N > 0 and not a[0].is_contiguous()):
        raise ValueError(f"sq_err_sample: a must be an fp32 device tensor [N, ...] that is dense within an image, got {a.dtype} {tuple(a.shape)}")
    if b.dtype != torch.float32 or b.shape != a.shape or not b.is_contiguous() or b.device != a.device:
        raise ValueError(f"sq_err_sample: b must be a contiguous fp32 tensor {tuple(a.shape)}, got {b.dtype} {tuple(b.shape)}")
    ws = _workspace(int(lib().dcvic_sq_err_sample_workspace_doubles(N, M)), a.device, "sq_err_sample", torch.float64)
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    da = torch.empty(a.shape, dtype=torch.float32, device=a.device) if want_grad else None
    per = torch.empty(N, dtype=torch.float32, device=a.device) if want_per_sample else None
    check(lib().dcvic_sq_err_sample_f32(_p(a), a.stride(0) if N > 1 else M, _p(b), _p(_flat_f32(w, N, "sq_err_sample: sample weights")), _p(loss),
                                        _p(da), _p(per), _p(ws), N, M, _stream()), "sq_err_sample")
    return loss, da, per


# ------------------------------------------------------------------------------------------- batch statistics (csrc/bn_train.hip)
def _bn_views(name: str, x: Tensor, *others: Optional[Tensor]):
    """(N, C, HW, workspace, its bytes) of [N, C, H, W] views of one shape, each with its own batch stride."""
    shape = _chk4(x, f"{name} x")
    for t in others:
        if t is not None and _chk4(t, name) != shape:
            raise ValueError(f"{name}: a tensor of {tuple(t.shape)} against x {tuple(x.shape)}")
    N, Cc, H, W = shape
    need = int(lib().dcvic_bn_workspace_bytes(N, Cc, H * W))
    ws = _workspace((need + 7) // 8, x.device, "bn", torch.float64)
    return N, Cc, H * W, ws, ws.numel() * 8


def bn_stats(x: Tensor):
    """(mean [C], unbiased standard deviation [C]) of x [N, C, H, W] over (N, H, W)  (dcvic_bn_stats_f32)."""
    N, Cc, HW, ws, wsb = _bn_views("bn_stats", x)
    mean, std = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
    check(lib().dcvic_bn_stats_f32(_p(x), _bs(x), _p(mean), _p(std), _p(ws), wsb, N, Cc, HW, _stream()), "bn_stats")
    return mean, std


def bn_train_fwd(x: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor], momentum: float,
                 eps: float, act: int = ops.ACT_NONE, out: Optional[Tensor] = None):
    """BatchNorm2d in training mode with an optional fused LeakyReLU(0.2) (dcvic_bn_train_fwd_f32): (y, save_mean [C], save_rstd [C]);
    the running statistics, when given, are updated in place."""
    y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    N, Cc, HW, ws, wsb = _bn_views("bn_train_fwd", x, y)
    for t, what in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _flat_f32(t, Cc, f"bn_train_fwd: {what}")
    mean, rstd = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
    check(lib().dcvic_bn_train_fwd_f32(_p(x), _bs(x), _p(y), _bs(y), _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(momentum),
                                       float(eps), _p(mean), _p(rstd), int(act), _p(ws), wsb, N, Cc, HW, _stream()), "bn_train_fwd")
    return y, mean, rstd


def bn_train_bwd(x: Tensor, g: Tensor, y: Optional[Tensor], save_mean: Tensor, save_rstd: Tensor, gamma: Tensor, dgamma: Optional[Tensor] = None,
                 dbeta: Optional[Tensor] = None, accumulate: bool = True, act: int = ops.ACT_NONE, dx: Optional[Tensor] = None) -> Tensor:
    """dx of bn_train_fwd for the gradient g on its output y (read only with an act); dgamma / dbeta [C], when given, are added to
    (accumulate) or overwritten  (dcvic_bn_train_bwd_f32)."""
    dx = dx if dx is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    N, Cc, HW, ws, wsb = _bn_views("bn_train_bwd", x, g, y, dx)
    for t, what in ((save_mean, "save_mean"), (save_rstd, "save_rstd"), (gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _flat_f32(t, Cc, f"bn_train_bwd: {what}")
    check(lib().dcvic_bn_train_bwd_f32(_p(x), _bs(x), _p(g), _bs(g), _p(y), _bs(y), _p(save_mean), _p(save_rstd), _p(gamma), _p(dx), _bs(dx),
                                       _p(dgamma), _p(dbeta), 1 if accumulate else 0, int(act), _p(ws), wsb, N, Cc, HW, _stream()), "bn_train_bwd")
    return dx


def actnorm_fwd(x: Tensor, loc: Tensor, scale: Tensor, act: int = ops.ACT_NONE, out: Optional[Tensor] = None) -> Tensor:
    """act(scale[c] * (x + loc[c]))  (dcvic_actnorm_fwd_f32); loc / scale hold C values ([1, C, 1, 1] is welcome)."""
    y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    N, Cc, H, W = _chk4(x, "actnorm_fwd x")
    if _chk4(y, "actnorm_fwd y") != (N, Cc, H, W):
        raise ValueError(f"actnorm_fwd: y {tuple(y.shape)} against x {tuple(x.shape)}")
    _flat_f32(loc, Cc, "actnorm_fwd: loc"), _flat_f32(scale, Cc, "actnorm_fwd: scale")
    check(lib().dcvic_actnorm_fwd_f32(_p(x), _bs(x), _p(y), _bs(y), _p(loc), _p(scale), int(act), N, Cc, H * W, _stream()), "actnorm_fwd")
    return y


def actnorm_bwd(x: Tensor, g: Tensor, y: Optional[Tensor], loc: Tensor, scale: Tensor, dloc: Optional[Tensor] = None, dscale: Optional[Tensor] = None,
                accumulate: bool = True, act: int = ops.ACT_NONE, dx: Optional[Tensor] = None) -> Tensor:
    """dx = scale * g' of actnorm_fwd; dloc = scale * sum g' and dscale = sum g' (x + loc), when given, are added to (accumulate) or
    overwritten  (dcvic_actnorm_bwd_f32)."""
    dx = dx if dx is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    N, Cc, HW, ws, wsb = _bn_views("actnorm_bwd", x, g, y, dx)
    for t, what in ((loc, "loc"), (scale, "scale"), (dloc, "dloc"), (dscale, "dscale")):
        _flat_f32(t, Cc, f"actnorm_bwd: {what}")
    check(lib().dcvic_actnorm_bwd_f32(_p(x), _bs(x), _p(g), _bs(g), _p(y), _bs(y), _p(loc), _p(scale), _p(dx), _bs(dx), _p(dloc), _p(dscale),
                                      1 if accumulate else 0, int(act), _p(ws), wsb, N, Cc, HW, _stream()), "actnorm_bwd")
    return dx


# ------------------------------------------------------------------------------------------- image distortions (csrc/msssim_loss.hip)
def _image_pair(name: str, a: Tensor, b: Tensor) -> None:
    for t, what in ((a, "first"), (b, "second")):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name}: the {what} operand must be a contiguous fp32 device tensor, got {t.dtype} {tuple(t.shape)} {t.device}")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"{name}: operands of {tuple(a.shape)} and {tuple(b.shape)}")


def ms_ssim_loss(real: Tensor, fake: Tensor, scale: float, want_grad: bool = True, want_per_plane: bool = False):
    """scale * sum over the N*C planes of (1 - MS-SSIM(real, fake)) with data_range = 1 on the planes as they are (dcvic_msssim_loss_f32):
    (loss: fp64 [1], dfake or None, per_plane: fp64 [N, C] MS-SSIM values or None); `real` is a constant.  [N, C, H, W], min(H, W) > 160."""
    _image_pair("ms_ssim_loss", real, fake)
    N, Cc, H, W = _chk4(fake, "ms_ssim_loss fake")
    need = int(lib().dcvic_msssim_loss_workspace_bytes(N, Cc, H, W))
    ws = _workspace((need + 7) // 8, fake.device, "msssim_loss", torch.float64)
    loss = torch.empty(1, dtype=torch.float64, device=fake.device)
    df = torch.empty_like(fake) if want_grad else None
    per = torch.empty((N, Cc), dtype=torch.float64, device=fake.device) if want_per_plane else None
    check(lib().dcvic_msssim_loss_f32(_p(real), _p(fake), N, Cc, H, W, float(scale), _p(loss), _p(per), _p(df), _p(ws), ws.numel() * 8, _stream()),
          "ms_ssim_loss")
    return loss, df, per


def abs_err(a: Tensor, b: Tensor, scale: float, want_grad: bool = True):
    """scale * sum |a - b| (dcvic_abs_err_f32): (loss: fp64 [1], da = scale * sign(a - b) or None); a, b [N, ...]."""
    _image_pair("abs_err", a, b)
    N = a.shape[0] if a.dim() > 0 else 0
    M = a.numel() // max(N, 1)
    need = int(lib().dcvic_abs_err_workspace_bytes(N, M))
    ws = _workspace((need + 7) // 8, a.device, "abs_err", torch.float64)
    loss = torch.empty(1, dtype=torch.float64, device=a.device)
    da = torch.empty_like(a) if want_grad else None
    check(lib().dcvic_abs_err_f32(_p(a), _p(b), M, N, float(scale), _p(loss), _p(da), _p(ws), ws.numel() * 8, _stream()), "abs_err")
    return loss, da


# ------------------------------------------------------------------------------------------- the rate term (csrc/rate_train.hip)
def gumbel_lut_bwd(logits: Tensor, noise: Tensor, glatent: Tensor, codebook: Tensor, pq_w: Tensor, tau: float) -> Tensor:
    """dlogits of ops.gumbel_lut's latent for a gradient `glatent` [N, D, H, W] on it: s_j * (v_j - sum_k s_k v_k) / tau with
    s = softmax((logits - log(noise)) / tau) recomputed and v_j = codebook[j] . (pq_w^T glatent)  (dcvic_gumbel_lut_bwd_f32)."""
    N, n_e, H, W = _chk4(logits, "gumbel_bwd logits")
    D = int(codebook.shape[1])
    if not (logits.is_contiguous() and noise.is_contiguous() and glatent.is_contiguous() and codebook.is_contiguous() and pq_w.is_contiguous()) \
            or tuple(noise.shape) != tuple(logits.shape) or tuple(glatent.shape) != (N, D, H, W) or int(codebook.shape[0]) != n_e:
        raise ValueError(f"gumbel_lut_bwd: logits {tuple(logits.shape)} noise {tuple(noise.shape)} glatent {tuple(glatent.shape)} codebook {tuple(codebook.shape)}")
    dl = torch.empty_like(logits)
    check(lib().dcvic_gumbel_lut_bwd_f32(_p(logits), _p(noise), _p(glatent), _p(codebook), _p(pq_w), float(tau), _p(dl), N, n_e, D, H * W, _stream()),
          "gumbel_lut_bwd")
    return dl


EB_PARAM_NAMES = tuple(f"_matrix{i}" for i in range(5)) + tuple(f"_bias{i}" for i in range(5)) + tuple(f"_factor{i}" for i in range(4))
_EB_WIDTH = (3, 9, 9, 9, 3, 3, 3, 3, 3, 1, 3, 3, 3, 3)


def _flat_f32(t: Optional[Tensor], n: int, what: str) -> Optional[Tensor]:
    """`t` (or None) checked to be a contiguous fp32 device tensor of n values."""
    if t is not None and (t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != n):
        raise ValueError(f"{what} must be a contiguous fp32 device tensor of {n} value(s), got {t.dtype} {tuple(t.shape)} {t.device}")
    return t


def _eb_struct(tensors: Optional[Sequence[Tensor]], C: int, what: str):
    """dcvic_eb_params / dcvic_eb_grads: 14 device pointers in the order of EB_PARAM_NAMES (a host struct, passed by address)."""
    if tensors is None:
        return None
    if len(tensors) != 14:
        raise ValueError(f"{what}: 14 tensors (matrix0..4, bias0..4, factor0..3), got {len(tensors)}")
    for t, k, name in zip(tensors, _EB_WIDTH, EB_PARAM_NAMES):
        _flat_f32(t, C * k, f"{what}: {name}")
    return (ctypes.c_void_p * 14)(*[t.data_ptr() for t in tensors])


def gaussian_rate_train(y: Tensor, mu: Tensor, sigma: Tensor, noise: Tensor, weights: Optional[Tensor], scale: float, y_hat: Optional[Tensor] = None,
                        lik: Optional[Tensor] = None, bits: Optional[Tensor] = None, loss: Optional[Tensor] = None, dy: Optional[Tensor] = None,
                        dmu: Optional[Tensor] = None, dsigma: Optional[Tensor] = None) -> None:
    """dcvic_gaussian_rate_train_f32 on [N, C, H, W] views (each with its own batch stride; mu / sigma and dmu / dsigma share one):
    bits [N] and loss [1] ACCUMULATE, every other given output is overwritten."""
    N, Cc, H, W = _chk4(y, "gaussian_rate_train y")
    for t, name in ((mu, "mu"), (sigma, "sigma"), (noise, "noise"), (y_hat, "y_hat"), (lik, "lik"), (dy, "dy"), (dmu, "dmu"), (dsigma, "dsigma")):
        if t is not None and _chk4(t, f"gaussian_rate_train {name}") != (N, Cc, H, W):
            raise ValueError(f"gaussian_rate_train: {name} {tuple(t.shape)} against y {tuple(y.shape)}")
    if _bs(mu) != _bs(sigma) or (dmu is not None and dsigma is not None and _bs(dmu) != _bs(dsigma)):
        raise ValueError("gaussian_rate_train: mu / sigma (and dmu / dsigma) must share a batch stride")
    ws = None
    if bits is not None or loss is not None:
        ws = _workspace(N * int(lib().dcvic_rate_blocks(Cc * H * W)), y.device, "rate_train", torch.float64)
    check(lib().dcvic_gaussian_rate_train_f32(_p(y), _bs(y), _p(mu), _p(sigma), _bs(mu), _p(noise), _bs(noise), _p(_flat_f32(weights, N, "gaussian_rate_train: sample weights")),
                                              float(scale), _p(y_hat), _bs(y_hat), _p(lik), _bs(lik), _p(_flat_f32(bits, N, "gaussian_rate_train: bits")),
                                              _p(_flat_f32(loss, 1, "gaussian_rate_train: loss")), _p(dy), _bs(dy), _p(dmu), _p(dsigma),
                                              _bs(dmu if dmu is not None else dsigma), _p(ws), N, Cc, H * W, _stream()), "gaussian_rate_train")


def eb_rate_train(z: Tensor, noise: Tensor, params: Sequence[Tensor], medians: Tensor, weights: Optional[Tensor], scale: float,
                  z_hat: Optional[Tensor] = None, lik: Optional[Tensor] = None, bits: Optional[Tensor] = None, loss: Optional[Tensor] = None,
                  dz: Optional[Tensor] = None, grads: Optional[Sequence[Tensor]] = None) -> None:
    """dcvic_eb_rate_train_f32 on contiguous [N, C, H, W]: `params` are the 14 RAW parameter tensors in the order of EB_PARAM_NAMES,
    `medians` a [C] view (quantiles[:, 0, 1]); bits, loss and the 14 `grads` ACCUMULATE, every other given output is overwritten."""
    N, Cc, H, W = _chk4(z, "eb_rate_train z")
    for t, name in ((z, "z"), (noise, "noise"), (z_hat, "z_hat"), (lik, "lik"), (dz, "dz")):
        if t is not None and (_chk4(t, f"eb_rate_train {name}") != (N, Cc, H, W) or not t.is_contiguous()):
            raise ValueError(f"eb_rate_train: {name} must be contiguous {tuple(z.shape)}")
    if medians.dtype != torch.float32 or not medians.is_cuda or medians.dim() != 1 or medians.numel() != Cc:
        raise ValueError(f"eb_rate_train: medians must be a [C] fp32 device view, got {tuple(medians.shape)}")
    ps, gs = _eb_struct(params, Cc, "eb_rate_train params"), _eb_struct(grads, Cc, "eb_rate_train grads")
    ws = None
    if bits is not None or loss is not None:
        ws = _workspace(int(lib().dcvic_eb_rate_train_workspace_doubles(N, Cc, H * W)), z.device, "eb_rate_train", torch.float64)
    check(lib().dcvic_eb_rate_train_f32(_p(z), _p(noise), ctypes.addressof(ps), _p(medians), max(1, medians.stride(0)), _p(_flat_f32(weights, N, "eb_rate_train: sample weights")),
                                        float(scale), _p(z_hat), _p(lik), _p(_flat_f32(bits, N, "eb_rate_train: bits")), _p(_flat_f32(loss, 1, "eb_rate_train: loss")),
                                        _p(dz), ctypes.addressof(gs) if gs is not None else None, _p(ws), N, Cc, H * W, _stream()), "eb_rate_train")


def eb_aux_loss(params: Sequence[Tensor], quantiles: Tensor, target: Tensor, dquantiles: Optional[Tensor] = None, accumulate: bool = False,
                want_value: bool = True) -> Optional[Tensor]:
    """dcvic_eb_aux_loss_f32: the value (1-element device tensor, or None) of EntropyBottleneck.loss(); its gradient w.r.t. `quantiles`
    [C, 1, 3] is written (or, with accumulate, added) to `dquantiles` when given."""
    Cc = quantiles.shape[0]
    for t, n, name in ((quantiles, 3 * Cc, "quantiles"), (target, 3, "target"), (dquantiles, 3 * Cc, "dquantiles")):
        _flat_f32(t, n, f"eb_aux_loss: {name}")
    ps = _eb_struct(params, Cc, "eb_aux_loss params")
    aux = torch.empty(1, dtype=torch.float32, device=quantiles.device) if want_value else None
    check(lib().dcvic_eb_aux_loss_f32(ctypes.addressof(ps), _p(quantiles), _p(target), _p(aux), _p(dquantiles), 1 if accumulate else 0, Cc, _stream()),
          "eb_aux_loss")
    return aux


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, b1: float, b2: float, eps: float, step: int, gscale: Optional[Tensor]) -> None:
    check(lib().dcvic_adam_step_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, b1, b2, eps, step, _p(gscale), _stream()), "adam_step")


def clip_scale(sumsq: Tensor, max_norm: float) -> Tensor:
    out = torch.empty(1, dtype=torch.float32, device=sumsq.device)
    check(lib().dcvic_clip_scale_f32(_p(sumsq), max_norm, _p(out), _stream()), "clip_scale")
    return out


def resample2(x: Tensor, down: bool) -> Tensor:
    N, Cc, H, W = _chk4(x, "resample x")
    if not x.is_contiguous():
        raise ValueError("resample2 needs a contiguous map")
    if down:
        out = torch.empty((N, Cc, H // 2, W // 2), dtype=torch.float32, device=x.device)
        check(lib().dcvic_resample2_f32(1, _p(x), _p(out), N * Cc, H // 2, W // 2, _stream()), "resample2")
    else:
        out = torch.empty((N, Cc, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        check(lib().dcvic_resample2_f32(0, _p(x), _p(out), N * Cc, H, W, _stream()), "resample2")
    return out


def u8_resample_crop(slab: Tensor, used: int, desc_host: int, N: int, S: int, table: Tensor, out: Tensor, stream: Optional[int] = None,
                     desc_off: int = 0) -> None:
    """The data feed's one launch per batch (csrc/data.hip, include/dcvic_data.h): `slab` a device uint8 tensor whose first `used` bytes
    hold N dcvic_crop_desc at `desc_off`, the resampling tables and the uint8 source windows (train/data.py slab_layout); `desc_host` the
    address of the same N descriptors in host memory, on which the entry point makes its checks; `table` the 256 fp32 of the
    uint8 -> [-1, 1] conversion; `out` [N, 3, S, S] fp32, written whole.  Launches on `stream` (a HIP stream handle), else the current one."""
    if slab.dtype != torch.uint8 or not slab.is_cuda or not slab.is_contiguous() or not 0 < used <= slab.numel():
        raise ValueError(f"u8_resample_crop: slab {slab.dtype} {tuple(slab.shape)} {slab.device}, used {used}")
    if table.dtype != torch.float32 or table.numel() != 256 or not table.is_contiguous() or table.device != slab.device:
        raise ValueError(f"u8_resample_crop: table {table.dtype} {tuple(table.shape)} {table.device}")
    if out.dtype != torch.float32 or tuple(out.shape) != (N, 3, S, S) or not out.is_contiguous() or out.device != slab.device:
        raise ValueError(f"u8_resample_crop: out {out.dtype} {tuple(out.shape)} {out.device}, expected ({N}, 3, {S}, {S}) fp32 on {slab.device}")
    if slab.device.index != torch.cuda.current_device():
        raise ValueError(f"u8_resample_crop: slab lives on {slab.device} but the current HIP device is cuda:{torch.cuda.current_device()}")
    check(lib().dcvic_u8_resample_crop_f32(_p(slab), int(used), _p(slab) + int(desc_off), int(desc_host), N, S, _p(table), _p(out),
                                           _stream() if stream is None else stream), "u8_resample_crop")
