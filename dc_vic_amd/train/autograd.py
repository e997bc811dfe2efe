"""A small reverse-mode tape over the HIP kernels -- what torch.autograd does for the reference's training step
(src/trainer/dual_cond_gan_distortion_vq_code_trainer.py:135-190: `l_total.backward()`, `d_loss.backward()`).

`Var` wraps a device tensor and its gradient; every differentiable op runs the inference kernel forward, records a
closure on the tape, and the closure launches the backward kernels (csrc/train.hip) or -- for the data gradient of a
convolution -- the forward convolution kernel on transposed / flipped weights.  Parameters live in flat buffers
(`ParamGroup`): weight gradients are accumulated straight into the flat gradient buffer, so Adam, gradient clipping and
the data-parallel all-reduce each see ONE contiguous tensor.  No torch autograd, no torch compute op on the path.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Union

import torch
import torch.nn as nn

from .. import ops
from ..layers import ActNorm, BatchNorm2d, Conv2d, ConvTranspose2d, GroupNorm, LayerNormC, Linear, copy_kernel_flags, invalidate_weight_caches
from . import kernels as K

Tensor = torch.Tensor


class Var:
    __slots__ = ("data", "grad", "needs_grad")

    def __init__(self, data: Tensor, needs_grad: bool = True):
        self.data = data
        self.grad: Optional[Tensor] = None
        self.needs_grad = needs_grad

    @property
    def shape(self):
        return self.data.shape


def const(t: Tensor) -> Var:
    return Var(t, needs_grad=False)


class ParamGroup:
    """The trainable parameters of some modules as views of ONE flat fp32 buffer (+ flat grad / Adam moments)."""

    def __init__(self, modules: Sequence[nn.Module], device, select: Optional[Callable[[str], bool]] = None):
        """`select` (optional): called with a parameter's name within its module (as named_parameters gives it); only the parameters it
        accepts join the group.  The others keep their own storage and receive no gradient from a Ctx of this group."""
        self.params: List[nn.Parameter] = []
        seen = set()
        for m in modules:
            for name, p in m.named_parameters():
                if select is not None and not select(name):
                    continue
                if id(p) not in seen and p.dtype == torch.float32:
                    seen.add(id(p))
                    self.params.append(p)
        n = sum(p.numel() for p in self.params)
        self.flat = torch.empty(n, dtype=torch.float32, device=device)
        self.grad = torch.zeros(n, dtype=torch.float32, device=device)
        self.m = torch.zeros(n, dtype=torch.float32, device=device)
        self.v = torch.zeros(n, dtype=torch.float32, device=device)
        self._gview: Dict[int, Tensor] = {}
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view(p.shape)           # the module now reads / Adam writes the flat buffer
            self._gview[id(p)] = self.grad[off:off + k].view(p.shape)
            off += k
        self.modules = list(modules)
        self.step_count = 0

    def numel(self) -> int:
        return self.flat.numel()

    def grad_of(self, p: nn.Parameter) -> Optional[Tensor]:
        return self._gview.get(id(p))

    def zero_grad(self) -> None:
        self.grad.zero_()

    def refresh_plans(self) -> None:
        """The flat buffer was updated in place (Adam kernel): cached packed weights / beta vectors are stale."""
        # (a whole model in the group: its captured hipGraphs hold the old packed weights; a module that was NOT trainable in some Ctx --
        # the discriminator inside the generator step -- cached a flipped / transposed COPY of its weights as its data-gradient plan)
        for mod in self.modules:
            invalidate_weight_caches(mod)


class Ctx:
    """One forward/backward pass: the tape and the parameter groups that receive weight gradients."""

    def __init__(self, groups: Sequence[ParamGroup] = ()):
        self.tape: List[Callable[[], None]] = []
        self.groups = list(groups)

    def pgrad(self, p: Optional[nn.Parameter]) -> Optional[Tensor]:
        if p is None:
            return None
        for g in self.groups:
            v = g.grad_of(p)
            if v is not None:
                return v
        return None

    def record(self, entry: Callable[[], None]) -> None:
        """Append one tape entry: backward() runs the entries last-in first-out, so this one runs after every entry recorded later."""
        self.tape.append(entry)

    def op(self, data: Tensor, backward: Callable[[Tensor], None], needs_grad: bool = True) -> Var:
        """The frame of a tape op: the output Var over `data`, and one entry that calls backward(out.grad) if a gradient arrived."""
        out = Var(data, needs_grad)

        def entry():
            if out.grad is not None:
                backward(out.grad)
        self.record(entry)
        return out

    def backward(self) -> None:
        for fn in reversed(self.tape):
            fn()
        self.tape = []

    def discard(self) -> None:
        """Forget the recorded pass without running it (a skipped step): the entries and what they hold are released."""
        self.tape = []


def acc(v: Var, g: Tensor) -> None:
    """v.grad += g (out of place: a gradient tensor may be shared by several consumers)."""
    if not v.needs_grad:
        return
    if v.grad is None:
        v.grad = g
    else:
        v.grad = K.ew(K.EW_ADD, None, v.grad.contiguous(), g.contiguous())


def _dense(t: Tensor) -> Tensor:
    return t if t.is_contiguous() else ops.copy_planes(torch.empty(t.shape, dtype=torch.float32, device=t.device), t, t.shape[2], t.shape[3])


# ------------------------------------------------------------------------------------------- channel views
def _cat(datas: Sequence[Tensor]) -> Tensor:
    N, _, H, W = datas[0].shape
    buf = torch.empty((N, sum(d.shape[1] for d in datas), H, W), dtype=torch.float32, device=datas[0].device)
    off = 0
    for d in datas:
        ops.copy_planes(buf[:, off:off + d.shape[1]], d, H, W)
        off += d.shape[1]
    return buf


def _hand_out(g: Tensor, parts: Sequence[Var]) -> None:
    """Consecutive channel ranges of `g`, as dense copies, to the parts that take a gradient."""
    off = 0
    for p in parts:
        c = p.shape[1]
        if p.needs_grad:
            acc(p, _dense(g[:, off:off + c]))
        off += c


def split_channels(ctx: Ctx, parent: Var, sizes: Sequence[int]) -> List[Var]:
    """Vars over consecutive channel-slice views of `parent`.  The entry recorded HERE runs after every consumer of the views: it
    gathers the gradients that arrived (zeros where none did) into one buffer of the parent's shape and adds it to the parent's."""
    if sum(sizes) != parent.shape[1]:
        raise ValueError(f"split_channels: sizes {tuple(sizes)} of {parent.shape[1]} channels")
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    views = [Var(parent.data[:, o:o + c], parent.needs_grad) for o, c in zip(offs, sizes)]

    def gather():
        if all(v.grad is None for v in views):
            return
        buf = torch.zeros(parent.shape, dtype=torch.float32, device=parent.data.device)
        for v, o, c in zip(views, offs, sizes):
            if v.grad is not None:
                ops.copy_planes(buf[:, o:o + c], v.grad, parent.shape[2], parent.shape[3])
        acc(parent, buf)
    ctx.record(gather)
    return views


def join_channels(ctx: Ctx, buf: Tensor, parts: Sequence[Var]) -> Var:
    """A Var over `buf`, whose consecutive channel slices ARE the parts' data (written there through `out=`): its gradient is handed
    to the parts slice by slice."""
    if sum(p.shape[1] for p in parts) != buf.shape[1]:
        raise ValueError(f"join_channels: parts of {[p.shape[1] for p in parts]} channels in a buffer of {buf.shape[1]}")
    return ctx.op(buf, lambda g: _hand_out(g, parts))


def cat_channels(ctx: Ctx, parts: Sequence[Var]) -> Var:
    return join_channels(ctx, _cat([p.data for p in parts]), parts)


# ------------------------------------------------------------------------------------------- convolution family
def _dgrad_plan(mod) -> ops.ConvPlan:
    w = mod.weight.detach()
    if isinstance(mod, Linear):
        return ops.ConvPlan(w.t().contiguous(), None, "conv")
    if isinstance(mod, ConvTranspose2d):
        # adjoint of ConvTranspose2d(k5, s2, p2, op1) = Conv2d(k5, s2, p2) with the same [Cin, Cout, k, k] tensor read as [out, in, k, k];
        # of ConvTranspose2d(k3, s1, p1) (the hyper-decoder branches' conv3) = Conv2d(k3, s1, p1) on it
        if mod.kernel_size == 3:
            return ops.ConvPlan(w, None, "conv", stride=1, pad=(1, 1))
        return ops.ConvPlan(w, None, "conv", stride=2, pad=(2, 2))
    k, s, p = mod.kernel_size, mod.stride, mod.padding
    if mod.asym_pad:
        raise NotImplementedError("the ldm Downsample conv is encoder-side only (never differentiated)")
    if s == 1:
        plan = ops.ConvPlan(w.flip(2, 3).transpose(0, 1).contiguous(), None, "conv", pad=(k - 1 - p, k - 1 - p))
        # the data gradient of a Conv2d(k3, s1, p1) is again one: Winograd (F(4x4) too) wherever the forward layer opted in (layers.allow_winograd)
        return copy_kernel_flags(plan, mod, wino=(k, p) == (3, 1))
    if (k, s, p) == (4, 2, 1):
        # adjoint = ConvTranspose2d(k4, s2, p1): output row 2m+py takes (input row, ky) in {(m-1, 3), (m, 1)} for py = 0 and
        # {(m, 2), (m+1, 0)} for py = 1 (oy = 2 iy - 1 + ky); four 2x2 sub-pixel convolutions
        ks = ((3, 1), (2, 0))
        wt = w.transpose(0, 1)                                   # [Cin_conv (out of the adjoint), Cout_conv, ky, kx]
        ph = []
        for py in (0, 1):
            for px in (0, 1):
                ph.append(wt[:, :, list(ks[py])][:, :, :, list(ks[px])].contiguous())
        return ops.ConvPlan.from_phases2(ph)
    if (k, s, p) == (5, 2, 2):
        # adjoint (even input sides) = ConvTranspose2d(k5, s2, p2, op1) with the same [Cout, Cin, k, k] tensor read as [in, out, k, k]:
        # the ELIC encoder's conv1..conv4 and the hyper-encoder's conv2 / conv3
        return ops.ConvPlan(w, None, "convT")
    raise NotImplementedError(f"conv dgrad for k{k} s{s} p{p}")


_DIFF_ACTS = (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU02, ops.ACT_HALF_TANH)    # derivative from the OUTPUT (K.EW_ACT_GRAD)


def _wgrad_geometry(mod):
    """(KH, KW, stride, pad, transposed) of the weight gradient of `mod`; transposed: G and X swap roles, result [Cin][Cout][k][k]."""
    if isinstance(mod, ConvTranspose2d):
        return (5, 5, 2, 2, True) if mod.kernel_size == 5 else (3, 3, 1, 1, True)
    if isinstance(mod, Linear):
        return 1, 1, 1, 0, False
    return mod.kernel_size, mod.kernel_size, mod.stride, mod.padding, False


def _check_s2_input(mod, H: int, W: int) -> None:
    if isinstance(mod, Conv2d) and (mod.kernel_size, mod.stride, mod.padding) == (5, 2, 2) and (H % 2 or W % 2):
        raise ValueError(f"differentiable Conv2d(k5, s2, p2) needs even input sides, got {H}x{W}")


# The weight gradient of a convolution of several sources: one dcvic_conv_wgrad_src_f32 launch per source (True), or one cat of the
# sources + one dcvic_conv_wgrad_f32 launch (False).  Same bits.  Measured at batch 8 x 256x256 (tools/analysis_tape_bench.py,
# profiles/analysis_tape_bench.json): 56.99 ms per step per source, 56.79 ms with the cat, the per-source form slower in every alternating
# round (two or three launch pairs per layer against a few plane copies and one pair), so the cat form is the default.
WGRAD_PER_SOURCE = False


def _cached(mod, attr: str, trainable: bool, build):
    """build(), kept on a frozen layer as `attr` = (mod._key(), value): keyed by the weights' version, so a reloaded checkpoint rebuilds
    it.  Trainable weights move every step: nothing is read from or left in the cache."""
    if trainable:
        return build()
    cached = getattr(mod, attr, None)
    if cached is None or cached[0] != mod._key():
        cached = (mod._key(), build())
        setattr(mod, attr, cached)
    return cached[1]


def _forward_plan(mod, trainable: bool, ups: bool) -> ops.ConvPlan:
    """The fp32 plan of `mod` on the tape.  Training ignores the decoder precision: wino / wino44 are copied, never the bf16 flag
    (layers.allow_bf16 is inference only)."""
    if ups:      # the differentiable Upsample conv is an explicit nearest x2, then this plain 3x3 convolution (ldm model.py:53-57)
        return _cached(mod, "_plain_plan", trainable, lambda: copy_kernel_flags(ops.ConvPlan(mod.weight, mod.bias, "conv", pad=(1, 1)), mod))
    if trainable:                        # built from the live weights (the SFT fusion blocks train; their 3x3 convs stay on Winograd)
        return copy_kernel_flags(mod._build_plan(), mod)
    return mod._get_plan(bf16=False)


def _param_grads(ctx: Ctx, mod, gw: Tensor, g: Tensor, datas: Sequence[Tensor]) -> None:
    """The weight gradient (of one source: on its dense form; of several: written per source into its channel range of the layer's
    [Cout, Cin, k, k] gradient, or from their cat) and the bias gradient, added into the flat gradient buffer."""
    KH, KW, st, pd, swapped = _wgrad_geometry(mod)
    if len(datas) > 1 and WGRAD_PER_SOURCE:
        off = 0
        for d in datas:
            K.conv_wgrad_src(g, d, gw, off, KH, KW, st, pd)
            off += d.shape[1]
    else:
        xs = _dense(datas[0]) if len(datas) == 1 else _cat(datas)
        if swapped:
            K.conv_wgrad(xs, g, gw, KH, KW, st, pd)             # roles swapped: result is [Cin][Cout][k][k]
        else:
            K.conv_wgrad(g, xs, gw, KH, KW, st, pd)
    gb = ctx.pgrad(mod.bias)
    if gb is not None:
        K.sum_rows(K.chan_reduce(g), gb, accumulate=True)


def conv(ctx: Ctx, x: Union[Var, Sequence[Var]], mod, act: int = ops.ACT_NONE, out: Optional[Tensor] = None, res: Optional[Var] = None,
         init: Optional[Var] = None) -> Var:
    """Conv2d / ConvTranspose2d / Linear stand-ins of dc_vic_amd.layers; bias and (optionally) ReLU / LeakyReLU / 0.5 tanh fused forward;
    `out`: a destination view, e.g. one half of the hyper-decoder's output.
    A plain Conv2d also reads the channel concatenation of several Vars (views welcome: each with its own batch stride), never
    materialised: act(conv(cat x) [+ init] + bias) [+ res].  One data gradient over all input channels, whose channel ranges are added to
    the sources that need one (a constant source -- the one-hot VQ feature -- takes none), and one weight gradient."""
    if act not in _DIFF_ACTS:
        raise ValueError("only activations whose derivative follows from the output (ReLU, LeakyReLU, 0.5 tanh) may be fused into a differentiable conv")
    if act != ops.ACT_NONE and res is not None:
        raise ValueError("conv_multi: the residual is added after the activation, whose derivative is then not a function of the output")
    srcs = [x] if isinstance(x, Var) else list(x)
    ups = isinstance(mod, Conv2d) and mod.upsample
    if (len(srcs) != 1 or res is not None or init is not None) and (not isinstance(mod, Conv2d) or ups or mod.asym_pad):
        raise NotImplementedError("conv_multi: plain Conv2d layers only")
    if not 1 <= len(srcs) <= ops.L.MAX_SRC:
        raise ValueError(f"conv_multi: 1..{ops.L.MAX_SRC} sources, got {len(srcs)}")
    chans = [int(v.shape[1]) for v in srcs]
    if isinstance(mod, Conv2d) and sum(chans) != mod.in_channels:
        raise ValueError(f"conv_multi: sources hold {chans} channels, the layer reads {mod.in_channels}")
    if any(v.needs_grad for v in srcs):
        _check_s2_input(mod, srcs[0].shape[2], srcs[0].shape[3])
    gw = ctx.pgrad(mod.weight)
    trainable = gw is not None
    datas = [K.resample2(_dense(srcs[0].data), down=False)] if ups else [v.data for v in srcs]
    y = _forward_plan(mod, trainable, ups)(datas, act=act, out=out, res=res.data if res is not None else None,
                                           init=init.data if init is not None else None)

    def backward(g):
        g = _dense(g)
        if res is not None:
            acc(res, g)
        if act != ops.ACT_NONE:
            g = K.ew(K.EW_ACT_GRAD, g, _dense(y), act=act)
        if init is not None:
            acc(init, g)
        if any(v.needs_grad for v in srcs):
            dx = _cached(mod, "_dgrad", trainable, lambda: _dgrad_plan(mod))(g)
            _hand_out(K.resample2(dx, down=True) if ups else dx, srcs)
        if trainable:
            _param_grads(ctx, mod, gw, g, datas)
    return ctx.op(y, backward)


conv_multi = conv       # the name the several-source form had as a function of its own


# ------------------------------------------------------------------------------------------- normalisation
def group_norm(ctx: Ctx, x: Var, mod: GroupNorm, act: int = ops.ACT_NONE) -> Var:
    xd = x.data

    def backward(g):
        dx, dg, db = K.groupnorm_bwd(xd, g, mod.weight, mod.bias, mod.num_groups, mod.eps, act)
        acc(x, dx)
        gw, gb = ctx.pgrad(mod.weight), ctx.pgrad(mod.bias)
        if gw is not None:
            K.sum_rows(dg, gw, accumulate=True)
            K.sum_rows(db, gb, accumulate=True)
    return ctx.op(ops.groupnorm(xd, mod.weight, mod.bias, mod.num_groups, mod.eps, act), backward)


def layer_norm_c(ctx: Ctx, x: Var, mod: LayerNormC) -> Var:
    xd = _dense(x.data)

    def backward(g):
        dx, part = K.layernorm_c_bwd(xd, _dense(g), mod.weight, mod.eps)
        acc(x, dx)
        gw, gb = ctx.pgrad(mod.weight), ctx.pgrad(mod.bias)
        if gw is not None:
            Cc = xd.shape[1]
            tmp = torch.empty(2 * Cc, dtype=torch.float32, device=xd.device)
            K.sum_rows(part, tmp, accumulate=False)
            K.ew(K.EW_ADD, None, gw, tmp[:Cc], out=gw)
            K.ew(K.EW_ADD, None, gb, tmp[Cc:], out=gb)
    return ctx.op(ops.layernorm_c(xd, mod.weight, mod.bias, mod.eps), backward)


_NORM_ACTS = (ops.ACT_NONE, ops.ACT_LRELU02)


def batch_norm(ctx: Ctx, x: Var, mod: BatchNorm2d, act: int = ops.ACT_NONE) -> Var:
    """nn.BatchNorm2d in training mode (+ fused LeakyReLU(0.2)): this call's own batch statistics, the running statistics and
    num_batches_tracked updated now, the gradients of csrc/bn_train.hip (dgamma / dbeta added into the flat gradient buffer)."""
    if act not in _NORM_ACTS:
        raise ValueError("batch_norm: only LeakyReLU(0.2) may be fused")
    if not mod.training:
        raise NotImplementedError("batch_norm: the eval-mode forward (running statistics) is not built: the discriminators stay in train mode")
    xd = x.data
    y, mean, rstd = K.bn_train_fwd(xd, mod.weight, mod.bias, mod.running_mean, mod.running_var, mod.momentum, mod.eps, act)
    mod.num_batches_tracked.add_(1)

    def backward(g):
        acc(x, K.bn_train_bwd(xd, g, y if act != ops.ACT_NONE else None, mean, rstd, mod.weight, ctx.pgrad(mod.weight), ctx.pgrad(mod.bias),
                              accumulate=True, act=act))
    return ctx.op(y, backward)


def act_norm(ctx: Ctx, x: Var, mod: ActNorm, act: int = ops.ACT_NONE) -> Var:
    """taming's ActNorm (+ fused LeakyReLU(0.2)): scale * (x + loc), initialised from the first training batch (loc = -mean,
    scale = 1 / (unbiased std + 1e-6)); dloc / dscale are added into the flat gradient buffer."""
    if act not in _NORM_ACTS:
        raise ValueError("act_norm: only LeakyReLU(0.2) may be fused")
    xd = x.data
    if mod.training and not mod.is_initialized():
        mean, std = K.bn_stats(xd)
        mod.loc.data.copy_(mean.neg_().view_as(mod.loc))                # once per module: C values
        mod.scale.data.copy_(std.add_(1e-6).reciprocal_().view_as(mod.scale))
        mod.mark_initialized()
    y = K.actnorm_fwd(xd, mod.loc, mod.scale, act)

    def backward(g):
        acc(x, K.actnorm_bwd(xd, g, y if act != ops.ACT_NONE else None, mod.loc, mod.scale, ctx.pgrad(mod.loc), ctx.pgrad(mod.scale),
                             accumulate=True, act=act))
    return ctx.op(y, backward)


# ------------------------------------------------------------------------------------------- elementwise
def activation(ctx: Ctx, x: Var, act: int) -> Var:
    xd = _dense(x.data)
    y = ops.activation(xd, act)
    ref = xd if act in (ops.ACT_SWISH, ops.ACT_GELU) else y
    return ctx.op(y, lambda g: acc(x, K.ew(K.EW_ACT_GRAD, _dense(g), ref, act=act)))


def add(ctx: Ctx, a: Var, b: Var, out: Optional[Tensor] = None) -> Var:
    """a + b; `out`: a destination view (one CHARM slice of the y_hat buffer)."""
    def backward(g):
        acc(a, g)
        acc(b, g)
    return ctx.op(ops.add(_dense(a.data), _dense(b.data), out=out), backward)


def nlam_gate(ctx: Ctx, x: Var, t: Var, a: Var) -> Var:
    """x + t * sigmoid(a)   (ChengNLAM, cheng_nlam.py:23-27)."""
    xd, td, ad = _dense(x.data), _dense(t.data), _dense(a.data)

    def backward(g):
        g = _dense(g)
        acc(x, g)
        acc(t, K.ew(K.EW_MUL_SIGMOID, g, ad))
        acc(a, K.ew(K.EW_MUL_DSIGMOID, g, td, ad))
    return ctx.op(ops.add_mul_sigmoid(xd, td, ad), backward)


def sft(ctx: Ctx, dec: Var, scale: Var, shift: Var, w: float = 1.0) -> Var:
    """dec + w * (dec * scale + shift)   (FuseSftBlock, codeformer_layers.py:65-66)."""
    dd, sd, hd = _dense(dec.data), _dense(scale.data), _dense(shift.data)

    def backward(g):
        g = _dense(g)
        acc(dec, K.ew(K.EW_SFT_DEC, g, sd, w=w))
        acc(scale, K.ew(K.EW_SFT_SCALE, g, dd, w=w))
        acc(shift, K.ew(K.EW_SFT_SHIFT, g, w=w))
    return ctx.op(ops.sft(dd, sd, hd, w=w), backward)


def chan_affine(ctx: Ctx, x: Var, s: Var, t: Var, add_x: bool = False) -> Var:
    """x * (1 + s[n][c]) + t[n][c] (+ x)   (BetaScaleShiftModule.forward; s, t: [B, C, 1, 1] with B in {1, N})."""
    xd = _dense(x.data)
    N, Cc = xd.shape[:2]
    sv, tv = s.data.reshape(s.data.shape[0], Cc).contiguous(), t.data.reshape(t.data.shape[0], Cc).contiguous()

    def backward(g):
        g = _dense(g)
        if x.needs_grad:
            dx = K.ew(K.EW_CHAN_SCALE, g, sv, vec_bs=Cc if sv.shape[0] > 1 else 0)
            if add_x:
                dx = K.ew(K.EW_ADD, None, dx, g)
            acc(x, dx)
        ds, dt = K.chan_reduce(g, xd), K.chan_reduce(g)                   # [N, C]
        if sv.shape[0] == 1:
            ds1, dt1 = torch.empty((1, Cc), dtype=torch.float32, device=g.device), torch.empty((1, Cc), dtype=torch.float32, device=g.device)
            K.sum_rows(ds, ds1.view(-1), accumulate=False)
            K.sum_rows(dt, dt1.view(-1), accumulate=False)
            ds, dt = ds1, dt1
        acc(s, ds.view(s.data.shape))
        acc(t, dt.view(t.data.shape))
    return ctx.op(ops.chan_affine(xd, sv, tv, add_=xd if add_x else None), backward)


def upsample2(ctx: Ctx, x: Var) -> Var:
    return ctx.op(K.resample2(_dense(x.data), down=False), lambda g: acc(x, K.resample2(_dense(g), down=True)))


# ------------------------------------------------------------------------------------------- attention
def attn_single_head(ctx: Ctx, qkv: Var, Cc: int) -> Var:
    """ldm AttnBlock core (model.py:186-196): forward = the fused flash kernel; backward recomputes the probabilities
    (bgemm + column softmax) and forms dV, dP, dS, dQ, dK with the strided batched GEMM."""
    qd = _dense(qkv.data)
    N, _, H, W = qd.shape
    HW = H * W
    scale = float(int(Cc) ** (-0.5))

    def backward(g):
        g = _dense(g)                                              # dO [N, C, HW]
        bs = 3 * Cc * HW
        q, k, v = qd[:, :Cc], qd[:, Cc:2 * Cc], qd[:, 2 * Cc:]
        St = torch.empty((N, HW, HW), dtype=torch.float32, device=qd.device)       # St[j][i] = P(query i -> key j)
        ops.bgemm(k, (bs, 1, HW), q, (bs, HW, 1), St, (HW * HW, HW), N, HW, HW, Cc, alpha=scale)
        ops.softmax_c_(St, N, HW, HW)
        dqkv = torch.empty_like(qd)
        dq, dk, dv = dqkv[:, :Cc], dqkv[:, Cc:2 * Cc], dqkv[:, 2 * Cc:]
        # dV[c][j] = sum_i dO[c][i] St[j][i]
        ops.bgemm(g, (Cc * HW, HW, 1), St, (HW * HW, 1, HW), dv, (bs, HW), N, Cc, HW, HW)
        # dSt[j][i] = sum_c V[c][j] dO[c][i]
        dSt = torch.empty_like(St)
        ops.bgemm(v, (bs, 1, HW), g, (Cc * HW, HW, 1), dSt, (HW * HW, HW), N, HW, HW, Cc)
        dS = K.softmax_c_bwd(St, dSt, scale)                        # includes the c^-0.5 factor
        # dQ[c][i] = sum_j K[c][j] dS[j][i] ; dK[c][j] = sum_i Q[c][i] dS[j][i]
        ops.bgemm(k, (bs, HW, 1), dS, (HW * HW, HW, 1), dq, (bs, HW), N, Cc, HW, HW)
        ops.bgemm(q, (bs, HW, 1), dS, (HW * HW, 1, HW), dk, (bs, HW), N, Cc, HW, HW)
        acc(qkv, dqkv)
    return ctx.op(ops.attn_fused(qd, Cc), backward)


def swin_attention(ctx: Ctx, qkv: Var, table: nn.Parameter, heads: int, ws: int, shift: int) -> Var:
    qd = _dense(qkv.data)

    def backward(g):
        gt = ctx.pgrad(table)
        dt = gt if gt is not None else torch.zeros_like(table)
        acc(qkv, K.swin_attn_bwd(qd, _dense(g), table, dt, heads, ws, shift, accumulate=gt is not None))
    return ctx.op(ops.swin_attn(qd, table, heads, ws, shift), backward)


# ------------------------------------------------------------------------------------------- losses (seed the gradients)
def mse_loss(ctx: Ctx, a: Var, target: Tensor, weight: float) -> Tensor:
    """weight * mean((a - target)^2): value as a 1-element device tensor, gradient seeded into `a`."""
    ad, td = _dense(a.data), _dense(target)
    n = ad.numel()
    val = K.reduce_loss(K.SUM_SQ_ERR, ad, td, weight / n)
    acc(a, K.ew(K.EW_MSE_GRAD, None, ad, td, w=weight / n))
    return val


def l1_loss(ctx: Ctx, a: Var, target: Tensor, weight: float) -> Tensor:
    """weight * mean|a - target| (distortion_loss.py `L1Loss`): value (fp64, 1 element) and gradient weight * sign(a - target) / numel,
    sign(0) = 0, from one pass of csrc/msssim_loss.hip; the gradient is seeded into `a`."""
    ad, td = _dense(a.data), _dense(target)
    val, da = K.abs_err(ad, td, weight / ad.numel(), want_grad=a.needs_grad)
    if da is not None:
        acc(a, da)
    return val


MS_SSIM_MIN_SIDE = 160              # pytorch-msssim asserts min(H, W) > (11 - 1) * 2^4


def ms_ssim_loss(ctx: Ctx, fake: Var, real: Tensor, weight: float) -> Tensor:
    """weight * (1 - MS_SSIM(data_range=1, size_average=True, channel=3)(real, fake)) on the images as they are (distortion_loss.py
    `MSSSIMLoss`, applied to the trainer's [-1, 1] images with `fake` unclamped): value (fp64, 1 element) and the gradient with respect
    to `fake` from csrc/msssim_loss.hip, seeded into `fake`; `real` is a constant.  RGB only, min(H, W) > 160."""
    fd, rd = _dense(fake.data), _dense(real)
    if fd.dim() != 4 or fd.shape[1] != 3:
        raise ValueError(f"ms_ssim_loss: RGB images [N, 3, H, W], got {tuple(fd.shape)}")
    N, Cc, H, W = fd.shape
    if min(H, W) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"ms_ssim_loss: images of {H} x {W}, MS-SSIM over five scales needs min(H, W) > {MS_SSIM_MIN_SIDE}")
    val, df, _ = K.ms_ssim_loss(rd, fd, weight / (N * Cc), want_grad=fake.needs_grad)
    if df is not None:
        acc(fake, df)
    return val


def bce_logits_loss(ctx: Ctx, x: Var, is_real: bool, weight: float) -> Tensor:
    """weight * BCEWithLogits(x, 1 or 0), mean reduction (src/losses/gan_loss.py:10-32)."""
    xd = _dense(x.data)
    n = xd.numel()
    val = K.reduce_loss(K.SUM_BCE, xd, None, weight / n, target=1 if is_real else 0)
    acc(x, K.ew(K.EW_BCE_GRAD, None, xd, w=weight / n, act=1 if is_real else 0))
    return val


def cross_entropy_loss(ctx: Ctx, logits: Var, target: Tensor, weight: float) -> Tensor:
    """weight * CrossEntropy(logits [N, C, H, W], target [N, H, W]), mean over N*H*W (cross_entropy_loss.py:10-28)."""
    ld = _dense(logits.data)
    N, Cc, H, W = ld.shape
    m = N * H * W
    nll, dl = K.cross_entropy(ld, target.contiguous(), weight / m, want_grad=True)
    val = K.reduce_loss(K.SUM, nll, None, weight / m)
    acc(logits, dl)
    return val


def focal_cross_entropy_loss(ctx: Ctx, logits: Var, target: Tensor, weight: float, gamma: float, reduction: str = "mean") -> Tensor:
    """weight * reduce((1 - p_t)^gamma * CrossEntropy(logits [N, C, H, W], target [N, H, W])) with reduce = mean over N*H*W or sum
    (cross_entropy_loss.py:33-53): value and gradient from one pass of csrc/chan_ce.hip; the gradient is seeded into `logits`."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"focal_cross_entropy_loss: reduction {reduction!r}, expected 'mean' or 'sum'")
    ld = _dense(logits.data)
    N, Cc, H, W = ld.shape
    val, dl = K.focal_ce(ld, target.contiguous(), gamma, weight / (N * H * W) if reduction == "mean" else weight, want_grad=logits.needs_grad)
    if dl is not None:
        acc(logits, dl)
    return val


def focal_cross_entropy_loss_weighted(ctx: Ctx, logits: Var, target: Tensor, w: Tensor, gamma: float) -> Tensor:
    """sum_n w[n] * sum_positions (1 - p_t)^gamma * CrossEntropy of image n (logits [N, C, H, W], target [N, H, W], w a device fp32 [N]
    vector: losses.sample_loss_weights states apply_loss_weight of the rate-distortion trainers in this form): value and gradient from
    one pass of csrc/sample_loss.hip; the gradient is seeded into `logits`."""
    val, dl, _ = K.focal_ce_sample(_dense(logits.data), target.contiguous(), w, gamma, want_grad=logits.needs_grad)
    if dl is not None:
        acc(logits, dl)
    return val


def mse_loss_weighted(ctx: Ctx, a: Var, target: Tensor, w: Tensor) -> Tensor:
    """sum_n w[n] * sum((a[n] - target[n])^2) with w a device fp32 [N] vector (losses.sample_loss_weights): value and gradient from
    one pass of csrc/sample_loss.hip over `a` (which may be a channel-slice view); the gradient is seeded into `a`."""
    val, da, _ = K.sq_err_sample(a.data, target.contiguous(), w, want_grad=a.needs_grad)
    if da is not None:
        acc(a, da)
    return val


def oasis_gan_loss(ctx: Ctx, logits: Var, target: Tensor, is_real: bool, weight: float, want_score: bool = False):
    """weight * CrossEntropy(logits [N, C, H, W], target + 1 if is_real else 0), mean over N*H*W (src/losses/oasis_gan_loss.py:40-79):
    value, gradient and -- with want_score -- mean(logits[:, 1:]) from one pass of csrc/chan_ce.hip.  Returns the value, or
    (value, score) with want_score; the gradient is seeded into `logits`."""
    ld = _dense(logits.data)
    N, Cc, H, W = ld.shape
    val, dl, score = K.oasis_ce(ld, target.contiguous(), is_real, weight / (N * H * W), want_grad=logits.needs_grad, want_score=want_score)
    if dl is not None:
        acc(logits, dl)
    return (val, score) if want_score else val


# ------------------------------------------------------------------------------------------- Gumbel-softmax VQ sample (csrc/gumbel.hip)
def gumbel_vq_latent(ctx: Ctx, logits: Var, noise: Tensor, codebook: Tensor, pq_w: Tensor, pq_b: Optional[Tensor], tau: float = 1.0):
    """hyperprior_dc_vic_model.py:254-260 with model.gumbel_sampling: the hard Gumbel-softmax sample of the code logits for the draw
    `noise` ~ Exp(1) (F.gumbel_softmax(logits, tau, hard=True, dim=1)), times the detached codebook, through the frozen post_quant_conv.
    -> (idx, latent Var).  A gradient arriving on the latent reaches `logits` through the straight-through softmax (the codebook and
    post_quant_conv take none); the softmax is recomputed from `logits` and `noise` in the backward kernel."""
    ld = _dense(logits.data)
    idx, lat = ops.gumbel_lut(ld, noise, codebook, pq_w, pq_b, tau)
    return idx, ctx.op(lat, lambda g: acc(logits, K.gumbel_lut_bwd(ld, noise, _dense(g), codebook, pq_w, tau)), needs_grad=logits.needs_grad)


# ------------------------------------------------------------------------------------------- the rate term (csrc/rate_train.hip)
def gaussian_rate(ctx: Ctx, y: Var, mu: Var, sigma: Var, noise: Tensor, weights: Optional[Tensor], scale: float, bits: Optional[Tensor],
                  loss: Optional[Tensor], dy_out: Optional[Tensor] = None, lik_out: Optional[Tensor] = None) -> Var:
    """The rate term of one Gaussian-conditional call (GaussianConditional.forward(training=True), ste_gaussian_conditional.py:16-23) in
    one pass: bits[n] += -log2 of image n's noisy likelihoods, loss[0] += sum_n scale * weights[n] * bits[n] (both accumulate: the
    caller zeroes them), and that loss term's gradients are seeded into `y`, `mu` and `sigma` now.  With `dy_out` (a [N, C, H, W] view,
    e.g. a CHARM slice of one 192-channel gradient) the gradient w.r.t. y is written there instead and the caller seeds the parent
    once; `lik_out` (a view too) takes the noisy likelihoods.  Returns y_hat = ste_round(y - mu) + mu: a gradient arriving on it goes to `y` unchanged and not to `mu`."""
    new = lambda: torch.empty(y.shape, dtype=torch.float32, device=y.data.device)
    out = ctx.op(new(), lambda g: acc(y, g), needs_grad=y.needs_grad)
    dy = dy_out if dy_out is not None else (new() if y.needs_grad else None)
    dmu, dsigma = (new() if mu.needs_grad else None), (new() if sigma.needs_grad else None)
    K.gaussian_rate_train(y.data, mu.data, sigma.data, noise, weights, scale, y_hat=out.data, lik=lik_out, bits=bits, loss=loss, dy=dy,
                          dmu=dmu, dsigma=dsigma)
    if dy is not None and dy_out is None:
        acc(y, dy)
    if dmu is not None:
        acc(mu, dmu)
    if dsigma is not None:
        acc(sigma, dsigma)
    return out


def eb_rate(ctx: Ctx, z: Var, eb, noise: Tensor, weights: Optional[Tensor], scale: float, bits: Optional[Tensor], loss: Optional[Tensor],
            lik_out: Optional[Tensor] = None) -> Var:
    """The rate term of the entropy bottleneck `eb` (EntropyBottleneck.forward(training=True)): bits / loss as in gaussian_rate; the
    loss term's gradient is seeded into `z` and, when `eb`'s parameters belong to one of ctx's groups, added to their views of the flat
    gradient buffer.  Returns z_hat = ste_round(z - medians) + medians: its gradient goes to `z` unchanged, none to the medians."""
    zd = _dense(z.data)
    out = ctx.op(torch.empty_like(zd), lambda g: acc(z, g), needs_grad=z.needs_grad)
    grads = [ctx.pgrad(getattr(eb, name)) for name in K.EB_PARAM_NAMES]
    grads = None if any(g is None for g in grads) else grads
    dz = torch.empty_like(zd) if z.needs_grad else None
    K.eb_rate_train(zd, _dense(noise), eb.raw_params(), eb.quantiles.data[:, 0, 1], weights, scale, z_hat=out.data, lik=lik_out, bits=bits, loss=loss,
                    dz=dz, grads=grads)
    if dz is not None:
        acc(z, dz)
    return out


def eb_aux_loss(ctx: Ctx, eb) -> Tensor:
    """EntropyBottleneck.loss(): sum |logits(quantiles) - target| as a 1-element device tensor; its gradient reaches `quantiles` only
    (added to the flat gradient buffer when `quantiles` belongs to one of ctx's groups)."""
    return K.eb_aux_loss(eb.raw_params(), eb.quantiles.data, eb.target, ctx.pgrad(eb.quantiles), accumulate=True)
