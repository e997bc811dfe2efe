"""Plain-torch restatement of the normalised GAN discriminators (test helper, no HIP): the PatchGAN and the OASIS U-Net built from
torch.nn modules with torch's own BatchNorm2d, ActNorm restated, and the state-dict keys of the product classes (train/nets.py),
so one synthetic state loads into both.  Runs in fp32 or fp64 on the CPU or on a device; tests/test_disc_norm_host.py pins it to
tests/golden/disc_norm.npz, which holds what the reference's own classes gave."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class ActNorm(nn.Module):
    """scale * (x + loc), both [1, C, 1, 1]; the first training call sets loc = -mean and scale = 1 / (unbiased std + 1e-6) per channel."""

    def __init__(self, num_features):
        super().__init__()
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))

    def forward(self, x):
        if self.training and int(self.initialized) == 0:
            with torch.no_grad():
                flat = x.transpose(0, 1).reshape(x.shape[1], -1)
                self.loc.copy_(-flat.mean(1).view(1, -1, 1, 1))
                self.scale.copy_(1 / (flat.std(1).view(1, -1, 1, 1) + 1e-6))
                self.initialized.fill_(1)
        return self.scale * (x + self.loc)


class SignQueue:
    """Sign decisions handed to a model's LeakyReLUs: `masks`, a list of bool tensors (True: the positive branch), is consumed one per
    LeakyReLU call in call order; `flips` records for each (positions whose own sign differs, their largest |value|, elements)."""

    def __init__(self):
        self.masks, self.flips = [], []


class LeakyReLU(nn.Module):
    """LeakyReLU(0.2); with a mask queued on the model's SignQueue, the branch is the mask's, not the value's own sign."""

    def __init__(self, signs):
        super().__init__()
        self.signs = signs

    def forward(self, v):
        if not self.signs.masks:
            return F.leaky_relu(v, 0.2)
        m = self.signs.masks.pop(0).to(v.device)
        diff = (v.detach() > 0) != m
        self.signs.flips.append((int(diff.sum()), float(v.detach()[diff].abs().max()) if diff.any() else 0.0, v.numel()))
        return torch.where(m, v, 0.2 * v)


def norm_layer(ch, norm_type, norm_kwargs):
    if norm_type == "batchnorm":
        return nn.BatchNorm2d(ch, **norm_kwargs)
    return ActNorm(ch) if norm_type == "actnorm" else nn.Identity()


def fourier(beta, L, max_beta, use_pi, include_x):
    """FourierEncoding.embed (host, fp32): beta [B] or a number -> [B, 2L (+1)] = [x,] sin(x 2^k [pi]), cos(...) of x = 2 beta / max - 1."""
    b = (torch.as_tensor(beta, dtype=torch.float32).reshape(-1, 1) / max_beta - 0.5) * 2
    f = torch.pow(torch.tensor([2.0]), torch.arange(L)).unsqueeze(0) * (math.pi if use_pi else 1.0)
    parts = [torch.sin(b * f), torch.cos(b * f)]
    return torch.cat(([b] if include_x else []) + parts, dim=1)


class _BetaCond(nn.Module):
    def _init_cond(self, max_beta_1, max_beta_2, L, cond_ch, use_pi, include_x):
        self._enc = (L, max_beta_1, max_beta_2, use_pi, include_x)
        n_in = 2 * (2 * L + 1) if include_x else 4 * L
        return nn.Sequential(nn.Linear(n_in, cond_ch), nn.ReLU(), nn.Linear(cond_ch, cond_ch))

    def _cond(self, mlp, beta_1, beta_2, x, embed=None):
        L, m1, m2, use_pi, include_x = self._enc
        embed = embed or (lambda b, mb: fourier(b, L, mb, use_pi, include_x))
        c = torch.cat([embed(beta_1, m1), embed(beta_2, m2)], dim=1).to(device=x.device, dtype=x.dtype)
        return mlp(c)[:, :, None, None]


class PatchGAN(_BetaCond):
    def __init__(self, input_nc=11, ndf=64, out_nc=1, n_layers=3, keep_shape=False, use_actnorm=False, norm_type="none", norm_kwargs={},
                 max_beta_1=-1.0, max_beta_2=-1.0, L=10, cond_ch=8, use_pi=False, include_x=True, **_):
        super().__init__()
        self.signs = SignQueue()
        norm_type = "actnorm" if use_actnorm else norm_type
        bias = norm_type != "batchnorm"
        seq = [nn.Conv2d(input_nc, ndf, 4, 2, 1), LeakyReLU(self.signs)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 2, 1, bias=bias), norm_layer(ndf * mult, norm_type, norm_kwargs), LeakyReLU(self.signs)]
        k = 3 if keep_shape else 4
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [nn.Conv2d(ndf * prev, ndf * mult, k, 1, 1, bias=bias), norm_layer(ndf * mult, norm_type, norm_kwargs), LeakyReLU(self.signs)]
        seq += [nn.Conv2d(ndf * mult, out_nc, k, 1, 1)]
        self.main = nn.Sequential(*seq)
        self.mlp = self._init_cond(max_beta_1, max_beta_2, L, cond_ch, use_pi, include_x)

    def forward(self, x, beta_1, beta_2, embed=None):
        c = self._cond(self.mlp, beta_1, beta_2, x, embed)
        return self.main(torch.cat([x, c.expand(x.shape[0], -1, x.shape[2], x.shape[3])], dim=1))


class _Emb(nn.Module):
    def __init__(self, mlp):
        super().__init__()
        self.mlp = mlp


class UNet(_BetaCond):
    def __init__(self, input_nc=3, ndf=64, n_layers=3, num_upsample=1, out_nc=128, use_actnorm=False, norm_type="none", norm_kwargs={},
                 max_beta_1=-1.0, max_beta_2=-1.0, L=10, cond_ch=8, use_pi=False, include_x=True, **_):
        super().__init__()
        self.signs = SignQueue()
        norm_type = "actnorm" if use_actnorm else norm_type
        bias = norm_type != "batchnorm"
        ch = [ndf * min(2 ** i, 8) for i in range(n_layers)]
        self.body = nn.ModuleList([nn.Sequential(nn.Conv2d(input_nc, ch[0], 4, 2, 1), LeakyReLU(self.signs))])
        for n in range(1, n_layers):
            self.body.append(nn.Sequential(nn.Conv2d(ch[n - 1], ch[n], 4, 2, 1, bias=bias), norm_layer(ch[n], norm_type, norm_kwargs), LeakyReLU(self.signs)))
        self.bottleneck = nn.Sequential(nn.Conv2d(ch[-1], ch[-1], 3, 1, 1, bias=bias), norm_layer(ch[-1], norm_type, norm_kwargs), LeakyReLU(self.signs))
        self.up_blocks = nn.ModuleList()
        for i in range(num_upsample):
            self.up_blocks.append(nn.Sequential(nn.Upsample(scale_factor=2), nn.Conv2d(ch[n_layers - 1 - i], ch[n_layers - 2 - i], 3, 1, 1),
                                                norm_layer(ch[n_layers - 2 - i], norm_type, norm_kwargs), LeakyReLU(self.signs)))
        self.head = nn.Sequential(nn.Conv2d(ch[n_layers - 1 - num_upsample], 64, 1), LeakyReLU(self.signs), nn.Conv2d(64, out_nc, 1))
        self.beta_emb = _Emb(self._init_cond(max_beta_1, max_beta_2, L, cond_ch, use_pi, include_x))

    def forward(self, x, beta_1, beta_2, embed=None):
        c = self._cond(self.beta_emb.mlp, beta_1, beta_2, x, embed)
        h = torch.cat([x, c.expand_as(x)], dim=1)                  # the reference's quirk: cond_ch must equal x's channels
        skips = []
        for blk in self.body:
            h = blk(h)
            skips.append(h)
        h = self.bottleneck(h)
        for i, blk in enumerate(self.up_blocks):
            h = blk(h) + skips[-i - 2]
        return self.head(h)


CLASSES = {"DualBetaCondTamingNLayerDiscriminator": PatchGAN, "OasisDualBetaCondTamingNLayerDiscriminator": UNet}


def build(d_type, kwargs, state, dtype=torch.float32):
    """The restated class in train mode with `state` (name -> tensor) loaded strictly, floating tensors cast to `dtype`."""
    D = CLASSES[d_type](**kwargs)
    D.load_state_dict(state, strict=True)
    return D.to(dtype).train()


def norm_buffers(D):
    """{key: tensor} of every norm layer's buffers (running_mean, running_var, num_batches_tracked, initialized), cloned."""
    leaves = ("running_mean", "running_var", "num_batches_tracked", "initialized")
    return {k: v.detach().clone() for k, v in D.state_dict().items() if k.rsplit(".", 1)[-1] in leaves}


def norm_param_names(D):
    """Keys of the norm layers' parameters (BatchNorm weight / bias, ActNorm loc / scale)."""
    out = []
    for name, m in D.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            out += [f"{name}.weight", f"{name}.bias"]
        elif isinstance(m, ActNorm):
            out += [f"{name}.loc", f"{name}.scale"]
    return out
