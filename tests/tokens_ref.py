"""What the selection-set tests share: CPU restatements of the two kernels of csrc/tokens.hip (include/dcvic_tokens.h), the torch chain
kernel B replaces, the entry points' argument refusals, the reference's crop loop restated literally, and folder builders.

A plain module: no fixtures, nothing that needs a GPU at import."""
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

GUARD = 64
SENT_F, SENT_I = -12345.0, -7


# ---------------------------------------------------------------------------------------------------- kernel A
def table():
    from dc_vic_amd.train.data import conversion_table
    return conversion_table()


def u8_case(N, H, W, seed):
    """uint8 [N, H, W, 3] whose values include 0 and 255."""
    a = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    a.view(-1)[0], a.view(-1)[-1] = 0, 255
    return a


def u8_hwc_to_f32_nchw_ref(src, tab):
    """out[n, c, y, x] = tab[src[n, y, x, c]]: dcvic_u8_hwc_to_f32_nchw restated."""
    return tab[src.long()].permute(0, 3, 1, 2).contiguous()


def table_expression(src):
    """The project's expression on the same bytes (io_pipeline.u8_to_model_range): what the table stands for."""
    return ((src.permute(0, 3, 1, 2).float().div(255.0) - 0.5) / 0.5).contiguous()


# ---------------------------------------------------------------------------------------------------- kernel B
def token_case(N, h, w, n_e, seed, dtype=torch.int64):
    """Tokens [N, h, w] in [0, n_e) that include 0, n_e - 1 and repeats (where there is room for them)."""
    t = torch.randint(0, n_e, (N, h, w), generator=torch.Generator().manual_seed(seed))
    f = t.view(-1)
    if f.numel() >= 4:
        f[0], f[1], f[2], f[3] = 0, n_e - 1, n_e - 1, 0
    return t.to(dtype)


def codebook_case(n_e, D, seed):
    return torch.randn((n_e, D), generator=torch.Generator().manual_seed(seed))


def torch_chain(tokens, codebook):
    """(idx, zq, feat) as comp_model.vq_indices_to_latent and _index_feat build them: embedding, permute, one_hot, cast, cat."""
    idx = tokens.long()
    zq = F.embedding(idx, codebook).permute(0, 3, 1, 2).contiguous()
    onehot = F.one_hot(idx, codebook.shape[0]).permute(0, 3, 1, 2).to(zq.dtype)
    return idx, zq, torch.cat([zq, onehot], dim=1).contiguous()


def vq_token_feat_ref(tokens, codebook):
    """dcvic_vq_token_feat_f32 restated, with its rule for a token outside [0, n_e): never an address, NaN zq, zero one-hot row, idx
    carried through."""
    n_e, D = codebook.shape
    idx = tokens.long()
    ok = (idx >= 0) & (idx < n_e)
    safe = torch.where(ok, idx, torch.zeros_like(idx))
    zq = codebook[safe]                                                  # [N, h, w, D]
    zq = torch.where(ok.unsqueeze(-1), zq, torch.full_like(zq, float("nan"))).permute(0, 3, 1, 2).contiguous()
    onehot = (torch.arange(n_e).view(1, n_e, 1, 1) == safe.unsqueeze(1)) & ok.unsqueeze(1)
    return idx, zq, torch.cat([zq, onehot.float()], dim=1).contiguous()


# ---------------------------------------------------------------------------------------------------- refusals
FAKE = 4096                       # non-null and aligned, never dereferenced: every refusal precedes the launch


def check_refusals():
    """Every refusal of both entry points returns DCVIC_EINVAL with the entry point's name in front (host and GPU test files)."""
    from dc_vic_amd import _lib
    L = _lib.lib()

    def a(src=FAKE, N=2, H=8, W=8, tab=FAKE, out=FAKE):
        return L.dcvic_u8_hwc_to_f32_nchw(src, N, H, W, tab, out, None)

    def b(tok=FAKE, nbytes=1, cb=FAKE, N=2, h=4, w=4, D=4, n_e=256, idx=FAKE, zq=FAKE, feat=FAKE):
        return L.dcvic_vq_token_feat_f32(tok, nbytes, cb, N, h, w, D, n_e, idx, zq, feat, None)

    cases = [
        (a, dict(src=None), "null pointer"), (a, dict(tab=None), "null pointer"), (a, dict(out=None), "null pointer"),
        (a, dict(N=0), "empty batch"), (a, dict(H=0), "empty batch"), (a, dict(W=-1), "empty batch"), (a, dict(N=65536), "65535"),
        (a, dict(H=1 << 15, W=(1 << 13) + 1), "2^28"), (a, dict(out=FAKE + 2), "4-byte aligned"),
        (b, dict(tok=None), "null pointer"), (b, dict(cb=None), "null pointer"), (b, dict(idx=None, zq=None, feat=None), "no output"),
        (b, dict(N=0), "empty problem"), (b, dict(h=0), "empty problem"), (b, dict(D=0), "empty problem"), (b, dict(n_e=-3), "empty problem"),
        (b, dict(N=65536), "65535"), (b, dict(h=1 << 15, w=(1 << 13) + 1), "2^28"), (b, dict(n_e=1 << 19), "2^19"),
        (b, dict(nbytes=4), "token_bytes=4"), (b, dict(nbytes=0), "token_bytes=0"),
        (b, dict(nbytes=8, tok=FAKE + 4), "8-byte aligned"), (b, dict(idx=FAKE + 4), "8-byte aligned"),
        (b, dict(zq=FAKE + 2), "4-byte aligned"), (b, dict(feat=FAKE + 1), "4-byte aligned"), (b, dict(cb=FAKE + 2), "4-byte aligned"),
    ]
    for fn, kw, words in cases:
        assert fn(**kw) == -1, (fn.__name__, kw)
        msg = L.dcvic_last_error().decode()
        front = "u8_hwc_to_f32_nchw:" if fn is a else "vq_token_feat:"
        assert msg.startswith(front) and words in msg, (msg, words)
    return len(cases)


# ---------------------------------------------------------------------------------------------------- the crop plan
def reference_loop(paths, size_of, seed, num_img, patch=256):
    """The reference's loop, statement for statement, on the GLOBAL generators as it runs them: seed both, shuffle the sorted list
    in place, walk it, skip a small image without a draw, draw top then left."""
    random.seed(seed)
    np.random.seed(seed)
    lst = sorted(paths)
    np.random.shuffle(lst)
    out = []
    for p in lst:
        w, h = size_of[p]
        if min(w, h) < patch:
            continue
        top = random.randint(0, h - patch)
        left = random.randint(0, w - patch)
        out.append((p, top, left))
        if len(out) == num_img:
            break
    return out


# ---------------------------------------------------------------------------------------------------- the host list before the set
def list_before(root):
    """The host list and its partition as binary_rate_search formed them before SelectionSet existed, restated: what the host
    fallback (and load_dataset / batches, which now call the package) must still give."""
    from glob import glob
    from PIL import Image
    items = []
    for path in sorted(glob(os.path.join(root, "*.png"))):
        img = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
        x = (torch.from_numpy(img.copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5
        npy = path[:-4] + ".npy"
        items.append((x, torch.from_numpy(np.load(npy).astype(np.int32)).long() if os.path.exists(npy) else None))
    return items


def batches_before(items, bs):
    out, i = [], 0
    while i < len(items):
        j = i + 1
        while j < len(items) and j - i < bs and items[j][0].shape == items[i][0].shape and (items[j][1] is None) == (items[i][1] is None):
            j += 1
        out.append((torch.stack([it[0] for it in items[i:j]]), torch.stack([it[1] for it in items[i:j]]) if items[i][1] is not None else None))
        i = j
    return out


# ---------------------------------------------------------------------------------------------------- folders
def write_png(path, H, W, seed):
    from PIL import Image
    a = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    Image.fromarray(a, mode="RGB").save(path)
    return a


def make_folder(root, shapes, tokens, n_embed=256, dtype=np.uint8):
    """<i>.png of shapes[i] = (H, W), and <i>.npy of the padded token shape for every i in `tokens`."""
    from dc_vic_amd.selection_set import padded_token_shape
    os.makedirs(root, exist_ok=True)
    for i, (H, W) in enumerate(shapes):
        write_png(os.path.join(root, f"{i}.png"), H, W, 100 + i)
        if i in tokens:
            np.save(os.path.join(root, f"{i}.npy"), np.random.default_rng(200 + i).integers(0, n_embed, padded_token_shape(H, W)).astype(dtype))
    return str(root)
