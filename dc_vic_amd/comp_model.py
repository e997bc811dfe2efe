"""The DC-VIC codec model (compress / decompress / run_model) on HIP kernels.

Drop-in mirror of the reference's model classes and builders:
  src/models/__init__.py:14-32 (build_comp_model), src/models/subnet/__init__.py:18-32 (build_subnet),
  src/models/vq_vae_builder.py:10-23, src/models/subnet/vq_estimator/__init__.py (build_vq_estimator),
  src/models/comp_model/base_model.py:16-189 (BaseModel),
  src/models/comp_model/hyperprior_vic_model.py:30-534 (HyperpriorVicModel),
  src/models/comp_model/hyperprior_dc_vic_model.py:25-483 (HyperpriorDualCondVicModel),
  src/models/comp_model/hyperprior_charm_dc_vic_model.py:16-91 (HyperpriorCharmDualCondVicModel),
  src/models/comp_model/hyperprior_charm_vic_model.py:14-52 (HyperpriorCharmVicModel, the unconditioned model of stage 1-1).
Same class names / registry keys / method names / state-dict keys / bitstream; inference only.
Differences by design (MI355X-first):
  * everything, including hyper-decoder + CHARM, stays on the GPU on both sides (kernels are
    deterministic and batch-invariant, so encoder and decoder agree bit for bit); only int32
    symbols / cdf indexes and the final bytes cross PCIe;
  * `compress_batch` / `decompress_batch` code N images per call (one rANS stream per image, coded
    in parallel on host threads); `compress` / `decompress` keep the reference's one-image contract.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from copy import deepcopy
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .charm import Minnen20CharmContextModel  # noqa: F401  (registers)
from .codec_utils import HeaderHandler
from .elic import ElicDualBetaFtFeatFusionDecoder, ElicDualBetaFtVqScEncoder, ElicFeatFusionDecoder, ElicVqCatScEncoder  # noqa: F401
from .entropy import EntropyBottleneck, GaussianMeanScaleConditional, get_scale_table, host_threads
from .fusion import build_vq_fusion_module
from .hyperprior import Minnen20HyperDecoder, Minnen20HyperEncoder  # noqa: F401
from .layers import WeightFingerprint, allow_bf16, invalidate_weight_caches
from .registry import (CONTEXTMODEL_REGISTRY, DECODER_REGISTRY, ENCODER_REGISTRY, ENTROPYMODEL_REGISTRY,
                       HYPERDECODER_REGISTRY, HYPERENCODER_REGISTRY, LRP_REGISTRY, MODEL_REGISTRY, VQ_ESTIMATOR_REGISTRY)
from .swin import DualBlockSwinVqEstimator  # noqa: F401
from .vqgan import VQModelInterface

Tensor = torch.Tensor

SPLIT_DECODE_RESOLUTION = 1024   # hyperprior_vic_model.py:25-27
SPLIT_WINDOW_SIZE = 512
# Marked layers that stay fp32 in decoder precision "bf16" (the fidelity rule of the mode: >= 50 dB PSNR against the fp32 reconstruction,
# with margin for the uint8 PNG).  bf16 rounding errors compound through the decoder: every layer alone costs less than the bar, all of them
# together 44.9 dB.  These are the 16 largest contributors, measured one layer at a time (tools/bf16_layer_sensitivity.py,
# profiles/bf16_layer_sensitivity.json): the three Upsample convs, the SFT scale convs, the mid blocks and the first full-resolution block.
BF16_KEEP_FP32 = (
    "vq_model.decoder.up.3.upsample.conv",
    "vq_model.decoder.mid.block_1.conv2",
    "fusion_module.fusion_modules.block_1_4.scale.2",
    "vq_model.decoder.up.2.upsample.conv",
    "vq_model.decoder.mid.block_1.conv1",
    "vq_model.decoder.up.1.upsample.conv",
    "fusion_module.fusion_modules.block_1_4.scale.0",
    "fusion_module.fusion_modules.block_1_2.scale.2",
    "fusion_module.fusion_modules.block_1_8.scale.0",
    "fusion_module.fusion_modules.block_1_2.scale.0",
    "fusion_module.fusion_modules.block_1_8.scale.2",
    "vq_model.decoder.mid.block_2.conv2",
    "vq_model.decoder.mid.block_2.conv1",
    "vq_model.decoder.up.3.block.0.conv1",
    "vq_model.decoder.up.3.block.0.conv2",
    "vq_model.decoder.up.3.block.1.conv1",
)
SPLIT_STRIDE = 256
# tiling windows of a > 1024-px image decoded / encoded per kernel launch (the reference loops one by one): 32 x 512^2 windows
# are ~25 GB of activations at the VQGAN decoder's widest point -- nothing on a 288 GB part
TILE_BATCH = max(1, int(os.environ.get("DCVIC_TILE_BATCH", "32")))


class _GraphCache:
    """hipGraph replay of a pure-device network segment (no host sync inside): the encoder networks of `compress_batch` and the decoder
    networks of `decompress_batch` are ~640 kernel launches per 32-image batch, a third of them shorter than the ~10 us the Python /
    ctypes launcher needs per launch, so the GPU idles between them (6 ms of a 166-ms step by the rocprofv3 trace).  A segment is captured
    on torch's capture stream -- the C-ABI kernels launch on torch's current stream, so they are recorded like any other work -- and
    replayed afterwards; inputs are copied into the graph's static buffers, outputs are the graph's static tensors (valid until the next
    replay).  Same kernels, same arguments: results are bit-identical to the eager path (tested).
    Policy: a (segment, input shapes, conditioning) key is captured the SECOND time it is seen (`capture_after`; a folder of images that
    all differ in size stays eager: a capture costs two extra passes), up to `max_pixels` per call and `max_entries` graphs (LRU).
    Captures that fail (unsupported call inside the segment) fall back to the eager path for good.  An entry whose modules' weights are
    no longer the ones it was captured with is dropped, never replayed (`run`).  On by default since round 3
    (measured 193 -> 200 images/s at batch 32); `DCVIC_GRAPHS=0` switches it off.  Per-launch HIP events (bench.py's roofline steps,
    ops.kernel_events_start) and the stage hook bypass it."""

    def __init__(self, max_entries: int = 4):
        self.entries: "OrderedDict" = OrderedDict()
        self.seen: Dict = {}
        self.max_entries = int(os.environ.get("DCVIC_GRAPH_MAX_ENTRIES", str(max_entries)))
        self.disabled = os.environ.get("DCVIC_GRAPHS", "1") == "0"
        self.max_pixels = int(os.environ.get("DCVIC_GRAPH_MAX_PIXELS", str(4 << 20)))      # 32 x 256^2 = 2.1 M, 8 x 512x768 = 3.1 M
        self.capture_after = max(1, int(os.environ.get("DCVIC_GRAPH_CAPTURE_AFTER", "2")))

    def clear(self):
        self.entries.clear()
        self.seen.clear()

    def usable(self, n_pixels: int) -> bool:
        return (not self.disabled) and n_pixels <= self.max_pixels and ops._EVENTS is None and STAGE_HOOK is None

    def run(self, key, fn, inputs: Sequence[Tensor], keep=None, modules: Sequence[nn.Module] = ()):
        """`modules`: the modules `fn` runs.  The captured graph holds raw pointers to their packed weights (and to the parameters
        themselves) of that moment, and nothing per layer runs during a replay, so the entry carries the fingerprint of their
        parameters and buffers (layers.WeightFingerprint) and is replayed only while it still matches; otherwise it is dropped and the
        key starts again at its first sighting (eager, which re-packs the layers, then capture)."""
        ent = self.entries.get(key)
        if ent is not None and ent[4]() != ent[5]:
            del self.entries[key]
            self.seen.pop(key, None)
            ent = None
        if ent is None:
            n = self.seen.get(key, 0) + 1
            if len(self.seen) > 256:
                self.seen.clear()
            self.seen[key] = n
            if n < self.capture_after:
                return fn(*inputs)                     # first sighting of this shape: eager
            static_in = [torch.empty_like(t) for t in inputs]
            for s_, t in zip(static_in, inputs):
                s_.copy_(t)
            try:
                if n == 1:
                    # capture at first sight (capture_after = 1): a warm-up pass for the lazy weight packs, function attributes and
                    # caches.  From the second sighting on the eager pass(es) already did that: the capture itself executes nothing,
                    # so capturing costs one launcher pass (~10 ms of host time), not a network pass
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        fn(*static_in)
                    torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                # thread_local: only THIS thread's calls are policed during the capture -- under torch.distributed the RCCL watchdog
                # thread polls events at any time, which the default (global) mode would turn into a failed capture
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    out = fn(*static_in)
            except Exception as e:                     # noqa: BLE001 -- any capture failure means "stay eager"
                self.disabled = True
                torch.cuda.synchronize()
                import sys
                print(f"[dc_vic_amd] hipGraph capture disabled: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
                if os.environ.get("DCVIC_GRAPH_DEBUG"):
                    import traceback
                    traceback.print_exc()
                return fn(*inputs)
            watch = WeightFingerprint(modules)
            ent = (graph, static_in, out, keep() if callable(keep) else keep, watch, watch())
            self.entries[key] = ent
            while len(self.entries) > self.max_entries:
                self.entries.popitem(last=False)
        else:
            self.entries.move_to_end(key)
        graph, static_in, out = ent[:3]
        for s_, t in zip(static_in, inputs):
            s_.copy_(t)
        graph.replay()
        return out


STAGE_HOOK = None     # diagnostic: callable(name) invoked at stage boundaries of compress_batch / decompress_batch


def _mark(name: str) -> None:
    if STAGE_HOOK is not None:
        STAGE_HOOK(name)


def _get(opt, key, default=None):
    try:
        return opt[key]
    except (KeyError, TypeError):
        return default


def build_subnet(subnet_opt: Dict, subnet_type: str):
    subnet_opt = deepcopy(dict(subnet_opt))
    network_type = subnet_opt.pop("type")
    registry = {
        "encoder": ENCODER_REGISTRY, "decoder": DECODER_REGISTRY, "hyperencoder": HYPERENCODER_REGISTRY,
        "hyperdecoder": HYPERDECODER_REGISTRY, "context_model": CONTEXTMODEL_REGISTRY,
        "entropy_model": ENTROPYMODEL_REGISTRY, "residual_predictor": LRP_REGISTRY,
    }[subnet_type]
    return registry.get(network_type)(**subnet_opt)


def build_vq_estimator(opt: Dict):
    opt = deepcopy(dict(opt))
    return VQ_ESTIMATOR_REGISTRY.get(opt.pop("type"))(**opt)


def build_pretrained_vq_model(vq_model_opt: Dict, device) -> VQModelInterface:
    opt = deepcopy(dict(vq_model_opt))
    ckpt_path = opt.pop("ckpt_path", None)
    if hasattr(opt.get("ddconfig"), "to_dict"):
        opt["ddconfig"] = opt["ddconfig"].to_dict()
    model = VQModelInterface(**opt)
    if ckpt_path:
        if not os.path.exists(ckpt_path):
            raise FileNotFoundError(f"VQGAN checkpoint {ckpt_path} not found (set subnet.vq_model.ckpt_path, or null to skip)")
        sd = torch.load(ckpt_path, map_location="cpu", weights_only=True)["state_dict"]
        sd = {k: v for k, v in sd.items() if not k.startswith("loss.")}
        model.load_state_dict(sd)
    return model.to(device)


def build_comp_model(opt):
    opt = deepcopy(opt)
    if _get(opt, "model"):
        model_opt = deepcopy(dict(opt["model"]))
        model_type = model_opt.pop("type")
        return MODEL_REGISTRY.get(model_type)(opt, **model_opt)
    raise ValueError('"model_type" key is not supported. Please use trainer.type')


def build_trained_comp_model(opt, ckpt_path: str):
    model = build_comp_model(opt)
    model.load_learned_weight(ckpt_path=ckpt_path)
    return model


def _starts(size: int, stride: int, patch: int, pre_div: bool) -> List[int]:
    """Window starts of the tiling branches (hyperprior_vic_model.py:197-213 / 420-436)."""
    if size < patch:
        # the reference loop would emit a negative start here (size - patch) and slice a wrapped, narrower window
        raise ValueError(f"tiling (max(H, W) > {SPLIT_DECODE_RESOLUTION}) needs both padded sides >= {SPLIT_WINDOW_SIZE} px; "
                         f"got a side of {size * (SPLIT_WINDOW_SIZE // patch)} px")
    out = []
    rng = range(size // stride + 1) if pre_div else range(0, size, stride)
    for i in rng:
        s = i * stride if pre_div else i
        if s + patch < size:
            out.append(s)
        else:
            out.append(size - patch)
            break
    return out


class BaseModel(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.device = _get(opt, "device", "cuda:0")
        if str(self.device) == "cuda" and torch.cuda.is_available():
            self.device = f"cuda:{torch.cuda.current_device()}"          # the reference's `-d cuda`: the current device
        if str(self.device).startswith("cuda") and torch.cuda.is_available():
            # the C-ABI kernels launch on the current device's current stream (`-d cuda:1` must make cuda:1 current)
            torch.cuda.set_device(torch.device(self.device))
        self.convert_img_range = bool(_get(opt, "convert_img_range_to_01", False))
        if self.convert_img_range:
            raise NotImplementedError("convert_img_range_to_01 is not used by the DC-VIC configs")
        self._build_subnets()
        self.stride = 64
        self._graphs = _GraphCache()

    def _build_subnets(self):
        raise NotImplementedError()

    # base_model.py:35-43
    def img_preprocess(self, real_images: Tensor, is_train: bool = True) -> Tensor:
        if is_train:
            raise NotImplementedError("dc_vic_amd implements the inference path only")
        out = real_images.to(self.device, dtype=torch.float32).contiguous()
        return self.pad_images(out)

    # base_model.py:45-57
    def img_postprocess(self, *images: Tensor, size: Tuple[int, int], is_train: bool):
        H, W = size
        out = [ops.crop_clamp(img, H, W) for img in images]
        return out[0] if len(out) == 1 else tuple(out)

    def pad_images(self, *images: Tensor):
        out = [self._pad_image(img, self.stride) for img in images]
        return out[0] if len(out) == 1 else tuple(out)

    @staticmethod
    def _pad_image(x: Tensor, stride: int, mode: str = "reflect") -> Tensor:
        _, _, H, W = x.shape
        padW = int(np.ceil(W / stride) * stride - W)
        padH = int(np.ceil(H / stride) * stride - H)
        if padH == 0 and padW == 0:
            return x
        return ops.pad_reflect(x, padH, padW)

    @staticmethod
    def _crop_image(x: Tensor, H: int, W: int) -> Tensor:
        return ops.crop(x, H, W)

    def crop_images(self, *images: Tensor, size: Tuple[int, int]):
        H, W = size
        out = [self._crop_image(i, H, W) for i in images]
        return out[0] if len(out) == 1 else tuple(out)

    def load_state_dict(self, state_dict, strict: bool = True):
        out = super().load_state_dict(state_dict, strict=strict)
        self.invalidate_weight_caches()
        return out

    def invalidate_weight_caches(self) -> None:
        """Drop every copy of the weights the model keeps: packed plans, fused packs, cached beta vectors, captured hipGraphs
        (layers.invalidate_weight_caches).  Weight changes torch versions (load_state_dict on the model or a child, in-place ops on a
        parameter, a replaced parameter) are detected without it; a `p.data` or raw-pointer write is not -- call this after one."""
        invalidate_weight_caches(self)

    # base_model.py:106-130
    def load_learned_weight(self, ckpt_path: str, strict: bool = False) -> Dict[str, List[str]]:
        """-> dict(loaded, missing, unexpected): the keys of the checkpoint that were loaded, the model's keys it lacks (they keep the
        values they have) and its keys the model lacks (dropped); with strict both must be empty."""
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        state_dict = ckpt["comp_model"]
        new_sd = OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state_dict.items())
        model_dict = self.state_dict()
        report = dict(loaded=[k for k in new_sd if k in model_dict], missing=[k for k in model_dict if k not in new_sd],
                      unexpected=[k for k in new_sd if k not in model_dict])
        if not strict:
            model_dict.update({k: v for k, v in new_sd.items() if k in model_dict})
            self.load_state_dict(model_dict)
        else:
            self.load_state_dict(new_sd)
        for m in self.children():
            if isinstance(m, EntropyBottleneck):
                m.update(force=False)
        return report

    def codec_setup(self):
        raise NotImplementedError()


@MODEL_REGISTRY.register()
class HyperpriorVicModel(BaseModel):
    def __init__(self, opt, gumbel_sampling: bool = False, gumbel_kwargs: Dict = {}, enc_vq_input: str = "norm_indices",
                 enc_input_vq_recon: bool = False) -> None:
        super().__init__(opt)
        assert enc_vq_input in ["norm_indices", "onehot_indices", "long_indices"]
        if enc_vq_input != "onehot_indices" or enc_input_vq_recon:
            raise NotImplementedError("only enc_vq_input='onehot_indices' (the shipped configs) is built")
        self.enc_vq_input = enc_vq_input
        # training mode only (hyperprior_vic_model.py:393-406): read by the GAN-stage trainers, never by an inference path
        self.gumbel_sampling, self.gumbel_kwargs = bool(gumbel_sampling), dict(gumbel_kwargs or {})
        self.n_embed = self.vq_model.n_embed
        self.model_stride, self.y_stride = 64, 16
        self._decoder_precision = "fp32"
        self.to(self.device)

    DECODER_PRECISIONS = ("fp32", "bf16")

    @property
    def decoder_precision(self) -> str:
        """"fp32" (default) or "bf16": the arithmetic of the VQGAN decoder's and the SFT fusion blocks' 3x3 convolutions."""
        return self._decoder_precision

    def set_decoder_precision(self, precision: str) -> None:
        """"bf16" runs the 3x3 convolutions of the frozen VQGAN decoder and of the SFT fusion blocks (the layers after the estimator's
        argmax, layers.allow_bf16) on the bf16-MFMA kernel; "fp32" restores the default kernels bit for bit.  Bitstreams, VQ indices,
        symbols, latents and the estimator's logits do not depend on it, only the reconstruction does (>= 50 dB PSNR against fp32).
        Honoured by run_model, decompress_batch / decompress and decode_split; hipGraph segments are keyed by it."""
        if precision not in self.DECODER_PRECISIONS:
            raise ValueError(f"decoder precision must be one of {self.DECODER_PRECISIONS}, got {precision!r}")
        on = precision == "bf16"
        allow_bf16(self.vq_model.decoder, on)
        allow_bf16(self.fusion_module, on)
        mods = dict(self.named_modules())
        for name in BF16_KEEP_FP32:
            if name in mods:
                mods[name].bf16_keep_fp32 = on
        self._decoder_precision = precision

    def _build_subnets(self) -> None:
        sub = self.opt["subnet"]
        self.encoder = build_subnet(sub["encoder"], "encoder")
        self.decoder = build_subnet(sub["decoder"], "decoder")
        self.hyperencoder = build_subnet(sub["hyperencoder"], "hyperencoder")
        self.hyperdecoder = build_subnet(sub["hyperdecoder"], "hyperdecoder")
        self.entropy_model_z = build_subnet(sub["entropy_model_z"], "entropy_model")
        self.entropy_model_y = build_subnet(sub["entropy_model_y"], "entropy_model")
        self.vq_estimator = build_vq_estimator(sub["vq_estimator"])
        self.vq_model = build_pretrained_vq_model(sub["vq_model"], device=self.device)
        self.vq_model.quantize.sane_index_shape = True
        self.fusion_module = build_vq_fusion_module(sub["fusion_module"])

    # hyperprior_vic_model.py:80-82
    def likelihood_to_bit(self, likelihood: Tensor, num_pixel: int):
        """(bitcost, bitcost / num_pixel) over the whole tensor, as 0-dim tensors like the reference."""
        bits = ops.neglog2_sum(likelihood).double().sum()
        return bits, bits / num_pixel

    # hyperprior_vic_model.py:66-78
    def get_rate_summary_dict(self, out_dict: Dict, num_pixel: int) -> Dict[str, Tensor]:
        lk, qlk = out_dict["likelihoods"], out_dict["q_likelihoods"]
        _, y_bpp = self.likelihood_to_bit(lk["y"], num_pixel)
        _, z_bpp = self.likelihood_to_bit(lk["z"], num_pixel)
        if qlk["y"] is lk["y"] and qlk["z"] is lk["z"]:
            yq_bpp, zq_bpp = y_bpp, z_bpp          # eval mode: both likelihoods are the quantised one
        else:
            _, yq_bpp = self.likelihood_to_bit(qlk["y"], num_pixel)
            _, zq_bpp = self.likelihood_to_bit(qlk["z"], num_pixel)
        return dict(y_likelihood=lk["y"], z_likelihood=lk["z"], bpp=y_bpp + z_bpp, y_q_likelihood=qlk["y"],
                    z_q_likelihood=qlk["z"], qbpp=yq_bpp + zq_bpp)

    # ------------------------------------------------------------------ VQ encode (137-246)
    def _vq_encode_split(self, real_images: Tensor) -> Tensor:
        """hyperprior_vic_model.py:190-246: 512-px windows, stride 256, centre regions stitched.  The reference encodes the windows
        one by one; here up to TILE_BATCH of them are stacked into ONE encoder call (the windows are independent and every kernel
        is batch-invariant, so the stitched latent is bit-identical to the window-by-window loop -- asserted in test_tiling_vs_oracle):
        a 1280x2048 image is one 28-window batch in the batch-32 regime instead of 28 launches in the N=1 regime."""
        N, _, H, W = real_images.shape
        stride, patch = SPLIT_STRIDE, SPLIT_WINDOW_SIZE
        df = 2 ** (self.vq_model.encoder.num_resolutions - 1)
        ndim = self.vq_model.embed_dim
        lefts = _starts(W, stride, patch, True)
        tops = _starts(H, stride, patch, True)
        z_out = torch.zeros((N, ndim, H // df, W // df), dtype=torch.float32, device=real_images.device)
        wins = [(y0, x0) for y0 in tops for x0 in lefts]
        per = max(1, TILE_BATCH // N)
        for c0 in range(0, len(wins), per):
            chunk = wins[c0:c0 + per]
            crop = torch.empty((N * len(chunk), real_images.shape[1], patch, patch), dtype=torch.float32, device=real_images.device)
            for k, (y0, x0) in enumerate(chunk):
                ops.copy_window(crop[k * N:(k + 1) * N], real_images[:, :, y0:y0 + patch, x0:x0 + patch])
            zb = self.vq_model.encode(crop)
            for k, (y0, x0) in enumerate(chunk):
                z = zb[k * N:(k + 1) * N]
                off = (stride // 2) // df
                _x0, _y0 = x0 // df, y0 // df
                l = _x0 + off if x0 > 0 else 0
                t = _y0 + off if y0 > 0 else 0
                r = _x0 + off + stride // df if x0 < lefts[-1] else W // df
                b = _y0 + off + stride // df if y0 < tops[-1] else H // df
                ops.copy_window(z_out[:, :, t:b, l:r], z[:, :, t - _y0:b - _y0, l - _x0:r - _x0])
        return z_out

    def vq_encode(self, real_images: Tensor, vq_indices: Optional[Tensor] = None, want_feat: bool = False):
        """Returns (gt_vq_latent, gt_vq_indices[, feat = cat[latent, onehot]])."""
        if vq_indices is not None:
            # pre-computed tokens (scripts/build_openimage_val_dataset.py -> binary_rate_search / beta_selection callers)
            # uint8 / int64 tokens on the device go to the kernel as they are; anything else becomes int64 on the device first.  One
            # launch writes idx, zq and feat with the bits of vq_indices_to_latent and _index_feat (csrc/tokens.hip)
            tok = vq_indices
            if not (tok.device == real_images.device and tok.dtype in (torch.uint8, torch.int64)):
                tok = tok.to(real_images.device).long()
            given = tok.dtype == torch.int64       # .long() of an int64 tensor is that tensor: return it, as before
            idx, zq, feat = ops.vq_token_feat(tok.contiguous(), self.vq_model.quantize.embedding.weight, want_idx=not given, want_feat=want_feat)
            idx = tok if given else idx
            if want_feat:
                return zq, idx, feat
            return zq, idx
        N, _, H, W = real_images.shape
        _z = self._vq_encode_split(real_images) if max(H, W) > SPLIT_DECODE_RESOLUTION else self.vq_model.encode(real_images)
        # n_embed > 1024 (hyperprior_vic_model.py:149-150 `_vq_quantize_split`, which chunks the latent to bound the [HW, n_e]
        # distance matrix): the sharded-codebook kernel streams the codebook through LDS instead, any size in one launch
        r = self.vq_model.quantize(_z, want_feat=want_feat)
        if want_feat:
            zq, _, (_, _, idx), feat = r
            return zq, idx, feat
        zq, _, (_, _, idx) = r
        return zq, idx

    def _index_feat(self, latent: Tensor, indices: Tensor) -> Tensor:
        """cat[latent, one_hot(indices)] from the indices GIVEN (hyperprior_vic_model.py:268-271), not from a search of the gathered
        latent: the search returns the first of two equal codebook rows, whatever index the caller holds.  The torch form, for callers
        that hold a latent already; vq_encode with tokens gets the same bits from dcvic_vq_token_feat_f32."""
        n_e = self.vq_model.quantize.embedding.weight.shape[0]
        onehot = torch.nn.functional.one_hot(indices.long(), n_e).permute(0, 3, 1, 2).to(latent.dtype)
        return torch.cat([latent, onehot], dim=1).contiguous()

    def vq_indices_to_latent(self, indices: Tensor) -> Tensor:
        e = self.vq_model.quantize.embedding(indices)          # [N, H, W, D]
        return e.permute(0, 3, 1, 2).contiguous()

    # ------------------------------------------------------------------ encoder (248-290)
    def comp_encode(self, real_images: Tensor, gt_vq_latent: Tensor, gt_vq_indices: Tensor, enc_kwargs: Dict = {},
                    feat: Optional[Tensor] = None) -> Tensor:
        if feat is None:
            feat = self._index_feat(gt_vq_latent, gt_vq_indices.to(gt_vq_latent.device))
        return self.encoder(real_images, feat, **enc_kwargs)

    # ------------------------------------------------------------------ decode (276-288, 413-473)
    def _decode(self, y_hat: Tensor, w: float, beta_rate, beta_vq, want_logits: bool = False, want_embed: bool = False):
        """-> (img, idx), + logits with want_logits, + the estimator's predicted embedding (out_vq_latent) with want_embed."""
        N, _, yH, yW = y_hat.shape
        cat_bufs = self.fusion_module.alloc_cat_buffers(N, 2 * yH, 2 * yW, y_hat.device)
        feat_out = {k: cat_bufs[k][:, : self.fusion_module.fusion_modules[k].cond_ch] for k in cat_bufs}
        feat_1, _ = self.decoder.get_feats(y_hat, beta_1=beta_rate, beta_2=beta_vq, feat_out=feat_out)
        embed, logits = self.vq_estimator(feat_1, want_embed=want_embed)
        pq = self.vq_model.post_quant_conv
        idx, lat = ops.argmax_lut(logits, self.vq_model.quantize.embedding.weight, pq.weight.reshape(pq.out_channels, -1).contiguous(), pq.bias)
        img = self.fusion_module(lat, None, self.vq_model.decoder, w=w, cat_bufs=cat_bufs)
        return (img, idx) + ((logits,) if want_logits else ()) + ((embed,) if want_embed else ())

    def decode_split(self, y_hat: Tensor, fuse_w: float, **kwargs) -> Tensor:
        """hyperprior_vic_model.py:413-473: 32x32-latent windows (512 px), stride 16, centre regions stitched into a buffer pre-filled
        with -100.  Windows are decoded as batches of up to TILE_BATCH (see _vq_encode_split): same bits, batch-32 regime."""
        N, _, yH, yW = y_hat.shape
        df = 16
        stride, patch = SPLIT_STRIDE // df, SPLIT_WINDOW_SIZE // df
        lefts = _starts(yW, stride, patch, False)
        tops = _starts(yH, stride, patch, False)
        out = torch.full((N, 3, yH * df, yW * df), -100.0, dtype=torch.float32, device=y_hat.device)
        wins = [(y0, x0) for y0 in tops for x0 in lefts]
        per = max(1, TILE_BATCH // N)
        for c0 in range(0, len(wins), per):
            chunk = wins[c0:c0 + per]
            crop = torch.empty((N * len(chunk), y_hat.shape[1], patch, patch), dtype=torch.float32, device=y_hat.device)
            for k, (y0, x0) in enumerate(chunk):
                ops.copy_window(crop[k * N:(k + 1) * N], y_hat[:, :, y0:y0 + patch, x0:x0 + patch])
            ob, _ = self._decode(crop, w=fuse_w, **kwargs)
            for k, (y0, x0) in enumerate(chunk):
                o = ob[k * N:(k + 1) * N]
                off = (stride // 2) * df
                _x0, _y0 = x0 * df, y0 * df
                l = _x0 + off if x0 > 0 else 0
                t = _y0 + off if y0 > 0 else 0
                r = _x0 + off + stride * df if x0 < lefts[-1] else yW * df
                b = _y0 + off + stride * df if y0 < tops[-1] else yH * df
                ops.copy_window(out[:, :, t:b, l:r], o[:, :, t - _y0:b - _y0, l - _x0:r - _x0])
        return out

    # ------------------------------------------------------------------ entropy stage
    def _entropy_encode_side(self, y: Tensor, want_symbols: bool):
        """hyper-encoder -> z symbols / z_hat / z bits -> hyper-decoder -> CHARM (all on the GPU)."""
        N = y.shape[0]
        z = self.hyperencoder(y)
        bits_z = torch.zeros(N, dtype=torch.float32, device=y.device)
        bits_y = torch.zeros(N, dtype=torch.float32, device=y.device)
        z_hat = torch.empty_like(z)
        z_lik = torch.empty_like(z)
        z_sym = torch.empty(z.shape, dtype=torch.int32, device=y.device) if want_symbols else None
        ops.eb_rate(z, self.entropy_model_z.packs(), z_hat, z_sym, z_lik, bits_z)
        hyper_out = self.hyperdecoder(z_hat)
        r = self._run_context(y, hyper_out, want_symbols, bits_y)
        return dict(z=z, z_hat=z_hat, z_likelihood=z_lik, z_symbols=z_sym, bits_z=bits_z, bits_y=bits_y, hyper_out=hyper_out, **r)

    def _run_context(self, y, hyper_out, want_symbols, bits_y):
        raise NotImplementedError("only the CHARM variants (HyperpriorCharmVicModel, HyperpriorCharmDualCondVicModel) are shipped")

    def codec_setup(self):
        """hyperprior_dc_vic_model.py:65-89: build the integer CDF tables; strides are properties of the
        architecture (4 stride-2 encoder stages -> y_stride 16, 2 more in the hyper-encoder -> 64)."""
        self.entropy_model_z.update(force=True)
        self.entropy_model_y.update_scale_table(get_scale_table(), force=True)
        self.yC = self.encoder.conv4.out_channels
        self.zC = self.hyperencoder.conv3.out_channels
        self.y_stride = 2 ** self.encoder.num_downscale
        self.model_stride = self.y_stride * 2 ** self.hyperencoder.n_downsampling_layers


@MODEL_REGISTRY.register()
class HyperpriorDualCondVicModel(HyperpriorVicModel):
    def __init__(self, opt, gumbel_sampling: bool = False, gumbel_kwargs: Dict = {}, enc_vq_input: str = "norm_indices",
                 enc_input_vq_recon: bool = False, num_beta_levels: int = 100, use_selected_beta_pairs: bool = False,
                 selected_beta_rate: Optional[List[float]] = None, selected_beta_vq: Optional[List[float]] = None) -> None:
        super().__init__(opt, gumbel_sampling=gumbel_sampling, gumbel_kwargs=gumbel_kwargs, enc_vq_input=enc_vq_input,
                         enc_input_vq_recon=enc_input_vq_recon)
        self.max_beta_rate = float(opt["subnet"]["decoder"]["max_beta_1"])
        self.max_beta_vq = float(opt["subnet"]["decoder"]["max_beta_2"])
        self.num_beta_levels = num_beta_levels
        self.use_selected_beta_pairs = use_selected_beta_pairs
        self.selected_beta_rate = list(selected_beta_rate) if selected_beta_rate is not None else None
        self.selected_beta_vq = list(selected_beta_vq) if selected_beta_vq is not None else None
        if self.use_selected_beta_pairs:
            assert isinstance(self.selected_beta_rate, list) and isinstance(self.selected_beta_vq, list)
            assert len(self.selected_beta_rate) == len(self.selected_beta_vq)

    # hyperprior_dc_vic_model.py:120-170 (inference branch: betas must be given)
    def data_preprocess(self, real_images: Tensor, vq_indices: Optional[Tensor] = None, beta_rate=None, beta_vq=None,
                        is_train: bool = True, fix_entropy_models: bool = False, fusion_w: Optional[float] = None,
                        sample_batch_beta: bool = False) -> dict:
        if is_train:
            raise NotImplementedError("dc_vic_amd implements the inference path only")
        if beta_rate is None or beta_vq is None:
            raise ValueError('"beta_rate" and "beta_vq" must be specified if is_train=False')
        real_images = self.img_preprocess(real_images, is_train=False)
        if vq_indices is not None:
            vq_indices = vq_indices.to(self.device)
        return dict(real_images=real_images, beta_rate=beta_rate, beta_vq=beta_vq, vq_indices=vq_indices,
                    fix_entropy_models=fix_entropy_models, fusion_w=fusion_w)

    # ------------------------------------------------------------------ run_model (112-118, 208-274)
    @torch.no_grad()
    def run_model(self, real_images: Tensor, is_train: bool = False, beta_rate=None, beta_vq=None, vq_indices=None,
                  fusion_w: Optional[float] = None, **unused) -> Dict:
        if is_train:
            raise NotImplementedError("dc_vic_amd implements the inference path only")
        if beta_rate is None or beta_vq is None:
            raise ValueError('"beta_rate" and "beta_vq" must be specified if is_train=False')
        N, _, H, W = real_images.shape
        x = self.img_preprocess(real_images, is_train=False)
        gt_vq_latent, gt_vq_indices, feat = self.vq_encode(x, vq_indices, want_feat=True)
        y = self.comp_encode(x, gt_vq_latent, gt_vq_indices, enc_kwargs=dict(beta_1=beta_rate, beta_2=beta_vq), feat=feat)
        e = self._entropy_encode_side(y, want_symbols=False)
        y_hat = e["y_hat"]
        w = 1.0
        if max(x.shape[2:]) > SPLIT_DECODE_RESOLUTION:
            fake = self.decode_split(y_hat, w, beta_rate=beta_rate, beta_vq=beta_vq)
            out_idx = torch.zeros_like(gt_vq_indices)
            logits = embed = None
            vq_acc = 0.0
        else:
            fake, out_idx, logits, embed = self._decode(y_hat, w, beta_rate, beta_vq, want_logits=True, want_embed=True)
            vq_acc = float((out_idx.cpu() == gt_vq_indices.cpu()).float().mean())
        num_pixel = N * H * W
        bits = (e["bits_y"].double().sum() + e["bits_z"].double().sum()).item()
        bpp = bits / num_pixel
        fake_c = ops.crop_clamp(fake, H, W)
        real_c = ops.crop_clamp(x, H, W)
        return dict(real_images=real_c, fake_images=fake_c, y_hat=y_hat, z_hat=e["z_hat"], bpp=bpp, qbpp=bpp,
                    y_likelihood=e["y_likelihood"], z_likelihood=e["z_likelihood"], y_q_likelihood=e["y_likelihood"],
                    z_q_likelihood=e["z_likelihood"], gt_vq_latent=gt_vq_latent, gt_vq_indices=gt_vq_indices,
                    out_vq_indices=out_idx, out_vq_logits=logits, out_vq_latent=embed, vq_accuracy=vq_acc, beta_rate=beta_rate, beta_vq=beta_vq,
                    bits_per_image=(e["bits_y"] + e["bits_z"]))

    # ------------------------------------------------------------------ validation (442-480)
    @torch.no_grad()
    def validation(self, images: Sequence[Tensor], max_sample_size: int = 100, beta_rate: Optional[float] = None,
                   beta_vq: Optional[float] = None) -> List[Dict]:
        """One row {idx, bpp, psnr, ms_ssim, vq_acc, vq_mse} per image of `images` (host or device [1, 3, H, W] in [-1, 1], at most
        max_sample_size, one at a time as the reference's batch-1 loader): bpp and vq_acc are run_model's, psnr and ms_ssim those of
        metrics.ms_ssim_psnr on its cropped real / fake images, vq_mse the mean squared error of out_vq_latent against gt_vq_latent.
        Images with a side over SPLIT_DECODE_RESOLUTION are refused: the tiled decoder does not produce out_vq_latent."""
        from . import metrics
        from .train import kernels as K
        beta_rate = float(beta_rate) if beta_rate is not None else self.max_beta_rate / 2.0
        beta_vq = float(beta_vq) if beta_vq is not None else self.max_beta_vq / 2.0
        rows = []
        for idx, x in enumerate(list(images)[:max_sample_size]):
            if x.dim() != 4 or x.shape[0] != 1:
                raise ValueError(f"validation: image {idx} has shape {tuple(x.shape)}, expected [1, 3, H, W]")
            if max(x.shape[2:]) > SPLIT_DECODE_RESOLUTION:
                raise ValueError(f"validation: image {idx} is {x.shape[3]} x {x.shape[2]}; sides over {SPLIT_DECODE_RESOLUTION} decode "
                                 "tiled, without the out_vq_latent that vq_mse needs")
            out = self.run_model(x, is_train=False, beta_rate=beta_rate, beta_vq=beta_vq)
            ms, psnr = metrics.ms_ssim_psnr(out["real_images"], out["fake_images"])
            emb, gt = out["out_vq_latent"], out["gt_vq_latent"].contiguous()
            vq_mse = K.reduce_loss(K.SUM_SQ_ERR, emb, gt, 1.0 / emb.numel())
            rows.append(dict(idx=idx + 1, bpp=float(out["bpp"]), psnr=float(psnr[0]), ms_ssim=float(ms[0]), vq_acc=float(out["vq_accuracy"]),
                             vq_mse=float(vq_mse[0])))
        return rows

    def _segment_modules(self, segment: str) -> Tuple[nn.Module, ...]:
        """The modules whose weights the hipGraph segment "enc" (compress_batch) / "dec" (decompress_batch) reads."""
        vq = self.vq_model
        if segment == "enc":
            return (vq.encoder, vq.quant_conv, vq.quantize, self.encoder)
        return (self.decoder, self.vq_estimator, vq.quantize, vq.post_quant_conv, self.fusion_module, vq.decoder)

    # ------------------------------------------------------------------ compress (330-376)
    @torch.no_grad()
    def compress_batch(self, real_images: Tensor, quality_ind: int) -> Dict:
        """N images of one size -> N bitstreams (`string_lists[i] = [header, z_str, y_str]`)."""
        beta_rate = self.selected_beta_rate[quality_ind]
        beta_vq = self.selected_beta_vq[quality_ind]
        N, _, H, W = real_images.shape
        _mark("begin")
        if self._graphs.usable(N * H * W) and max(H, W) <= SPLIT_DECODE_RESOLUTION:
            # small batch: the encoder networks as one replayed hipGraph (launch-bound otherwise)
            def seg(xi):
                x_ = self.img_preprocess(xi, is_train=False)
                lat_, idx_, feat_ = self.vq_encode(x_, None, want_feat=True)
                y_ = self.comp_encode(x_, lat_, idx_, enc_kwargs=dict(beta_1=beta_rate, beta_2=beta_vq), feat=feat_)
                return idx_, y_
            gt_vq_indices, y = self._graphs.run(("enc", tuple(real_images.shape), quality_ind, float(beta_rate), float(beta_vq)), seg,
                                                [real_images.to(self.device, dtype=torch.float32).contiguous()],
                                                keep=lambda: list(self.encoder._vec_cache.values()),
                                                modules=self._segment_modules("enc"))
            gt_vq_indices, y = gt_vq_indices.clone(), y.clone()
        else:
            x = self.img_preprocess(real_images, is_train=False)
            _mark("preproc")
            gt_vq_latent, gt_vq_indices, feat = self.vq_encode(x, None, want_feat=True)
            _mark("encode_nn_vqgan_vq")
            y = self.comp_encode(x, gt_vq_latent, gt_vq_indices, enc_kwargs=dict(beta_1=beta_rate, beta_2=beta_vq), feat=feat)
            _mark("encode_nn_elic")
        e = self._entropy_encode_side(y, want_symbols=True)
        y_hat = e["y_hat"]
        maxabs = ops.absmax(y_hat)
        _mark("entropy_model_gpu")
        thr = host_threads()
        # one D2H per array; the rANS streams are independent -> host threads
        z_sym = e["z_symbols"].reshape(N, -1).cpu().numpy()
        y_sym = e["symbols"].reshape(N, -1).cpu().numpy()
        y_idx = e["indexes"].reshape(N, -1).cpu().numpy()
        maxabs_h = maxabs.cpu().numpy()
        bits_y = e["bits_y"].cpu().numpy().astype(np.float64)
        bits_z = e["bits_z"].cpu().numpy().astype(np.float64)
        zC, zH, zW = e["z"].shape[1:]
        _mark("symbols_d2h")
        z_strs = self.entropy_model_z.tables().encode(z_sym, self.entropy_model_z._channel_indexes(N, zH * zW), threads=thr)
        y_strs = self.entropy_model_y.tables().encode(y_sym, y_idx, threads=thr)
        hh = HeaderHandler()
        string_lists = [[hh.encode((H, W), float(maxabs_h[i]), quality_ind), z_strs[i], y_strs[i]] for i in range(N)]
        _mark("rans_encode_cpu")
        return dict(string_lists=string_lists, z_hat=e["z_hat"], y_hat=y_hat, z_likelihood=e["z_likelihood"],
                    y_likelihood=e["y_likelihood"], vq_indices=gt_vq_indices, y=y, z=e["z"], y_symbols=e["symbols"],
                    y_indexes=e["indexes"], z_symbols=e["z_symbols"], mu=e["mu"], sigma=e["sigma"],
                    pred_y_bit=bits_y, pred_z_bit=bits_z, pred_y_bpp=bits_y / (H * W), pred_z_bpp=bits_z / (H * W))

    @torch.no_grad()
    def compress(self, real_images: Tensor, quality_ind: Optional[int], vq_indices=None) -> Dict:
        N = real_images.shape[0]
        assert N == 1, f"In compress mode, batch_size must be 1, but {N}"
        r = self.compress_batch(real_images, quality_ind)
        return {
            "string_list": r["string_lists"][0], "z_hat": r["z_hat"], "y_hat": r["y_hat"],
            "z_likelihood": r["z_likelihood"], "y_likelihood": r["y_likelihood"],
            "pred_y_bit": float(r["pred_y_bit"][0]), "pred_y_bpp": float(r["pred_y_bpp"][0]),
            "pred_z_bit": float(r["pred_z_bit"][0]), "pred_z_bpp": float(r["pred_z_bpp"][0]),
            "vq_indices": r["vq_indices"], "y_symbols": r["y_symbols"], "y_indexes": r["y_indexes"], "z_symbols": r["z_symbols"],
            "y": r["y"], "z": r["z"], "mu": r["mu"], "sigma": r["sigma"],
        }

    # ------------------------------------------------------------------ decompress (389-440)
    def _decompress_entropy(self, z_strs: Sequence[bytes], y_strs: Sequence[bytes], zH: int, zW: int):
        raise NotImplementedError("only the CHARM variant is shipped")

    @torch.no_grad()
    def decompress_batch(self, string_lists: Sequence[Sequence[bytes]], want_u8: bool = False):
        """All streams must carry the same (H, W, quality).  Returns (images, z_hat, y_hat[, uint8 HWC])."""
        hh = HeaderHandler()
        heads = []
        for sl in string_lists:
            assert len(sl) == 3, f"String list length should be 3 (header, z, and y), but got {len(sl)}"
            heads.append(hh.decode(sl[0]))
        H, W = heads[0]["img_size"]
        q = heads[0]["quality_ind"]
        for h in heads:
            if h["img_size"] != (H, W) or h["quality_ind"] != q:
                raise ValueError("decompress_batch needs equal image sizes and quality (group the streams first)")
        padH = int(np.ceil(H / self.model_stride)) * self.model_stride
        padW = int(np.ceil(W / self.model_stride)) * self.model_stride
        zH, zW = padH // self.model_stride, padW // self.model_stride
        beta_rate, beta_vq = self.selected_beta_rate[q], self.selected_beta_vq[q]
        _mark("begin")
        y_hat, z_hat = self._decompress_entropy([sl[1] for sl in string_lists], [sl[2] for sl in string_lists], zH, zW)
        _mark("entropy_decode_rans_cpu_charm_gpu")
        w = 1.0
        if max(H, W) > SPLIT_DECODE_RESOLUTION:
            fake = self.decode_split(y_hat, w, beta_rate=beta_rate, beta_vq=beta_vq)
        elif self._graphs.usable(len(string_lists) * padH * padW):
            fake = self._graphs.run(("dec", tuple(y_hat.shape), q, float(beta_rate), float(beta_vq), self.decoder_precision),
                                    lambda yh: self._decode(yh, w, beta_rate, beta_vq)[0], [y_hat.contiguous()],
                                    keep=lambda: list(self.decoder._vec_cache.values()),
                                    modules=self._segment_modules("dec"))
        else:
            fake, _ = self._decode(y_hat, w, beta_rate, beta_vq)
        _mark("decode_nn")
        if want_u8:
            img, u8 = ops.crop_clamp(fake, H, W, want_u8=True)
            _mark("postproc")
            return img, z_hat, y_hat, u8
        out = ops.crop_clamp(fake, H, W)
        _mark("postproc")
        return out, z_hat, y_hat

    @torch.no_grad()
    def decompress(self, string_list: List) -> Tuple[Tensor, Tensor, Tensor]:
        assert len(string_list) == 3, f"String list length should be 3 (header, z, and y), but got {len(string_list)}"
        return self.decompress_batch([string_list])


class _CharmEntropy:
    """What the two CHARM models share (hyperprior_charm_vic_model.py:14-52, hyperprior_charm_dc_vic_model.py:16-56): the context model
    among the sub-networks and the entropy side through it."""

    def _build_subnets(self) -> None:
        super()._build_subnets()
        self.context_model = build_subnet(self.opt["subnet"]["context_model"], "context_model")

    def _run_context(self, y, hyper_out, want_symbols, bits_y):
        return self.context_model.run(y, hyper_out, self.entropy_model_y, want_likelihood=True, want_symbols=want_symbols, bits_out=bits_y)

    def estimate_entropy(self, y: Tensor, is_train: bool = False):
        if is_train:
            raise NotImplementedError("dc_vic_amd implements the inference path only")
        return self._entropy_dict(y, self._entropy_encode_side(y, want_symbols=False))

    @staticmethod
    def _entropy_dict(y: Tensor, e: Dict) -> Dict:
        """estimate_entropy's keys from _entropy_encode_side's: in eval mode both likelihoods are the quantised one."""
        return {"quantized_code": {"y": e["y_hat"], "z": e["z_hat"]}, "latent_code": {"y": y, "z": e["z"]},
                "likelihoods": {"y": e["y_likelihood"], "z": e["z_likelihood"]},
                "q_likelihoods": {"y": e["y_likelihood"], "z": e["z_likelihood"]}}


@MODEL_REGISTRY.register()
class HyperpriorCharmDualCondVicModel(_CharmEntropy, HyperpriorDualCondVicModel):
    # hyperprior_charm_dc_vic_model.py:83-91
    def _decompress_entropy(self, z_strs, y_strs, zH: int, zW: int):
        z_hat = self.entropy_model_z.decompress(list(z_strs), (zH, zW))
        hyper_out = self.hyperdecoder(z_hat)
        y_hat, _ = self.context_model.forward_decompress(list(y_strs), hyper_out, self.entropy_model_y)
        return y_hat, z_hat


@MODEL_REGISTRY.register()
class HyperpriorCharmVicModel(_CharmEntropy, HyperpriorVicModel):
    """hyperprior_charm_vic_model.py over hyperprior_vic_model.py: the unconditioned model stage 1-1 trains (ElicVqCatScEncoder,
    ElicFeatFusionDecoder: no beta anywhere).  Inference here, training mode on the tape (train/nets.py); the reference has no
    compress / decompress for this class, nor has this one."""

    def _build_subnets(self) -> None:
        if _get(self.opt["subnet"], "residual_predictor"):
            raise NotImplementedError("Residual Predictor is not available yet in HypepriorCharmModel.")      # the reference's words (:19-20)
        super()._build_subnets()

    # hyperprior_vic_model.py:84-135 (run_model = data_preprocess, forward, data_postprocess)
    @torch.no_grad()
    def run_model(self, real_images: Tensor, is_train: bool = False, vq_indices=None, fusion_w: Optional[float] = None,
                  run_vq_decoder: bool = True, fix_entropy_models: bool = False) -> Dict:
        """The reference's keywords and no others: a beta here is a caller's mistake, not something to drop silently."""
        if is_train:
            raise NotImplementedError("dc_vic_amd implements the inference path only")
        if not run_vq_decoder:
            raise NotImplementedError("run_vq_decoder: false is not built")
        N, _, H, W = real_images.shape
        x = self.img_preprocess(real_images, is_train=False)
        gt_vq_latent, gt_vq_indices, feat = self.vq_encode(x, vq_indices, want_feat=True)
        y = self.comp_encode(x, gt_vq_latent, gt_vq_indices, feat=feat)
        e = self._entropy_encode_side(y, want_symbols=False)
        y_hat, z_hat = e["y_hat"], e["z_hat"]
        if max(x.shape[2:]) > SPLIT_DECODE_RESOLUTION:
            fake = self.decode_split(y_hat, 1.0, beta_rate=None, beta_vq=None)
            out_idx = torch.zeros_like(gt_vq_indices)
            logits = embed = None
            vq_acc = 0.0
        else:
            fake, out_idx, logits, embed = self._decode(y_hat, 1.0, None, None, want_logits=True, want_embed=True)
            vq_acc = float((out_idx.cpu() == gt_vq_indices.cpu()).float().mean())
        bpp = (e["bits_y"].double().sum() + e["bits_z"].double().sum()).item() / (N * H * W)          # as the dual model's run_model
        return dict(real_images=ops.crop_clamp(x, H, W), fake_images=ops.crop_clamp(fake, H, W), y_hat=y_hat, z_hat=z_hat,
                    out_vq_latent=embed, gt_vq_latent=gt_vq_latent, out_vq_logits=logits, gt_vq_indices=gt_vq_indices, vq_accuracy=vq_acc,
                    **self._entropy_dict(y, e), y_likelihood=e["y_likelihood"], z_likelihood=e["z_likelihood"], bpp=bpp,
                    y_q_likelihood=e["y_likelihood"], z_q_likelihood=e["z_likelihood"], qbpp=bpp, out_vq_indices=out_idx,
                    bits_per_image=(e["bits_y"] + e["bits_z"]))

    # hyperprior_vic_model.py:486-514
    @torch.no_grad()
    def validation(self, images: Sequence[Tensor], max_sample_size: int = 100) -> List[Dict]:
        """One row {idx, bpp, psnr, ms_ssim, vq_acc} per image of `images` ([1, 3, H, W] in [-1, 1], at most max_sample_size)."""
        from . import metrics
        rows = []
        for idx, x in enumerate(list(images)[:max_sample_size]):
            if x.dim() != 4 or x.shape[0] != 1:
                raise ValueError(f"validation: image {idx} has shape {tuple(x.shape)}, expected [1, 3, H, W]")
            out = self.run_model(x, is_train=False)
            ms, psnr = metrics.ms_ssim_psnr(out["real_images"], out["fake_images"])
            rows.append(dict(idx=idx + 1, bpp=float(out["bpp"]), psnr=float(psnr[0]), ms_ssim=float(ms[0]), vq_acc=float(out["vq_accuracy"])))
        return rows
