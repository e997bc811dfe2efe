#!/usr/bin/env python3
"""Stage-3 / 1-3 GAN training and stage 1-1 / 1-2 rate-distortion training of DC-VIC on MI355X -- counterpart of the reference's scripts/train.py:16-27 +
src/trainer/base_trainer.py:130-152 (train_loop) for the `DualBetaCondGanDistortionVqCodeTrainer` of config/exp1_stage3.yaml.

    python scripts/train.py CONFIG [--model_path CKPT | --synthetic_weights] [--dataset_root DIR | --synthetic_data]
                            [--batch_size 8] [--total_iter N] [--save_dir DIR] [--save_step N] [--seed S] [-d cuda:0]
                            [--data_workers N] [--data_depth 2]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 scripts/train.py ...

One process per GPU; every rank draws its own crops (sampler sharded by rank), gradients are averaged with bucketed RCCL
all-reduces of the flat gradient buffers (the reference is single-GPU, README.md:64-65).  Data: PNG / JPG files under
--dataset_root -> RandomCrop 256 (reflect pad if smaller) -> horizontal flip -> [-1, 1] (src/dataset/data_transform.py:19-45),
or seeded synthetic tensors.  The real-data stream is dc_vic_amd/train/data.py's: CropPlanner states it from the seed and the image
headers (without resize it is CropDataset's below, bit for bit), --data_workers threads decode --data_depth batches ahead, the crop's
source window travels as uint8 through pinned memory and one HIP launch per batch (csrc/data.hip) does Pillow's 8-bit resampling, the
flip, the [-1, 1] conversion and the NCHW layout; --data_workers 0 runs the same stream serially on the host (equal bits).  The YAML's
`dataset.train_dataset` section is honoured or refused before any GPU work (read_train_dataset: image_size 256, resize_range [f_min, f_max]
with interpolation bicubic / bilinear = the reference's PilRandomResize, root_dir and subset_list = its root_dir/train_{k}/*.jpg layout,
used when --dataset_root is absent or holds only train_{k} folders); `dataset.batch_size` is reported, --batch_size decides; rank 0 prints
`[train] data: ...`.  --resume replays the plan's draws, so a resumed run sees the batches of the uninterrupted one.  Checkpoints use the reference's file format: `comp_model_iterXXXXXXX.pth.tar` =
{'iter', 'comp_model': state_dict}, `discriminator_iter...` = {'iter', 'discriminator': state_dict} (model_saver.py:39-46).
The optimizer / loss settings are the YAML's `optim` / `loss` sections when present (config/exp1_stage1_3.yaml:43-79), else
their stage-3 values (g_scheduler and d_scheduler milestones are read separately).  Every `loss` entry's `type` and keywords are
honoured or refused before any GPU work (dc_vic_amd/train/losses.py read_loss_section: CrossEntropyLoss / FocalCrossEntropyLoss,
MSELoss normalize_img / mse_scale, VanillaMSELoss reduction, LPIPSLoss alex; under the rate-distortion trainer also the distortions
L1Loss and MSSSIMLoss, csrc/msssim_loss.hip, on crops with min(H, W) > 160); rank 0 prints them as `[train] losses: ...`.
Without `model.use_selected_beta_pairs` (config/exp1_stage1_3.yaml) beta_rate and beta_vq are drawn per sample from the
(num_beta_levels + 1)-point grids; `trainer.beta_policy` / `trainer.beta_offset` are read by no GAN trainer of the reference and ignored there.  LPIPS: pass --lpips_path (a torch.save'd state
dict of lpips.LPIPS(net='alex'), loaded with weights_only=True); its weights cannot be fetched offline, so without it a positive
perceptual weight is an ERROR unless --allow_synthetic_lpips opts into synthetic AlexNet weights (benchmarks / plumbing only).
`model.gumbel_sampling: true` (GAN trainers only; the rate-distortion trainer refuses it): the decoder reads a hard Gumbel-softmax
sample of the code logits instead of their argmax (csrc/gumbel.hip), so the distortion, perceptual and adversarial losses reach the VQ
estimator; `model.gumbel_kwargs` may set `tau` (> 0, default 1) and nothing else (train/build.py read_gumbel_options); the noise comes from a device
generator the trainer owns, saved in and restored from the training state (rank 0's); rank 0 prints `[train] VQ sampling: ...`.
--save_step also writes training_state_iter*.pth.tar (Adam moments, step counts, scheduler epochs, beta-sampler RNG; the
reference saves optimizer + scheduler state too, base_trainer.py:178-214) and --resume continues from it.
Validation (base_trainer.py:130-192): every --eval_step iterations (YAML `eval_step`, 0 = off) rank 0 runs the sorted *.png of
--eval_dataset_root (YAML `dataset.eval_dataset.root_dir`; at most 100, decoded once at start-up) through the model and prints
`validation iterN` with one `key: value` line per metric; with --save_dir the row {iter, <label>_<metric>...} is appended to
<save_dir>/eval_result.csv (--resume carries the earlier rows over).  Its time is left out of samples/s.
GAN loss: `DualBetaCondGanDistortionVqCodeTrainer` (PatchGAN, VanillaGANLoss) or `DualBetaCondOasisGanDistortionVqFusionTrainer`
(config/dc_vic_oasis.yaml: 257-way per-token discriminator, OasisGANLoss), chosen by --gan {vanilla,oasis}, else the YAML's
`trainer.type`, else `loss.gan_loss.type`, else the discriminator's `out_nc` (1 -> vanilla, n_embed + 1 -> oasis); see choose_gan_trainer
in dc_vic_amd/train/build.py, which holds the choice of the trainer, the mapping of the YAML's sections to its arguments and build_trainer.
Rate-distortion (config/exp1_stage1_2.yaml): `trainer.type: DualBetaCondRateDistortionVqCodeTrainer` builds dc_vic_amd/train/rd_trainer.py
(choose_trainer, in front of choose_gan_trainer): the whole model but the VQGAN trains on rate + distortion + perceptual + code losses with
per-sample weights exp(beta) or beta + offset (`trainer.beta_policy`, `beta_offset`, `sample_beta_batch`; `loss.rate_loss` and the
`reduction: none` entries are read), `optim.aux_optimizer.lr` drives the entropy bottleneck's quantiles.  No discriminator is built and
no discriminator_* file is written or read (the trainer's checkpoint_modules names the files of a checkpoint); --gan with such a config is an error.
Stage 1-1 (config/exp1_stage1_1.yaml, config/dc_vic_synthetic_stage1_1.yaml): `trainer.type: RateDistortionVqCodeTrainer` over `model.type:
HyperpriorCharmVicModel` trains the unconditioned model (no beta pair, plain reductions) under `optim.g_scheduler`'s LinearWarmupScheduler
(read_g_scheduler; `optim.g_optimizer` / `aux_optimizer` are read by read_rd_optimizers); over another model type it is refused.  It is the
one stage that starts without a checkpoint: with neither --model_path nor --synthetic_weights the model is initialised from --seed by the
reference's constructor rules (dc_vic_amd/train/init.py) around the pretrained VQGAN of `subnet.vq_model.ckpt_path`, which must exist.
A stage 1-2 run starts from a stage 1-1 or a dual-conditioned checkpoint (--model_path) or synthetic weights: where the checkpoint's keys
and the model's differ, rank 0 prints `[train] weights: N tensors loaded; missing ...; unexpected ...` by module, and the conditioning
modules a stage 1-1 file lacks keep their constructor initialisation.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from glob import glob

import numpy as np
import torch

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dc_vic_amd import BaseConfig, build_comp_model  # noqa: E402
from dc_vic_amd.parallel import launched_by_a_launcher, pin_rank_cpus, self_launch  # noqa: E402
from dc_vic_amd.train.build import (RD_STAGE_1_1, build_discriminator, build_rd_trainer, build_trainer, choose_gan_trainer, choose_trainer,  # noqa: E402,F401
                                    from_scratch_vqgan, get_in, read_discriminator, read_gumbel_options, weight_load_report)
from dc_vic_amd.train.init import reference_init_  # noqa: E402
from dc_vic_amd.train.data import HostFeed, TrainFeed, list_train_images, read_train_dataset  # noqa: E402
from dc_vic_amd.train.losses import read_loss_section  # noqa: E402
from dc_vic_amd.train.trainer import DEFAULT_LOSS  # noqa: E402
from dc_vic_amd.train.validation import EvalCSV, eval_image_paths, load_eval_images  # noqa: E402


class CropDataset:
    """OpenImages-style folder -> random 256 crops, flips, [-1, 1]; sharded by rank, reshuffled every epoch."""

    def __init__(self, root: str, size: int, rank: int, world: int, seed: int):
        self.paths = sorted(p for ext in ("png", "jpg", "jpeg") for p in glob(os.path.join(root, f"*.{ext}")))
        assert self.paths, f'dataset_root "{root}" holds no image'
        self.size, self.rank, self.world = size, rank, world
        self.rng = np.random.RandomState(seed * 1000 + rank)
        self.order, self.pos = [], 0

    def _next_path(self) -> str:
        if self.pos >= len(self.order):
            perm = np.random.RandomState(len(self.order) + 17).permutation(len(self.paths))     # same permutation on every rank
            self.order = [int(i) for i in perm[self.rank::self.world]] or [int(perm[0])]
            self.pos = 0
        p = self.paths[self.order[self.pos]]
        self.pos += 1
        return p

    def batch(self, n: int) -> torch.Tensor:
        from PIL import Image
        out = torch.empty((n, 3, self.size, self.size), dtype=torch.float32)
        for i in range(n):
            a = np.asarray(Image.open(self._next_path()).convert("RGB"), dtype=np.uint8)
            H, W = a.shape[:2]
            if H < self.size or W < self.size:        # RandomCrop(pad_if_needed, padding_mode='reflect')
                a = np.pad(a, ((0, max(0, self.size - H)), (0, max(0, self.size - W)), (0, 0)), mode="reflect")
                H, W = a.shape[:2]
            y0, x0 = self.rng.randint(0, H - self.size + 1), self.rng.randint(0, W - self.size + 1)
            c = a[y0:y0 + self.size, x0:x0 + self.size]
            if self.rng.rand() < 0.5:
                c = c[:, ::-1]
            out[i] = (torch.from_numpy(c.copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5
        return out


def list_training_set(a, opt):
    """The training images of a run, before any GPU work (pure host: the YAML's `dataset` section and a directory listing) ->
    None for --synthetic_data, else dict(paths, root, layout "flat" | "subsets", section = read_train_dataset's dict).  --dataset_root DIR
    is listed flat (sorted png / jpg / jpeg, as CropDataset lists it); if DIR holds no image at its top level but the `train_{k}`
    folders of the YAML's subset_list, it is read by subsets (openimage_dataset.py:14-34).  Without --dataset_root the YAML's
    dataset.train_dataset.root_dir is used, by subsets when the YAML names a subset_list.  SystemExit names the key and value the
    section is refused for, a missing folder and an empty listing."""
    if a.synthetic_data:
        return None
    try:
        sec = read_train_dataset(opt, threaded=a.data_workers != 0)
    except ValueError as e:
        raise SystemExit(str(e))
    root, src = (a.dataset_root, "--dataset_root") if a.dataset_root else (sec["root_dir"], "dataset.train_dataset.root_dir")
    if not root:
        raise SystemExit("no training data: pass --dataset_root DIR or --synthetic_data, or set dataset.train_dataset.root_dir in the YAML")
    if not os.path.isdir(root):
        raise SystemExit(f'{src}: folder "{root}" does not exist')
    sub = sec["subset_list"]
    try:
        if a.dataset_root:
            paths, layout = list_train_images(root), "flat"
            if not paths and sub and any(os.path.isdir(os.path.join(root, f"train_{k}")) for k in sub):
                paths, layout = list_train_images(root, sub), "subsets"
        else:
            paths, layout = (list_train_images(root, sub), "subsets") if sub else (list_train_images(root), "flat")
    except ValueError as e:
        raise SystemExit(f"{src}: {e}")
    if not paths:
        raise SystemExit(f'{src}: folder "{root}" holds no image ({"train_{k}/*.jpg of subset_list " + str(sub) if layout == "subsets" else "*.png, *.jpg, *.jpeg"})')
    return dict(paths=paths, root=root, layout=layout, section=sec)


def build_train_data(a, opt, rank, world, device, listing=None):
    """(feed, log line) of a run's real-data stream, (None, None) for --synthetic_data: TrainFeed (decode threads, pinned uint8, one HIP
    launch per batch) or, with --data_workers 0, HostFeed (serial, on the host).  Both serve the stream of CropPlanner, which without
    resize_range is CropDataset's bit for bit.  `listing`: list_training_set's answer when the caller already has it."""
    listing = list_training_set(a, opt) if listing is None else listing
    if listing is None:
        return None, None
    sec = listing["section"]
    kw = dict(resize_range=sec["resize_range"], interpolation=sec["interpolation"])
    if a.data_workers == 0:
        feed, how = HostFeed(listing["paths"], 256, rank, world, a.seed, **kw), "serial on the host (--data_workers 0)"
    else:
        feed = TrainFeed(listing["paths"], 256, rank, world, a.seed, device, workers=a.data_workers, depth=a.data_depth, **kw)
        how = f"{feed.workers} decode threads, depth {feed.depth}"
    rr = sec["resize_range"]
    line = (f"data: {len(listing['paths'])} images under \"{listing['root']}\" ({'flat' if listing['layout'] == 'flat' else 'by subsets ' + str(sec['subset_list'])}); "
            f"crop 256; resize " + ("off" if rr is None else f"[{rr[0]:g}, {rr[1]:g}] {sec['interpolation']}") + f"; {how}"
            + (f"; the YAML's dataset.batch_size {sec['batch_size']} is not used, --batch_size {a.batch_size} decides"
               if sec["batch_size"] is not None and sec["batch_size"] != a.batch_size else ""))
    return feed, line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("config_path", type=str)
    p.add_argument("--model_path", type=str, default=None)
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--dataset_root", type=str, default=None)
    p.add_argument("--synthetic_data", action="store_true")
    p.add_argument("--batch_size", type=int, default=8, help="per GPU (the reference trains with 6, BASELINE config 5 asks 8)")
    p.add_argument("--total_iter", type=int, default=None)
    p.add_argument("--save_dir", type=str, default=None)
    p.add_argument("--save_step", type=int, default=0)
    p.add_argument("--log_step", type=int, default=10)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("-d", "--device", type=str, default="cuda:0")
    p.add_argument("--lpips_path", type=str, default=None, help="state dict of lpips.LPIPS(net='alex') (torch.save'd; loaded with weights_only=True)")
    p.add_argument("--allow_synthetic_lpips", action="store_true", help="train the perceptual term against SYNTHETIC AlexNet / head weights (plumbing / benchmarks only)")
    p.add_argument("--resume", type=str, default=None, help="training_state_iterXXXXXXX.pth.tar written by --save_step (loads the comp_model / discriminator files beside it)")
    p.add_argument("--gpus", type=int, default=0, help="data-parallel over N GPUs of this node: without a launcher this process starts the N ranks itself")
    p.add_argument("--eval_dataset_root", type=str, default=None, help="folder of eval PNGs (overrides the YAML's dataset.eval_dataset.root_dir)")
    p.add_argument("-e", "--eval_step", type=int, default=None, help="validate every N iterations (overrides the YAML's eval_step; 0 = off)")
    p.add_argument("--gan", choices=("vanilla", "oasis"), default=None, help="GAN loss / trainer (default: from the YAML, see choose_gan_trainer)")
    p.add_argument("--data_workers", type=int, default=None, help="image decode threads of this rank (default: min(8, its share of the cores)); 0 = the serial host path")
    p.add_argument("--data_depth", type=int, default=2, help="batches decoded ahead of the trainer")
    a = p.parse_args()
    if (a.data_workers is not None and a.data_workers < 0) or a.data_depth < 1:
        raise SystemExit(f"--data_workers {a.data_workers} / --data_depth {a.data_depth}: need workers >= 0 and depth >= 1")
    opt0 = BaseConfig.fromfile(a.config_path, {"is_train": True})
    gan_kind, trainer_name, _ = choose_trainer(opt0, a.gan)                # before any GPU work
    from_scratch = trainer_name == RD_STAGE_1_1 and not a.model_path and not a.synthetic_weights
    vqgan_path = from_scratch_vqgan(opt0) if from_scratch else None        # likewise: a start from the initialisation needs the VQGAN
    losses = read_loss_section(opt0)                                       # likewise: every `loss` entry is honoured or refused
    if gan_kind != "rd":
        read_gumbel_options(opt0)                                          # likewise
        d_read = read_discriminator(opt0)                                  # likewise: the type and every option it does not build
        if d_read["norm_type"] == "actnorm" and max(a.gpus, int(os.environ.get("WORLD_SIZE", "1"))) > 1:
            raise SystemExit("discriminator.norm_type: actnorm cannot train on more than one rank: its data-dependent initialisation (loc and "
                             "scale from the first batch) would differ per rank")
    listing = list_training_set(a, opt0)                                   # likewise: the `dataset` section, the folder, its listing
    if a.eval_dataset_root is not None:
        try:                                          # a folder named on the command line must hold PNGs: checked before any GPU work
            eval_image_paths(a.eval_dataset_root)
        except ValueError as e:
            raise SystemExit(f"--eval_dataset_root: {e}")
    if a.gpus > 1 and not launched_by_a_launcher():
        sys.exit(self_launch(a.gpus))                     # parent: never touches the GPU
    if a.gpus > 0 and int(os.environ.get("WORLD_SIZE", "1")) != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE', '1')}")

    rank, world, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))
    eval_images = None
    if a.eval_dataset_root is not None and rank == 0:
        try:
            eval_images = load_eval_images(a.eval_dataset_root)
        except ValueError as e:
            raise SystemExit(f"--eval_dataset_root: {e}")
    pin_rank_cpus()
    dist = None
    device = a.device
    if world > 1:
        import torch.distributed as dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        device = f"cuda:{local_rank}"
        torch.cuda.set_device(local_rank)
        dist_.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(device))
        dist = dist_
    opt = BaseConfig.fromfile(a.config_path, {"device": device, "is_train": True})
    ck = opt["subnet"]["vq_model"].get("ckpt_path")
    if ck and not os.path.exists(ck):
        opt["subnet"]["vq_model"]["ckpt_path"] = None
    if from_scratch:
        torch.manual_seed(a.seed)                   # identical initialisation on every rank
    model = build_comp_model(opt)
    if a.synthetic_weights:
        from dc_vic_amd.synth import load_synth_weights
        load_synth_weights(model, 1234)
    elif from_scratch:
        reference_init_(model, torch.Generator().manual_seed(a.seed))
        if rank == 0:
            print(f"[train] weights: initialised from seed {a.seed}; VQGAN from {vqgan_path}", flush=True)
    else:
        line = weight_load_report(model.load_learned_weight(ckpt_path=a.model_path))
        if line and rank == 0:
            print("[train] " + line, flush=True)
    torch.manual_seed(a.seed)                       # identical D initialisation on every rank
    D, d_line = (None, None) if gan_kind == "rd" else build_discriminator(opt, device)             # the rate-distortion trainer has none
    w_perc = losses["weights"].get("perceptual", DEFAULT_LOSS["perceptual"])
    lpips_state = None
    if a.lpips_path:
        lpips_state = torch.load(a.lpips_path, map_location="cpu", weights_only=True)
    elif w_perc > 0:
        msg = (f"perceptual_loss has weight {w_perc} but no --lpips_path was given: the `lpips` AlexNet / head weights cannot be fetched "
               "offline, so the term would be computed with SYNTHETIC weights (not LPIPS).")
        if not a.allow_synthetic_lpips:
            raise SystemExit(msg + "  Pass --lpips_path STATE_DICT, set loss.perceptual_loss.loss_weight: 0, or opt in with --allow_synthetic_lpips.")
        if rank == 0:
            print("[train] WARNING: " + msg, file=sys.stderr, flush=True)
    trainer, lines = build_trainer(opt, losses, model, D, dist, a.seed * 100 + rank, lpips_state, a.gan)
    if rank == 0:
        for line in lines + ([d_line] if d_line else []):
            print("[train] " + line, flush=True)
    start_iter = 0
    if a.resume:
        # base_trainer.py:178-214: comp_model / discriminator / training_state files of one iteration
        st = torch.load(a.resume, map_location="cpu", weights_only=False)        # our own file (numpy RNG state inside)
        d_ = os.path.dirname(a.resume)
        it_tag = os.path.basename(a.resume).replace("training_state_", "")
        for name, mod in trainer.checkpoint_modules().items():
            mod.load_state_dict(torch.load(os.path.join(d_, f"{name}_" + it_tag), map_location="cpu", weights_only=True)[name])
        trainer.resync_parameters()
        start_iter = trainer.load_training_state(st)
    total_iter = a.total_iter or int(get_in(opt, "total_iter", default=500000))
    eval_step = a.eval_step if a.eval_step is not None else int(get_in(opt, "eval_step", default=10000))
    eval_root = a.eval_dataset_root or get_in(opt, "dataset", "eval_dataset", "root_dir", default=None)
    if a.eval_dataset_root is None and eval_root and eval_step > 0 and rank == 0:
        if os.path.isdir(eval_root) and glob(os.path.join(eval_root, "*.png")):
            eval_images = load_eval_images(eval_root)
        else:
            print(f'[train] eval_dataset.root_dir "{eval_root}" holds no PNG: training without validation', flush=True)
    do_eval = bool(eval_root) and eval_step > 0 and (rank != 0 or eval_images is not None)
    if world > 1:                                     # every rank must agree on whether to meet at the validation barrier
        flag = torch.tensor([1 if do_eval else 0], device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        do_eval = bool(flag.item())
    eval_csv = None
    if do_eval and rank == 0 and a.save_dir:
        os.makedirs(a.save_dir, exist_ok=True)
        path = os.path.join(a.save_dir, "eval_result.csv")
        prev = None
        if a.resume:                                  # base_trainer.py: the job's CSV is loaded and extended
            prev = path if os.path.exists(path) else os.path.join(os.path.dirname(a.resume), "eval_result.csv")
        eval_csv = EvalCSV(path, resume_from=prev, start_iter=start_iter)
    gen = torch.Generator().manual_seed(a.seed * 7919 + rank)
    if a.save_dir and rank == 0:
        os.makedirs(a.save_dir, exist_ok=True)
    data, data_line = build_train_data(a, opt, rank, world, device, listing)
    try:                                              # the feed's threads are joined on every way out
        if data_line and rank == 0:
            print("[train] " + data_line, flush=True)
        if data is None:
            for _ in range(start_iter):          # resume: the synthetic stream continues where the interrupted run stopped
                torch.rand((a.batch_size, 3, 256, 256), generator=gen)
        else:
            data.skip(start_iter * a.batch_size)  # likewise the real one: the plan replays its draws from the image headers
        t0 = time.perf_counter()
        t_eval = 0.0                                      # time spent in validation (and at its barrier): not training throughput
        for it in range(start_iter + 1, total_iter + 1):
            x = (torch.rand((a.batch_size, 3, 256, 256), generator=gen) * 2 - 1) if data is None else data.batch(a.batch_size)
            log = trainer.optimize_parameters(it, {"real_images": x})
            if rank == 0 and (it % a.log_step == 0 or it == 1 or it == total_iter):
                dt = time.perf_counter() - t0 - t_eval
                msg = "skipped (loss anomaly)" if log is None else " ".join(f"{k} {v:.5g}" for k, v in log.items())
                print(f"iter {it:7d} | {world * a.batch_size * (it - start_iter) / dt:7.2f} samples/s | {msg}", flush=True)
            if do_eval and it % eval_step == 0:
                tv = time.perf_counter()
                if rank == 0:
                    res = trainer.validation(it, eval_images)
                    # base_trainer.py:178-192: the log lines, then the CSV row
                    print(f"validation iter{it} ({time.perf_counter() - tv:.2f} s)\n" + "".join(f"\t {k}: {v:.4f}\n" for k, v in res.items()),
                          end="", flush=True)
                    if eval_csv is not None:
                        eval_csv.append({"iter": it, **res})
                if dist is not None:
                    dist.barrier()
                t_eval += time.perf_counter() - tv
            if a.save_dir and a.save_step and it % a.save_step == 0 and rank == 0:
                for name, mod in trainer.checkpoint_modules().items():
                    torch.save({"iter": it, name: {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}},
                               os.path.join(a.save_dir, f"{name}_iter{it:07d}.pth.tar"))
                torch.save(trainer.training_state(it), os.path.join(a.save_dir, f"training_state_iter{it:07d}.pth.tar"))
    finally:
        if data is not None:
            data.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
