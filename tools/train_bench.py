#!/usr/bin/env python3
"""samples/s of the stage-3 training step (BASELINE config 5: 256x256 crops, batch 8 per GPU, G + D step) -- a SEPARATE metric,
never mixed into bench.py's headline.  python tools/train_bench.py [--gan {vanilla,oasis} | --stage 1_2 [--distortion {MSELoss,L1Loss,MSSSIMLoss}] | --stage 1_1] [--batch 8] [--steps 5] [--warmup 2]
[--disc_norm {none,batchnorm,actnorm}] [--disc unet]
(--disc_norm: the discriminator's normalisation layers, csrc/bn_train.hip; --disc unet: the OASIS U-Net discriminator with --gan oasis; --gan oasis: the 257-class per-token discriminator of config/dc_vic_oasis.yaml and the OASIS cross-entropy loss; --stage 1_2: the
rate-distortion step of train/rd_trainer.py with config/exp1_stage1_2.yaml's trainer and loss sections, no discriminator; --stage 1_1: the
unconditioned model's step with config/dc_vic_synthetic_stage1_1.yaml, from the synthetic weights the two models share); under
torch.distributed.run it is data-parallel (weak scaling) and reports the aggregate."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--gan", choices=("vanilla", "oasis"), default="vanilla")
    p.add_argument("--disc_norm", choices=("none", "batchnorm", "actnorm"), default="none", help="the discriminator's norm_type")
    p.add_argument("--disc", choices=("patchgan", "unet"), default="patchgan", help="unet: the OASIS U-Net discriminator (needs --gan oasis)")
    p.add_argument("--stage", choices=("3", "1_2", "1_1"), default="3",
                   help="3: the G + D step (default); 1_2: the rate-distortion step; 1_1: the unconditioned model's rate-distortion step")
    p.add_argument("--distortion", choices=("MSELoss", "L1Loss", "MSSSIMLoss"), default="MSELoss", help="--stage 1_2: distortion_loss.type")
    a = p.parse_args()
    rank, world, lr_ = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(lr_)
    dev = f"cuda:{lr_}"
    dist = None
    if world > 1:
        import torch.distributed as dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist_.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
        dist = dist_
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    cfg = BaseConfig.fromfile(os.path.join(ROOT, "config", "dc_vic_synthetic_stage1_1.yaml" if a.stage == "1_1" else "dc_vic_synthetic.yaml"), {"device": dev})
    m = build_comp_model(cfg)
    load_synth_weights(m, 1234)
    if a.stage == "1_1":
        from dc_vic_amd.train.build import build_rd_stage_1_1_trainer
        from dc_vic_amd.train.losses import read_loss_section
        tr, what = build_rd_stage_1_1_trainer(cfg, read_loss_section(cfg), m, dist, rank, None)[0], "stage 1-1 rate-distortion step (unconditioned model)"
    elif a.stage == "1_2":
        tr, what = rd_trainer(m, dist, rank, a.distortion), "stage 1-2 rate-distortion step" + (f" ({a.distortion})" if a.distortion != "MSELoss" else "")
    else:
        tr, what = gan_trainer(a, m, dev, dist, rank), "stage-3 G+D step"
    g = torch.Generator().manual_seed(100 + rank)
    x = torch.rand((a.batch, 3, 256, 256), generator=g) * 2 - 1
    for _ in range(a.warmup):
        tr.optimize_parameters(0, {"real_images": x})
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(a.steps):
        log = tr.optimize_parameters(i, {"real_images": x})
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    if rank == 0:
        print(json.dumps({"metric": f"training samples/sec, {what} @256x256", "value": world * a.batch * a.steps / dt, "unit": "samples/s",
                          "gan": a.gan if a.stage == "3" else None, "disc": a.disc if a.stage == "3" else None,
                          "disc_norm": a.disc_norm if a.stage == "3" else None, "stage": a.stage, "n_gpus": world, "steps": a.steps, "ms_per_step": 1e3 * dt / a.steps,
                          "batch_per_gpu": a.batch, "dtype": "f32",
                          "data": "synthetic", "lpips": "included, synthetic weights (parity unpinned)", "last_log": log}), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def rd_trainer(m, dist, rank, distortion="MSELoss"):
    from dc_vic_amd.train import DualBetaCondRateDistortionVqCodeTrainer
    from dc_vic_amd.train.build import rd_trainer_kwargs
    from dc_vic_amd.train.losses import read_loss_section
    with open(os.path.join(ROOT, "tests", "golden", "reference_loss_sections.json")) as f:
        opt = json.load(f)["exp1_stage1_2.yaml"]
    if distortion != "MSELoss":
        opt["loss"]["distortion_loss"] = dict(type=distortion, loss_weight=opt["loss"]["distortion_loss"]["loss_weight"])
    return DualBetaCondRateDistortionVqCodeTrainer(m, dist=dist, seed=rank, **rd_trainer_kwargs(opt, read_loss_section(opt)))


def gan_trainer(a, m, dev, dist, rank):
    from dc_vic_amd.train import (DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondOasisGanDistortionVqFusionTrainer,
                                  DualBetaCondTamingNLayerDiscriminator, OasisDualBetaCondTamingNLayerDiscriminator)
    torch.manual_seed(0)
    n_cls = m.vq_model.quantize.embedding.weight.shape[0] + 1
    if a.disc == "unet":
        if a.gan != "oasis":
            raise SystemExit("--disc unet needs --gan oasis: its logits are one class column per VQ token")
        D = OasisDualBetaCondTamingNLayerDiscriminator(input_nc=6, cond_ch=3, n_layers=4, num_upsample=1, ndf=64, out_nc=n_cls, norm_type=a.disc_norm,
                                                       max_beta_1=3.0, max_beta_2=3.5).to(dev)
    else:
        dkw = dict(out_nc=n_cls, keep_shape=True) if a.gan == "oasis" else {}
        D = DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type=a.disc_norm, max_beta_1=3.0, max_beta_2=3.5, **dkw).to(dev)
    cls = DualBetaCondOasisGanDistortionVqFusionTrainer if a.gan == "oasis" else DualBetaCondGanDistortionVqCodeTrainer
    return cls(m, D, dist=dist, seed=rank)

if __name__ == "__main__":
    main()
