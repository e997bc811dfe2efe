"""Training step of DC-VIC on HIP kernels: a reverse-mode tape (autograd.py), the backward / loss /
optimizer kernels (csrc/train.hip via kernels.py), differentiable forwards of the trainable sub-networks, the PatchGAN and the
OASIS U-Net discriminators with their BatchNorm / ActNorm layers (nets.py, csrc/bn_train.hip) and the stage-3 GAN trainers (PatchGAN / BCE and OASIS / per-token cross entropy, csrc/chan_ce.hip) with
data-parallel gradient averaging (trainer.py); the stage 1-2 rate-distortion trainer with per-sample beta weights and the stage 1-1 trainer of the unconditioned model (rd_trainer.py,
csrc/sample_loss.hip); the initialisation a stage 1-1 run starts from (init.py); the code losses of the YAML's `loss` section (plain and focal cross entropy,
csrc/chan_ce.hip) and its host-side reading (losses.py); the choice and construction of the trainer a config asks for (build.py:
choose_trainer, rd_trainer_kwargs / gan_trainer_kwargs, build_trainer); the real-data feed (data.py: the seeded crop plan, Pillow's 8-bit resampling
restated, decode threads, pinned uint8 staging and the one launch of csrc/data.hip per batch)."""
from .autograd import Ctx, ParamGroup, Var  # noqa: F401
from .nets import DualBetaCondTamingNLayerDiscriminator, OasisDualBetaCondTamingNLayerDiscriminator  # noqa: F401
from .trainer import (Adam, DualBetaCondGanDistortionVqCodeTrainer, DualBetaCondOasisGanDistortionVqFusionTrainer, LinearWarmupScheduler, MultiStepLR,  # noqa: F401
                      OasisGANLoss, allreduce_mean_, sample_beta_grid)
from .rd_trainer import DualBetaCondRateDistortionVqCodeTrainer, RateDistortionVqCodeTrainer  # noqa: F401
from .losses import CrossEntropyLoss, FocalCrossEntropyLoss, RateLoss, read_loss_section, sample_loss_weights  # noqa: F401
from .data import CropPlanner, HostFeed, TrainFeed, list_train_images, pil_coeffs, read_train_dataset, window  # noqa: F401
