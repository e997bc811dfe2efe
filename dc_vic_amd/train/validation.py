"""Host side of the trainer's validation (base_trainer.py:130-192, dual_cond_rate_distortion_vq_code_trainer.py:202-233): the eval set
and the CSV log.  No GPU work here: the eval set is decoded once on the host; the metrics run on the GPU in
HyperpriorDualCondVicModel.validation and DualBetaCondGanDistortionVqCodeTrainer.validation."""
from __future__ import annotations

import csv
import os
from glob import glob
from typing import Dict, List, Optional

import numpy as np
import torch

MAX_EVAL_IMAGES = 100          # _validation's max_sample_size
MAX_EVAL_SIDE = 1024           # comp_model.SPLIT_DECODE_RESOLUTION: larger images decode tiled, where out_vq_latent (vq_mse) is None


def eval_image_paths(root: str, max_images: int = MAX_EVAL_IMAGES) -> List[str]:
    """The sorted *.png of `root` (kodak_dataset.py:22-23), at most `max_images`; ValueError if the folder is missing or holds none."""
    if not os.path.isdir(root):
        raise ValueError(f'eval_dataset_root "{root}" is not a directory')
    paths = sorted(glob(os.path.join(root, "*.png")))
    if not paths:
        raise ValueError(f'eval_dataset_root "{root}" holds no PNG')
    return paths[:max_images]


def load_eval_images(root: str, max_images: int = MAX_EVAL_IMAGES) -> List[torch.Tensor]:
    """The eval set as host fp32 [1, 3, H, W] tensors in [-1, 1] (ToTensor + Normalize(0.5, 0.5), data_transform.py:50-51).  An image
    with a side over 1024 is refused: validation reports vq_mse, which the tiled decoder of larger images does not produce."""
    from PIL import Image
    out = []
    for p in eval_image_paths(root, max_images):
        a = np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8)
        if max(a.shape[:2]) > MAX_EVAL_SIDE:
            raise ValueError(f"eval image {p} is {a.shape[1]} x {a.shape[0]}: validation takes sides up to {MAX_EVAL_SIDE} "
                             "(larger images decode tiled, without the predicted VQ latent that vq_mse needs)")
        out.append(((torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255.0) - 0.5) / 0.5)[None].contiguous())
    return out


class EvalCSV:
    """<save_dir>/eval_result.csv as logger.py:33-65 (CSVLogger) writes it: a header row, then one row per validation, `iter` an
    integer, floats as Python's shortest round-trip repr; the whole file is rewritten on every append.  `resume_from` (a CSV of an
    earlier run) and `start_iter`: its rows up to start_iter are carried over, so a run resumed from a checkpoint ends with the same
    file as an uninterrupted one."""

    def __init__(self, path: str, resume_from: Optional[str] = None, start_iter: int = 0):
        self.path = path
        self.header: Optional[List[str]] = None
        self.rows: List[List[str]] = []
        if resume_from is not None and os.path.exists(resume_from):
            with open(resume_from, newline="") as f:
                rd = list(csv.reader(f))
            if rd:
                self.header = rd[0]
                if not self.header or self.header[0] != "iter":
                    raise ValueError(f"{resume_from}: not an eval_result.csv (first column {self.header[:1]})")
                self.rows = [r for r in rd[1:] if r and int(r[0]) <= start_iter]
            self._write()

    def append(self, row: Dict[str, float]) -> None:
        keys = list(row.keys())
        if keys[0] != "iter":
            raise ValueError("eval row: the first key must be 'iter'")
        if self.header is None:
            self.header = keys
        elif keys != self.header:
            raise ValueError(f"eval row keys {keys} differ from the CSV header {self.header}")
        self.rows.append([str(int(row["iter"]))] + [repr(float(row[k])) for k in keys[1:]])
        self._write()

    def _write(self) -> None:
        if self.header is None:
            return
        tmp = self.path + ".tmp"
        with open(tmp, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(self.header)
            w.writerows(self.rows)
        os.replace(tmp, self.path)
