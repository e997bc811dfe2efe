#!/usr/bin/env python3
"""Bit equality of the three trainers between two trees of this repository (a parent commit's export and a working tree with the same
csrc/), the way profiles/tape_refactor_equivalence.json was made: the same seeded work in one process per tree, hashes compared.

    python tools/trainer_equivalence.py --root TREE --out FILE            # on the GPU, once per tree: the package found under TREE
    python tools/trainer_equivalence.py --merge PARENT.json THIS.json [--step-time FILE] --out profiles/trainer_refactor_equivalence.json

Work, per case of CASES on config/dc_vic_synthetic.yaml with load_synth_weights(1234), LPIPS on (synthetic weights), betas sampled:
step 1; step 2 with w['distortion'] = 1e9 (skipped); step 3; training_state through torch.save / torch.load into a fresh trainer (another
seed) on a fresh model given the first one's state_dict and resync_parameters(); step 4 there.  Hashed (sha256 of the bytes) after every
step: the returned log (keys, values as float64, or None), flat / m / v of every group, last_beta_rate / last_beta_vq, last_fake of the
GAN trainers; of the training state every tensor and array and the structure with its scalars.  Step 3's library calls are counted by
tools/analysis_tape_bench.count_calls.  Trainers are built by their constructors, which both trees have."""
import argparse
import hashlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import torch

DEV = "cuda:0"
SMALL, LARGE = (2, 3, 64, 64), (1, 3, 192, 192)        # MS-SSIM needs min(H, W) > 160
# config/exp1_stage1_2.yaml's trainer and loss sections as the trainer's arguments (tests/test_rd_trainer_host.py pins this dict)
STAGE_1_2 = dict(lr=1e-4, aux_lr=1e-3, milestones=[300000], gamma=0.1, clip_max_norm=1.0,
                 loss_weights=dict(distortion=50.0, perceptual=1.0, code_distortion=0.006, code_ce=0.003, rate=0.5),
                 beta_policy="exp", beta_offset=1.0, sample_beta_batch=True, rate_reduction="none", code_ce_gamma=2.0, code_ce_reduction="none",
                 code_distortion_reduction="none", distortion_factor=0.25, distortion_type="MSELoss", gumbel_sampling=False)
CASES = {
    "a_vanilla": ("vanilla", {}, SMALL),
    "b_oasis": ("oasis", {}, SMALL),
    "c_gumbel": ("vanilla", dict(gumbel_sampling=True, gumbel_kwargs=dict(tau=0.5)), SMALL),
    "d_focal_sum": ("vanilla", dict(code_ce_loss=("FocalCrossEntropyLoss", 0.5, 2.0), code_distortion_reduction="sum"), SMALL),
    "e_rd_stage_1_2": ("rd", STAGE_1_2, SMALL),
    "f_rd_linear_shared_beta": ("rd", dict(beta_policy="linear", sample_beta_batch=False, rate_reduction="none", code_ce_reduction="none",
                                           code_distortion_reduction="none"), SMALL),
    "g_rd_l1": ("rd", dict(STAGE_1_2, distortion_type="L1Loss"), SMALL),
    "h_rd_msssim": ("rd", dict(STAGE_1_2, distortion_type="MSSSIMLoss"), LARGE),
}


def sha(raw: bytes) -> str:
    return hashlib.sha256(raw).hexdigest()


def put(items, name, t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    items[name] = {"numel": int(a.size), "sha256": sha(a.reshape(-1).view(np.uint8).data)}


def put_log(items, name, log):
    if log is None:
        items[name] = {"numel": 0, "sha256": sha(b"None")}
        return
    keys = list(log)
    items[name] = {"numel": len(keys), "sha256": sha(",".join(keys).encode() + np.asarray([log[k] for k in keys], dtype=np.float64).tobytes())}


def put_state(items, name, st):
    """Every tensor / array of a training state under its path, and one item for the structure: paths, types and scalar values."""
    lines = []

    def walk(path, v):
        if isinstance(v, dict):
            for k in sorted(v):
                walk(f"{path}/{k}", v[k])
        elif isinstance(v, (tuple, list)):
            lines.append(f"{path}: {type(v).__name__}[{len(v)}]")
            for i, e in enumerate(v):
                walk(f"{path}/{i}", e)
        elif isinstance(v, (torch.Tensor, np.ndarray)):
            lines.append(f"{path}: {type(v).__name__} {v.dtype} {tuple(v.shape)}")
            put(items, f"{name}{path}", v)
        else:
            lines.append(f"{path}: {type(v).__name__} {v!r}")
    walk("", st)
    items[f"{name}/structure"] = {"numel": len(lines), "sha256": sha("\n".join(lines).encode())}


def run_tree(root: str, out: str) -> None:
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    from dc_vic_amd import BaseConfig, build_comp_model
    from dc_vic_amd.synth import load_synth_weights
    from dc_vic_amd import train as T
    assert os.path.abspath(T.__file__).startswith(root + os.sep), (T.__file__, root)
    spec = importlib.util.spec_from_file_location("dcvic_tape_bench_of_tree", os.path.join(root, "tools", "analysis_tape_bench.py"))
    tape_bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tape_bench)

    def fresh(kind, kw, seed):
        m = build_comp_model(BaseConfig.fromfile(os.path.join(root, "config", "dc_vic_synthetic.yaml"), {"device": DEV}))
        load_synth_weights(m, 1234)
        if kind == "rd":
            return m, None, T.DualBetaCondRateDistortionVqCodeTrainer(m, seed=seed, **kw)
        kw = dict(kw)
        if "code_ce_loss" in kw:
            name, *args = kw["code_ce_loss"]
            kw["code_ce_loss"] = getattr(T, name)(*args)
        torch.manual_seed(0)                # tools/train_bench.py's discriminators
        dkw = dict(out_nc=m.vq_model.quantize.embedding.weight.shape[0] + 1, keep_shape=True) if kind == "oasis" else {}
        D = T.DualBetaCondTamingNLayerDiscriminator(input_nc=11, n_layers=3, ndf=64, norm_type="none", max_beta_1=3.0, max_beta_2=3.5, **dkw).to(DEV)
        cls = T.DualBetaCondOasisGanDistortionVqFusionTrainer if kind == "oasis" else T.DualBetaCondGanDistortionVqCodeTrainer
        return m, D, cls(m, D, seed=seed, **kw)

    def groups(tr):
        return {k: getattr(tr, k) for k in ("g_group", "d_group", "group", "aux_group") if hasattr(tr, k)}

    items, calls = {}, {}
    for i, (case, (kind, kw, shape)) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(1000 + i)
        xs = [torch.rand(shape, generator=gen) * 2 - 1 for _ in range(4)]
        m, D, tr = fresh(kind, kw, seed=7)

        def step(t, it, key):
            log = t.optimize_parameters(it, {"real_images": xs[it - 1]})
            put_log(items, f"{key}/log", log)
            for gname, g in groups(t).items():
                for part in ("flat", "m", "v"):
                    put(items, f"{key}/{gname}/{part}", getattr(g, part))
            put(items, f"{key}/last_beta_rate", t.last_beta_rate)
            put(items, f"{key}/last_beta_vq", t.last_beta_vq)
            if getattr(t, "last_fake", None) is not None:
                put(items, f"{key}/last_fake", t.last_fake)
            return log

        assert step(tr, 1, f"{case}/step1") is not None, f"{case}: step 1 was skipped"
        w = tr.w["distortion"]
        tr.w["distortion"] = 1e9
        assert step(tr, 2, f"{case}/step2_skipped") is None, f"{case}: step 2 was not skipped"
        tr.w["distortion"] = w
        calls[case] = tape_bench.count_calls(lambda: step(tr, 3, f"{case}/step3"))
        buf = io.BytesIO()
        torch.save(tr.training_state(3), buf)
        st = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=False)
        put_state(items, f"{case}/training_state", st)
        m2, D2, t2 = fresh(kind, kw, seed=99)
        m2.load_state_dict(m.state_dict())
        if D is not None:
            D2.load_state_dict(D.state_dict())
        t2.resync_parameters()
        assert t2.load_training_state(st) == 3
        assert step(t2, 4, f"{case}/step4_resumed") is not None, f"{case}: step 4 was skipped"
        print(f"[equivalence] {case}: {calls[case]} library calls in step 3", flush=True)
        del m, D, tr, m2, D2, t2
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump({"root": os.path.basename(root), "device": torch.cuda.get_device_name(0), "library_calls_step3": calls, "items": items}, f, indent=1)
        f.write("\n")


def merge(parent: str, this: str, step_time, out: str) -> None:
    with open(parent) as f:
        P = json.load(f)
    with open(this) as f:
        Q = json.load(f)
    names = sorted(set(P["items"]) | set(Q["items"]))
    items = {}
    for n in names:
        p, q = P["items"].get(n), Q["items"].get(n)
        items[n] = {"numel": (q or p)["numel"], "sha256_parent": p and p["sha256"], "sha256_this": q and q["sha256"],
                    "equal": p is not None and q is not None and p == q}
    unequal = [n for n in names if not items[n]["equal"]]
    doc = {"what": "parent commit against this commit, the same seeded work in one process per tree on one MI355X (tools/trainer_equivalence.py): per case "
                   "step 1, a skipped step 2 (distortion x 1e9), step 3, the training state through torch.save / torch.load into a fresh trainer "
                   "on a fresh model, step 4 there; hashed after every step: the log, flat / m / v of every group, the beta pair, last_fake; and "
                   "the training state's structure and tensors",
           "cases": {k: {"trainer": v[0], "options": v[1], "shape": list(v[2])} for k, v in CASES.items()},
           "device": Q.get("device"), "all_equal": not unequal, "unequal": unequal,
           "library_calls_step3": {"counted_by": "tools/analysis_tape_bench.count_calls around optimize_parameters", "parent": P["library_calls_step3"],
                                   "this": Q["library_calls_step3"], "same": P["library_calls_step3"] == Q["library_calls_step3"]}}
    if step_time:
        with open(step_time) as f:
            doc["step_time"] = json.load(f)
    doc["items"] = items
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"all_equal {doc['all_equal']} over {len(names)} items; library calls the same: {doc['library_calls_step3']['same']}")
    if unequal:
        print("unequal: " + ", ".join(unequal[:20]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", help="the tree whose dc_vic_amd runs the work (needs a GPU)")
    p.add_argument("--merge", nargs=2, metavar=("PARENT", "THIS"), help="two --root results -> the record (needs no GPU)")
    p.add_argument("--step-time", help="a JSON document to store under the record's step_time key")
    p.add_argument("--out", required=True)
    a = p.parse_args()
    if bool(a.root) == bool(a.merge):
        raise SystemExit("give --root TREE or --merge PARENT THIS")
    if a.root:
        run_tree(a.root, a.out)
    else:
        merge(a.merge[0], a.merge[1], a.step_time, a.out)


if __name__ == "__main__":
    main()
