#!/usr/bin/env python3
"""A fingerprint of the training loops: ``engine.train_worker`` on the synthetic trees of the engine tests (depth-2 models, a handful
of iterations) for classification (one micro-batch per step), classification with two micro-batches and ``clip_grad``, segmentation
with a weight EMA, and detection.  Prints the loops' own ``Iteration`` lines and a sha256 per tensor of each run's last checkpoint
(``model``, optimizer ``state``, ``model_ema``).  Public API only: run the same file in two checkouts and diff the outputs.
usage: loop_fingerprint.py WORKDIR      (WORKDIR keeps the trees and the checkpoints)"""
import contextlib, copy, hashlib, io, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
import torch
from myrtle_vision.datasets.synthetic import make_dior_coco, make_dlrsd, make_resisc45
from myrtle_vision.engine import train_worker

RUNS = {"classification": ("classification", "vit_tiny.json", dict(local_batch_size=8, global_batch_size=8)),
        "classification_accum2_clip": ("classification", "vit_tiny.json", dict(local_batch_size=4, global_batch_size=8, clip_grad=0.05)),
        "segmentation_ema": ("segmentation", "seg_tiny.json", dict(local_batch_size=8, global_batch_size=8, model_ema_decay=0.5)),
        "detection": ("detection", "yolos_tiny.json", dict(local_batch_size=2, global_batch_size=2))}


def config(name, work):
    task, train, extra = RUNS[name]
    cfg = json.load(open(os.path.join(ROOT, task, "train_configs", train)))
    data = json.load(open(os.path.join(ROOT, task, "data_configs", "data_config.json")))
    if task == "classification":
        data["dataset_path"] = make_resisc45(os.path.join(work, "NWPU-RESISC45"), classes=45, per_class=2)
    elif task == "segmentation":
        data["dataset_path"] = make_dlrsd(os.path.join(work, "DLRSD_dataset"), count=48)
    else:
        norm = {"Normalize": {"Mean": [0.5] * 3, "Std": [0.5] * 3}}
        data["dataset_path"] = make_dior_coco(os.path.join(work, "DIOR-COCO"), counts=(8, 4, 4))
        data.update(train_subset=None, valid_subset=None, transform_ops_val={"RandomResize": {"scales": [96], "max_size_ratio": [4, 3]}, **norm},
                    transform_ops_train={"RandomHorizontalFlip": None, "RandomResize": {"scales": [64, 80], "max_size_ratio": [4, 3]}, **norm})
        cfg["vit_config"].update(embed_dim=64, heads=1, mlp_dim=128, num_det_tokens=10, precision="fp32")
    cfg["data_config_path"] = os.path.join(work, "data_config.json")
    json.dump(data, open(cfg["data_config_path"], "w"))
    cfg["train_config"].update(output_directory=os.path.join(work, "ckpt"), epochs=1, iters_per_checkpoint=1, iters_per_val=2, distributed=False,
                               pretrained_backbone=None, tensorboard_dir=os.path.join(work, "runs"), **extra)
    cfg["vit_config"]["depth"] = 2
    return task, cfg


def tensors(prefix, obj):
    if torch.is_tensor(obj):
        yield prefix, hashlib.sha256(obj.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
    elif isinstance(obj, dict):
        for k in obj:
            yield from tensors(f"{prefix}.{k}", obj[k])


for name in RUNS:
    work = os.path.join(sys.argv[1], name)
    os.makedirs(work, exist_ok=True)
    task, cfg = config(name, work)
    print(f"== {name}", flush=True)
    with contextlib.redirect_stdout(io.StringIO()) as said:
        train_worker(0, 1, copy.deepcopy(cfg), task)
    print("".join(line for line in said.getvalue().splitlines(True) if line.startswith("Iteration")), end="")
    out = cfg["train_config"]["output_directory"]
    last = sorted(os.listdir(out))[-1]
    ck = torch.load(os.path.join(out, last), map_location="cpu", weights_only=False)
    print(f"checkpoint {last} iteration {ck['iteration']}")
    for part in ("model", "optimizer", "model_ema"):
        for key, digest in tensors(part, ck[part]["state"] if part == "optimizer" else ck.get(part)):
            print(f"{digest}  {key}", flush=True)
