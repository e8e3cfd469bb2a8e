#!/usr/bin/env python3
"""ViT-B/16 at 384^2 (577 tokens), batch 64, bf16 training step: the key-tiled attention kernels (ops.ATTN_LONG = True, the
default) against the materialised fp32 attention the step took before (False), alternating in blocks of STEPS steps for ROUNDS
rounds in one process.  Per arm: ms/step (mean, std, min over blocks), img/s and torch.cuda.max_memory_allocated over the arm's
blocks.  PRECISION=bf16x3h (or any other ViT precision; default bf16) runs that precision's step instead: for bf16x3h the arms
are the key-tiled half kernels against the materialised fp32 path, for fp32 / bf16x3 the key-tiled fp32 kernels against it; the
lines then carry a "precision" field.

    ROUNDS=4 STEPS=5 [PRECISION=bf16x3h|fp32|bf16x3] python tools/bench_long_step.py [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
import torch  # noqa: E402

from myrtle_vision.hip import ops  # noqa: E402
from myrtle_vision.hip.functional import cross_entropy  # noqa: E402
from myrtle_vision.models.vit import ViT  # noqa: E402
from myrtle_vision.utils.optim import AdamW, ParamArena  # noqa: E402
from myrtle_vision.utils.utils import seed_everything  # noqa: E402

ROUNDS, STEPS, BATCH, SIZE = int(os.environ.get("ROUNDS", 4)), int(os.environ.get("STEPS", 5)), int(os.environ.get("BATCH", 64)), 384
PRECISION = os.environ.get("PRECISION", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    seed_everything(1234)
    vit = ViT(decoder="classification", image_size=SIZE, patch_size=16, num_classes=1000, dim=768, depth=12, heads=12,
              mlp_dim=3072, precision=PRECISION, q_format="FP32").to(dev)
    opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=6.25e-5, weight_decay=0.05)
    g = torch.Generator().manual_seed(1234)
    img = torch.randn(BATCH, 3, SIZE, SIZE, generator=g).to(dev)
    labels = torch.randint(0, 1000, (BATCH,), generator=g).to(dev)
    vit.train()

    def step():
        opt.zero_grad()
        loss = cross_entropy(vit(img), labels)
        loss.backward()
        opt.step()

    arms = {"long": True, "materialised": False}
    for on in arms.values():
        ops.ATTN_LONG = on
        for _ in range(2):
            step()
    times = {k: [] for k in arms}
    peak = {k: 0 for k in arms}
    for _ in range(ROUNDS):
        for k, on in arms.items():
            ops.ATTN_LONG = on
            step()                                    # one untimed step after the switch
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(STEPS):
                step()
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / STEPS)
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
    ops.ATTN_LONG = True
    lines = []
    for k in arms:
        t = times[k]
        rec = {"arm": k, "image_size": SIZE, "tokens": (SIZE // 16) ** 2 + 1, "batch": BATCH, "ms_per_step": round(statistics.mean(t), 2),
               "std": round(statistics.pstdev(t), 2), "min": round(min(t), 2), "img_per_s": round(BATCH / statistics.mean(t) * 1e3, 1),
               "max_memory_allocated_GB": round(peak[k] / 1e9, 2), "blocks": f"{ROUNDS} x {STEPS} steps",
               "device": torch.cuda.get_device_name(0)}
        if PRECISION != "bf16":
            rec["precision"] = PRECISION
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
