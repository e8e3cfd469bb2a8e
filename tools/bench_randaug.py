#!/usr/bin/env python3
"""Device time of the classification input chain with and without RandAugment (GPU), B = 256, 256^2 frames -> 224^2:

    a  today's chain: one mv_image_prepare
    b  the RandAugment chain (mv_image_resize_u8, 2 slots of mv_randaug_stats + mv_randaug_apply, mv_image_prepare through copying
       tables) on noise frames
    c  the same on flat frames: every pixel of an image in one histogram bin, the worst case of the LDS atomics
    d  the host chain's RandAugment alone (Pillow, one CPU core) per image, and what 8 workers deliver against the 7 300 img/s
       the training step consumes

a-c: device events round ``--iters`` calls on resident inputs (no upload), medians of ``--rounds`` alternating rounds, then a second
plain series (each variant's rounds back to back).  With prob 1.0 every slot runs an op, drawn as the worker draws them.

    python tools/bench_randaug.py [--rounds 15] [--iters 10]          -> profiles/randaug.txt is this output
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "myrtle-vision_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from myrtle_vision.datasets.device_transforms import DevicePlan  # noqa: E402
from myrtle_vision.datasets.transforms import RandAugment  # noqa: E402

NORM = {"Mean": [0.5] * 3, "Std": [0.5] * 3}
BASE = {"RandomResizedCrop": 224, "RandomHorizontalFlip": None, "Normalize": NORM}
STEP_IMG_S = 7300.0


def resident(plan, frames):
    random.seed(0)
    packed, _ = DevicePlan.collate([(plan(f), 0) for f in frames])
    return {k: v.cuda() for k, v in packed.items()}


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3             # microseconds per batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_randaug needs an MI355X: there is no CPU path to time")
    B = a.batch
    rng = np.random.default_rng(0)
    noise = [Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)) for _ in range(B)]
    flat = [Image.fromarray(np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (256, 256, 3)).copy()) for _ in range(B)]
    ra = {"prob": 1.0, "num_ops": 2}
    plain, aug = DevicePlan(BASE), DevicePlan(dict(BASE, RandAugment=ra))
    dev = torch.device("cuda")
    inputs = {"a image_prepare": (plain, resident(plain, noise)), "b randaug noise": (aug, resident(aug, noise)),
              "c randaug flat": (aug, resident(aug, flat))}
    vs = {name: (lambda p=p, d=d: p.apply(d, dev)) for name, (p, d) in inputs.items()}
    print(f"# classification input chain, microseconds per batch of {B} (256x256 -> 224x224; device events round {a.iters} calls, "
          f"{a.rounds} rounds); commit {os.environ.get('MV_COMMIT', 'unknown')}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}")
    print("# variant | series | median_us min_us max_us ratio_to_a img_per_s")
    for fn in vs.values():
        timed(fn, 3)
    alt = {v: [] for v in vs}
    for _ in range(a.rounds):
        for v, fn in vs.items():
            alt[v].append(timed(fn, a.iters))
    back = {v: [timed(fn, a.iters) for _ in range(a.rounds)] for v, fn in vs.items()}
    for series, us in (("alternating", alt), ("plain", back)):
        base = statistics.median(us["a image_prepare"])
        for v, t in us.items():
            m = statistics.median(t)
            print(f"{v} | {series} | {m:.1f} {min(t):.1f} {max(t):.1f} {m / base:.3f} {B / (m * 1e-6):.0f}")
    # d: Pillow on one core, the 224 x 224 images RandAugment sees in the host chain
    host = RandAugment(ra, NORM["Mean"])
    small = [f.resize((224, 224)) for f in noise]
    random.seed(0)
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        for f in small:
            host(f)
        ms.append((time.perf_counter() - t0) / B * 1e3)
    per = statistics.median(ms)
    print(f"d host RandAugment (Pillow, 1 core, 2 ops at prob 1.0): {per:.3f} ms/img = {1e3 / per:.0f} img/s/core; 8 workers "
          f"{8e3 / per:.0f} img/s = {8e3 / per / STEP_IMG_S:.2f} x the {STEP_IMG_S:.0f} img/s the step consumes (RandAugment alone, "
          f"decode and crop not counted)")
    print("e the training loop with and without the key: tools/bench_train_loop.py 24 256 4 classification vit_base_mixup_re.json "
          "and ... vit_base_mixup_re_ra.json, each in a process of its own")


if __name__ == "__main__":
    main()
