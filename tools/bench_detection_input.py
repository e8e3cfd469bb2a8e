#!/usr/bin/env python3
"""Detection input at the validation size: mv_image_prepare_ragged against the host chain (Pillow + collate) for one batch of 8
synthetic frames of mixed sizes resized to 800 on the short side (the shipped transform_ops_val).  Both are timed in the same
process, in alternating rounds; the outputs are compared bit for bit first.  GPU box:

    python tools/bench_detection_input.py [OUTPUT.txt]
"""
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "myrtle-vision_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from myrtle_vision.datasets.detection_transforms import collate_fn, from_config  # noqa: E402
from myrtle_vision.datasets.device_transforms import DetectionDevicePlan  # noqa: E402
from myrtle_vision.hip import ops  # noqa: E402

SIZES = ((800, 800), (600, 800), (800, 600), (480, 640), (720, 1280), (512, 512), (1000, 750), (640, 960))    # (h, w)
ROUNDS, KERNEL_ITERS, HOST_ITERS = 5, 50, 3

section = json.load(open(os.path.join(ROOT, "detection", "data_configs", "data_config.json")))["transform_ops_val"]
rng = np.random.default_rng(0)
frames = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in SIZES]
target = lambda: {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64), "area": torch.zeros(0),
                  "iscrowd": torch.zeros(0, dtype=torch.int64)}
host_chain, plan = from_config(section), DetectionDevicePlan(section)
threads = max(1, min(16, len(os.sched_getaffinity(0)), len(frames)))
pool = ThreadPoolExecutor(threads)


def host_batch():
    return collate_fn(list(pool.map(lambda f: host_chain(f, target()), frames)))


packed, _ = plan.collate([plan(f, target()) for f in frames])
d = {k: v.cuda() for k, v in packed.items() if k != "norm"}
mean, std = (tuple(float(v) for v in row) for row in packed["norm"])
run = lambda: ops.image_prepare_ragged(d["raw"], d["kh"], d["bh"], d["kv"], d["bv"], d["ext"], mean, std)
want = host_batch()[0]
img, mask = run()
torch.cuda.synchronize()
assert torch.equal(img.cpu(), want.tensors) and torch.equal(mask.cpu(), want.mask), "device batch differs from the host batch"
for _ in range(10):
    run()
torch.cuda.synchronize()

kernel_us, host_ms = [], []
start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(ROUNDS):
    start.record()
    for _ in range(KERNEL_ITERS):
        run()
    end.record()
    torch.cuda.synchronize()
    kernel_us.append(start.elapsed_time(end) / KERNEL_ITERS * 1e3)
    t0 = time.perf_counter()
    for _ in range(HOST_ITERS):
        host_batch()
    host_ms.append((time.perf_counter() - t0) / HOST_ITERS * 1e3)

B, _, H, W = img.shape
out_bytes = img.numel() * 4 + mask.numel()
src_bytes = sum(h * w * 3 for h, w in SIZES)
k, hst = statistics.median(kernel_us), statistics.median(host_ms)
lines = [
    f"# tools/bench_detection_input.py on {torch.cuda.get_device_name(0)}: {B} frames {list(SIZES)} -> padded batch {H} x {W} "
    f"(transform_ops_val: 800 on the short side, max 1333), taps per output pixel <= {d['kh'].shape[2]}",
    f"# {ROUNDS} alternating rounds; kernel: device events round {KERNEL_ITERS} launches; host: wall clock of {HOST_ITERS} batches, "
    f"Pillow resize + ToTensor + Normalize on {threads} threads, then the padded collate; decode is in neither",
    f"mv_image_prepare_ragged   median {k:9.1f} us per batch   (rounds: {', '.join(f'{v:.1f}' for v in kernel_us)})",
    f"host chain + collate      median {hst * 1e3:9.1f} us per batch   (rounds: {', '.join(f'{v * 1e3:.0f}' for v in host_ms)})",
    f"bytes per batch: {out_bytes / 1e6:.1f} MB written (fp32 batch + mask), {src_bytes / 1e6:.1f} MB of uint8 source "
    f"-> {out_bytes / k / 1e3:.1f} GB/s of output at the kernel's median",
    f"outputs identical bit for bit: yes",
]
print("\n".join(lines))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
