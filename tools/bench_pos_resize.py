#!/usr/bin/env python3
"""First-visit cost of ViT._pos_embedding at a grid the model has not seen (GPU): wall clock from the call to a device
synchronise, host work included -- what a detection step pays when its batch has a new padded (H, W).

Two paths on the same model, alternating: "matrix" = the host-built [gh*gw, 196] matrix, its blocking upload and one fp32 product
(what every non-native grid took before mv_pos_resize_fwd, and still the fallback), "kernel" = F.pos_resize.  Each grid is measured
once per path per round and is fresh for the matrix path every time (its cache is cleared).

    python tools/bench_pos_resize.py [--dim 768] [--rounds 5]        -> profiles/pos_resize.txt is this output
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "myrtle-vision_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from myrtle_vision.hip import functional as F  # noqa: E402
from myrtle_vision.models.vit import ViT  # noqa: E402

GRIDS = [(20, 33), (30, 50), (40, 66)]            # short side 320 / 480 / 640 at the 5:3 shape of the detection range


def matrix_path(vit, gh, gw):
    vit.__dict__.pop("_pos_resize_cache", None)                                   # first visit
    grid = vit.pos_embedding[0, 1:, :]
    out = F.linear(vit._pos_resize_matrix(gh, gw, grid.device), grid.t().contiguous(), None)
    return torch.cat((vit.pos_embedding[:, 0:1, :], out.unsqueeze(0)), dim=1)


def kernel_path(vit, gh, gw):
    return vit._pos_embedding(gh, gw)


def timed(fn, vit, gh, gw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn(vit, gh, gw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del r
    return dt * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    vit = ViT(decoder="detection", image_size=224, patch_size=16, num_classes=91, dim=a.dim, depth=1, heads=a.dim // 64,
              mlp_dim=4 * a.dim, q_format="FP32", precision="bf16").cuda().eval()
    print(f"# first-visit cost of _pos_embedding, ms wall clock incl. host work and a device synchronise; dim {a.dim}, "
          f"{a.rounds} rounds, commit {os.environ.get('MV_COMMIT', 'unknown')}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        for fn in (matrix_path, kernel_path):                                     # load code objects at a grid that is not timed
            timed(fn, vit, 9, 11)
        print("# grid path median_ms min_ms max_ms")
        for gh, gw in GRIDS:
            ms = {"matrix": [], "kernel": []}
            for _ in range(a.rounds):
                ms["matrix"].append(timed(matrix_path, vit, gh, gw))
                ms["kernel"].append(timed(kernel_path, vit, gh, gw))
            for name, v in ms.items():
                print(f"{gh}x{gw} {name} {statistics.median(v):.3f} {min(v):.3f} {max(v):.3f}")
        vit.__dict__.pop("_pos_resize_cache", None)


if __name__ == "__main__":
    main()
