#!/usr/bin/env python3
"""Forward + backward of the fused segmentation tail at the segmentation workload's own shapes (B = 256, C = 17, 14^2 -> 224^2 and
16^2 -> 256^2; bf16 gradient, ld = 24), four variants in one process, alternating:

    a  mv_seg_ce_*                                      (the plain mean cross entropy: what bench.py --workload seg runs)
    b  mv_seg_loss_* with every option off
    c  mv_seg_loss_* with class weights + label smoothing
    d  mv_seg_loss_* with class weights + label smoothing + Dice

Device events round ``--iters`` back-to-back calls, after a warm-up of every variant; ``--rounds`` rounds, median / min / max of the
per-call time and the ratio of the medians to (a).  Per-pixel HBM bytes are the same for all four by construction (forward: label 8 +
lse 4 + pred 1; backward: 2 x (label 8 + lse 4)); Dice adds a pass over the C probabilities per pixel and the per-class reductions.

    python tools/bench_seg_loss.py [--batch 256] [--iters 20] [--rounds 7]        -> profiles/seg_loss_tail.txt is this output
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "myrtle-vision_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from myrtle_vision.hip import ops  # noqa: E402

SHAPES = [(14, 224), (16, 256)]
C, LD = 17, 24


def variants(small, labels, weight, B, g, S):
    def plain(fwd=True, bwd=True, keep={}):
        if fwd:
            keep["f"] = ops.seg_ce_fwd(small, labels, B, C, g, g, S, S)
        if bwd:
            stats, lse, _, lab = keep["f"]
            ops.seg_ce_bwd(small, lab, lse, B, C, g, g, S, S, grad_dtype=torch.bfloat16, ld=LD, stats=stats)

    def recipe(cw, eps, lam):
        kw = dict(class_weight=cw, label_smoothing=eps, dice_weight=lam)

        def run(fwd=True, bwd=True, keep={}):
            if fwd:
                keep["f"] = ops.seg_loss_fwd(small, labels, B, C, g, g, S, S, dice_smooth=1.0, **kw)
            if bwd:
                stats, lse, _, coef, _, lab = keep["f"]
                ops.seg_loss_bwd(small, lab, lse, stats, coef, B, C, g, g, S, S, grad_dtype=torch.bfloat16, ld=LD, **kw)
        return run
    return {"a seg_ce": plain, "b seg_loss off": recipe(None, 0.0, 0.0), "c weights+smoothing": recipe(weight, 0.1, 0.0),
            "d weights+smoothing+dice": recipe(weight, 0.1, 0.5)}


def timed(fn, iters, **kw):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn(**kw)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3             # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_loss needs an MI355X: there is no CPU path to time")
    B = a.batch
    print(f"# fused segmentation tail, microseconds per call (device events round {a.iters} calls, {a.rounds} rounds, alternating); "
          f"B {B}, C {C}, bf16 gradient ld {LD}; commit {os.environ.get('MV_COMMIT', 'unknown')}, torch {torch.__version__}, "
          f"{torch.cuda.get_device_name(0)}")
    print("# shape variant window median_us min_us max_us ratio_to_a")
    gen = torch.Generator().manual_seed(0)
    for g, S in SHAPES:
        small = (3.0 * torch.randn(B * g * g, C, generator=gen)).cuda()
        labels = torch.randint(0, C, (B, S, S), generator=gen).cuda()
        weight = (0.25 + 1.5 * torch.rand(C, generator=gen)).cuda()
        vs = variants(small, labels, weight, B, g, S)
        windows = {"fwd+bwd": dict(fwd=True, bwd=True), "fwd": dict(fwd=True, bwd=False), "bwd": dict(fwd=False, bwd=True)}
        for fn in vs.values():                                # warm-up: code objects, the allocator's blocks
            timed(fn, 3)
        us = {(v, wn): [] for v in vs for wn in windows}
        for _ in range(a.rounds):
            for wn, kw in windows.items():
                for v, fn in vs.items():
                    us[(v, wn)].append(timed(fn, a.iters, **kw))
        for wn in windows:
            base = statistics.median(us[("a seg_ce", wn)])
            for v in vs:
                t = us[(v, wn)]
                print(f"{g}x{g}->{S}x{S} | {v} | {wn} | {statistics.median(t):.1f} {min(t):.1f} {max(t):.1f} {statistics.median(t) / base:.3f}")
        del small, labels, vs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
