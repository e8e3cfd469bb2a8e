#!/usr/bin/env python3
"""Generate the detection golden vectors by running the REFERENCE's own ViT(decoder="detection"), HungarianMatcher and
SetCriterion in the build container (the reference does not exist on the GPU box; nothing under tests/ reads it at test time):

    python tests/golden/gen_golden_detection.py

The reference is imported as ``gen_golden.py`` imports it (same qtorch stand-in, never called for q_format FP32).  Its detection
modules also import ``torchvision.ops.boxes``; torchvision is not installed, so a two-name in-memory stand-in is registered:
``box_convert`` and ``generalized_box_iou`` written from their definitions (torchvision/ops/boxes.py: areas, pairwise
intersection with clamp(min=0), union, enclosing box with clamp(min=0), ``iou - (areai - union) / areai``, no epsilon).

Parameters and inputs are formulas in ``oracle/detinit.py``; the targets are the formula ``det_targets`` below (recorded in the
json): 0..12 boxes per image, image 0 with none, widths and heights > 0.02.

A test that demands identical matcher indices could fail from near-ties alone, so every image's assignment is re-solved with the
cost matrix perturbed by +-1e-4 (uniform, 32 draws); a fixture whose indices change under any draw is not written: the target
seed is redrawn until the assignment is stable, and the smallest margin seen (second-best assignment cost minus the optimum,
over the images) is recorded.

The box losses have the same weakness one step later.  L1's gradient is sign(pred - target), GIoU's goes through max / min of the
corners and a clamp of the intersection width: where a matched prediction sits on such a point, the gradient JUMPS (by
2 * loss_bbox weight / num_boxes in one entry for L1), and a gradient comparison at any tolerance is decided by which side an
arithmetic's rounding lands on, not by its accuracy.  The coarsest arithmetic the fixtures judge is bf16, whose outputs are held
to 1.5e-2 of max |value| (tests/test_vit_parity.py BF16_LOGITS; boxes are sigmoids, max <= 1).  So a target set is also refused
while any matched pair has a coordinate within KINK_MARGIN = 1.5e-2 of its target's (L1), or a corner (cx +- w/2: 1.5 x the
coordinate error) within 1.5 * KINK_MARGIN of the target's corner (the max / min selections) or an intersection width or height
within 1.5 * KINK_MARGIN of zero (the clamp).  The smallest gap of the accepted set is recorded (``kink_check``).  Few sets
pass both checks (the more matched boxes, the fewer), so SEEDS seeds are tried and the accepted set with the most targets is kept;
ragged and large target sets are the business of the kernel cases in tests/detection_ref.py, which are judged against fp64.
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")


def box_convert(boxes, in_fmt, out_fmt):
    assert (in_fmt, out_fmt) == ("cxcywh", "xyxy")
    cx, cy, w, h = boxes.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def generalized_box_iou(boxes1, boxes2):
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = area1[:, None] + area2 - inter
    iou = inter / union
    lti = torch.min(boxes1[:, None, :2], boxes2[:, :2])
    rbi = torch.max(boxes1[:, None, 2:], boxes2[:, 2:])
    whi = (rbi - lti).clamp(min=0)
    areai = whi[:, :, 0] * whi[:, :, 1]
    return iou - (areai - union) / areai


def install_torchvision_standin():
    tv = sys.modules.get("torchvision") or types.ModuleType("torchvision")
    tvo, tvb = types.ModuleType("torchvision.ops"), types.ModuleType("torchvision.ops.boxes")
    tvb.box_convert, tvb.generalized_box_iou = box_convert, generalized_box_iou
    tvo.boxes = tvb
    tvo.box_convert, tvo.generalized_box_iou = box_convert, generalized_box_iou
    tv.ops = tvo
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.ops"] = tvo
    sys.modules["torchvision.ops.boxes"] = tvb


def det_targets(tag: str, seed: int, batch: int, num_classes: int):
    """Image 0: no targets; image b > 0: 1..12 boxes (a function of (tag, seed, b)); cx, cy in [0.2, 0.8], w, h in
    [0.03, 0.4] (> 0.02), labels in [0, num_classes)."""
    from oracle.detinit import _gen
    out = []
    for b in range(batch):
        g = _gen(f"dettgt:{tag}:{seed}:{b}")
        n = 0 if b == 0 else int(torch.randint(1, 13, (1,), generator=g))
        u = torch.rand(n, 4, generator=g)
        boxes = torch.stack((0.2 + 0.6 * u[:, 0], 0.2 + 0.6 * u[:, 1], 0.03 + 0.37 * u[:, 2], 0.03 + 0.37 * u[:, 3]), dim=-1)
        labels = torch.randint(0, num_classes, (n,), generator=g)
        out.append({"labels": labels, "boxes": boxes.float()})
    return out


def assignment_margin(cost: np.ndarray, draws: int = 32, eps: float = 1e-4, seed: int = 0):
    """(stable?, margin).  stable: the assignment is unchanged when the matrix is perturbed by uniform(-eps, eps), ``draws`` times.
    margin: cost of the second-best assignment minus the optimum -- the best solution that avoids one pair of the optimum, for
    every such pair (+inf without targets)."""
    if cost.shape[1] == 0:
        return True, float("inf")
    i0, j0 = linear_sum_assignment(cost)
    base = cost[i0, j0].sum()
    rng = np.random.default_rng(seed)
    stable = True
    for _ in range(draws):
        i, j = linear_sum_assignment(cost + rng.uniform(-eps, eps, size=cost.shape))
        stable = stable and np.array_equal(i, i0) and np.array_equal(j, j0)
    margin = float("inf")
    for a, b in zip(i0, j0):
        c = cost.copy()
        c[a, b] = 1e6
        i, j = linear_sum_assignment(c)
        margin = min(margin, float(cost[i, j].sum() - base))
    return stable, margin


KINK_MARGIN = 1.5e-2
SEEDS = 20000        # target seeds tried: the accepted set with the most targets is kept (ties: the smallest seed)


def kink_gap(pred: np.ndarray, tgt: np.ndarray) -> float:
    """Matched cxcywh boxes [n, 4] each: the smallest distance of a pair to a non-differentiable point of loss_bbox / loss_giou, in
    units of its margin (>= 1: far enough).  Coordinates against KINK_MARGIN; corners and the intersection extents against 1.5 x."""
    if len(pred) == 0:
        return float("inf")
    pred, tgt = pred.astype(np.float64), tgt.astype(np.float64)
    corners = lambda b: np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], 1)  # noqa: E731
    p, t = corners(pred), corners(tgt)
    iw = np.minimum(p[:, 2], t[:, 2]) - np.maximum(p[:, 0], t[:, 0])
    ih = np.minimum(p[:, 3], t[:, 3]) - np.maximum(p[:, 1], t[:, 1])
    coord = np.abs(pred - tgt).min() / KINK_MARGIN
    corner = min(np.abs(p - t).min(), np.abs(iw).min(), np.abs(ih).min()) / (1.5 * KINK_MARGIN)
    return float(min(coord, corner))


MICRO = dict(dim=192, depth=2, heads=3, mlp_dim=768)
BASE = dict(dim=768, depth=12, heads=12, mlp_dim=3072)
CASES = {
    "micro_det": (dict(decoder="detection", image_size=224, num_classes=20, **MICRO), 3),
    "base_det": (dict(decoder="detection", image_size=224, num_classes=20, **BASE), 2),
}
WEIGHT_DICT = {"loss_ce": 1.0, "class_error": 0.0, "loss_bbox": 5.0, "loss_giou": 2.0, "cardinality_error": 0.0}
EOS_COEF = 0.1
LOSSES = ["labels", "boxes", "cardinality"]


def run_case(name, kwargs, batch):
    from gen_golden import ViT, canonical                      # the reference's ViT (asserted there), qtorch stand-in installed
    from myrtle_vision.models.detector import SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    from oracle.detinit import det_images, det_param, summarize
    assert "/root/reference/" in sys.modules["myrtle_vision.models.detector"].__file__

    torch.manual_seed(0)
    torch.set_num_threads(8)
    vit = ViT(patch_size=16, q_format="FP32", **kwargs)
    shapes = {k: tuple(v.shape) for k, v in vit.state_dict().items()}
    vit.load_state_dict({k: det_param(k, s) for k, s in shapes.items()})
    vit.train()
    img = det_images(name, batch, kwargs["image_size"])
    matcher = HungarianMatcher()
    criterion = SetCriterion(kwargs["num_classes"], matcher=matcher, weight_dict=WEIGHT_DICT, eos_coef=EOS_COEF, losses=LOSSES)

    outputs = vit(img)
    Q = outputs["pred_logits"].shape[1]
    pred_boxes = outputs["pred_boxes"].detach()
    prob = outputs["pred_logits"].detach().softmax(-1)
    best = None                                                          # (total targets, seed, min_margin, min_kink)
    for seed in range(SEEDS):
        targets = det_targets(name, seed, batch, kwargs["num_classes"])
        total_targets = sum(len(t["labels"]) for t in targets)
        if best is not None and total_targets <= best[0]:
            continue
        costs = [(torch.cdist(pred_boxes[b], t["boxes"], p=1) - prob[b][:, t["labels"]]
                  - generalized_box_iou(box_convert(pred_boxes[b], "cxcywh", "xyxy"),
                                        box_convert(t["boxes"], "cxcywh", "xyxy"))).double().numpy()
                 for b, t in enumerate(targets)]
        min_kink = float("inf")
        for b, (t, cost) in enumerate(zip(targets, costs)):              # cheap test first: one solve per image
            if cost.shape[1] and min_kink >= 1.0:
                i, j = linear_sum_assignment(cost)
                min_kink = min(min_kink, kink_gap(pred_boxes[b].numpy()[i], t["boxes"].numpy()[j]))
        if min_kink < 1.0:
            continue
        ok, min_margin = True, float("inf")
        for b, cost in enumerate(costs):
            stable, margin = assignment_margin(cost, seed=b)
            ok, min_margin = ok and stable, min(min_margin, margin)
        if ok:
            best = (total_targets, seed, min_margin, min_kink)
    assert best is not None, "no stable, kink-free target set found"
    _, seed, min_margin, min_kink = best
    targets = det_targets(name, seed, batch, kwargs["num_classes"])

    indices = matcher(outputs, targets)
    losses = criterion(outputs, targets)
    total = sum(losses[k] * WEIGHT_DICT[k] for k in losses if k in WEIGHT_DICT)
    total.backward()

    out = {"pred_logits": outputs["pred_logits"].detach().numpy(), "pred_boxes": outputs["pred_boxes"].detach().numpy(),
           "total": total.detach().numpy()}
    for k, v in losses.items():
        out[k] = v.detach().numpy()
    for b, (i, j) in enumerate(indices):
        out[f"index_i:{b}"], out[f"index_j:{b}"] = i.numpy(), j.numpy()
    for b, t in enumerate(targets):
        out[f"tgt_labels:{b}"], out[f"tgt_boxes:{b}"] = t["labels"].numpy(), t["boxes"].numpy()
    unused = []
    for pname, p in vit.named_parameters():
        c = canonical(pname)
        if p.grad is None:
            unused.append(c)
            continue
        out[f"gsum:{c}"] = summarize(p.grad).numpy()
        if c.startswith("decoder."):
            out[f"grad:{c}"] = p.grad.detach().numpy()
    meta = {"kwargs": kwargs, "batch": batch, "q_format": None, "convert": False,
            "param_shapes": {k: list(s) for k, s in shapes.items()}, "state_keys": list(shapes.keys()),
            "unused_params": unused, "torch": torch.__version__, "num_queries": Q,
            "weight_dict": WEIGHT_DICT, "eos_coef": EOS_COEF, "losses": LOSSES,
            "targets": {"formula": "det_targets(name, seed, batch, num_classes) in tests/golden/gen_golden_detection.py",
                        "seed": seed, "seeds_tried": SEEDS, "sizes": [int(len(t["labels"])) for t in targets]},
            "tie_check": {"draws": 32, "eps": 1e-4, "stable": True,
                          "min_margin": None if min_margin == float("inf") else min_margin},
            "kink_check": {"margin": KINK_MARGIN, "corner_factor": 1.5, "min_gap_in_margins": min_kink}}
    return out, meta


def main():
    install_torchvision_standin()
    only = set(sys.argv[1:])
    here = os.path.dirname(os.path.abspath(__file__))
    for name, (kwargs, batch) in CASES.items():
        if only and name not in only:
            continue
        out, meta = run_case(name, kwargs, batch)
        np.savez_compressed(os.path.join(here, f"{name}.npz"), **out)
        with open(os.path.join(here, f"{name}.json"), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
        sz = os.path.getsize(os.path.join(here, f"{name}.npz"))
        print(f"{name}: {len(out)} arrays, {sz / 1024:.0f} KiB, targets {meta['targets']}, tie check {meta['tie_check']}, "
              f"kink check {meta['kink_check']}")


if __name__ == "__main__":
    main()
