"""Set loss and post-processing of the YOLOS detector -- MI355X-native counterpart of the reference
``src/myrtle_vision/models/detector.py`` (same constructor signatures, ``empty_weight`` buffer and returned keys).

The reference's criterion is a few dozen small torch launches per step; here the matching decides a per-query target class and
box (``mv_det_assign``) and ONE forward kernel computes the three losses and the two logged statistics, ONE backward kernel both
gradients (``F.det_set_loss``).  There is no CPU path.
"""
import numpy as np
import torch
from torch import nn

from myrtle_vision.hip import functional as F
from myrtle_vision.hip import ops
from myrtle_vision.models.matcher import HungarianMatcher, PackedTargets
from myrtle_vision.utils.utils import get_world_size, is_dist_avail_and_initialized

_LOSS_KEYS = {"labels": ("loss_ce", "class_error"), "cardinality": ("cardinality_error",), "boxes": ("loss_bbox", "loss_giou")}


class SetCriterion(nn.Module):
    """Hungarian assignment between targets and predictions, then class and box supervision of every matched pair
    (reference detector.py:16-21).

    ``num_classes``: object categories without the "no object" one; ``matcher``: module computing the assignment;
    ``weight_dict``: loss name -> weight (applied by the caller, as in the reference's training loop); ``eos_coef``: the
    classification weight of "no object"; ``losses``: any of "labels", "cardinality", "boxes"."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        self.match_status = None
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)

    def num_boxes(self, targets, device) -> float:
        """Target boxes per node for normalisation (reference detector.py:134-138): summed over the batch, all-reduced when
        torch.distributed is initialised, divided by the world size, at least 1."""
        n = float(sum(len(t["labels"]) for t in targets))
        if is_dist_avail_and_initialized():
            t = torch.as_tensor([n], dtype=torch.float, device=device)
            torch.distributed.all_reduce(t)
            n = float(t.item())
        return max(n / get_world_size(), 1.0)

    def forward(self, outputs, targets, packed=None):
        """``outputs``: {"pred_logits": [B, Q, C + 1], "pred_boxes": [B, Q, 4]}; ``targets``: a list of B dicts with
        "labels" [T_b] and "boxes" [T_b, 4] (cx, cy, w, h, normalised); ``packed``: the same targets already packed
        (``PackedTargets``).  -> {loss name: scalar} for the requested losses.

        With a ``HungarianMatcher(assignment="device")`` the assignment stays on the device and nothing here waits for it:
        ``self.match_status`` then holds the solver's per-image status (int32 [B], on the device, unread; ``None`` otherwise)
        for the caller to check where it next synchronises (``matcher.raise_for_status``)."""
        for loss in self.losses:
            assert loss in _LOSS_KEYS, f"do you really want to compute {loss} loss?"
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        ops.require_cuda(logits, boxes)
        assert len(targets) == logits.shape[0]
        B, Q, C1 = logits.shape
        dev = logits.device
        if packed is None:
            packed = PackedTargets(targets, dev)
        plain = {k: v for k, v in outputs.items() if k != "aux_outputs"}
        self.match_status = None
        if isinstance(self.matcher, HungarianMatcher) and self.matcher.on_device(plain, packed):
            match, self.match_status = self.matcher.match_device(plain, packed)
        else:
            if isinstance(self.matcher, HungarianMatcher):
                indices = self.matcher(plain, targets, packed=packed)
            else:
                indices = self.matcher(plain, targets)
            # query -> flat target index (or -1), built on the host from the matching and copied once
            match = np.full(B * Q, -1, dtype=np.int32)
            for b, (src, tgt) in enumerate(indices):
                if len(src):
                    match[b * Q + np.asarray(src, dtype=np.int64)] = packed.offsets[b] + np.asarray(tgt, dtype=np.int64)
            match = torch.from_numpy(match).to(dev)
        tgt_class, tgt_box = ops.det_assign(match, packed.labels, packed.boxes, B, Q, self.num_classes)

        weight = self.empty_weight
        if weight.dtype != torch.float32 or not weight.is_cuda:
            weight = weight.to(device=dev, dtype=torch.float32)
        out = F.det_set_loss(logits, boxes, tgt_class, tgt_box, weight, packed.tcount, self.num_boxes(targets, dev))
        values = dict(zip(("loss_ce", "loss_bbox", "loss_giou", "class_error", "cardinality_error"), out))
        return {k: values[k] for loss in self.losses for k in _LOSS_KEYS[loss]}


class PostProcess(nn.Module):
    """Model output -> the per-image {"scores", "labels", "boxes"} dicts the COCO API expects (reference detector.py:148-176)."""

    @torch.no_grad()
    def forward(self, outputs, target_sizes):
        """``target_sizes``: [B, 2] = (height, width) of every image (the original size for evaluation)."""
        out_logits, out_bbox = outputs["pred_logits"], outputs["pred_boxes"]
        assert len(out_logits) == len(target_sizes)
        assert target_sizes.shape[1] == 2
        ops.require_cuda(out_logits, out_bbox)
        sizes = target_sizes.to(device=out_logits.device, dtype=torch.float32).contiguous()
        scores, labels, boxes = ops.det_postprocess(out_logits.detach().float().contiguous(),
                                                    out_bbox.detach().float().contiguous(), sizes)
        return [{"scores": s, "labels": l, "boxes": b} for s, l, b in zip(scores, labels, boxes)]
