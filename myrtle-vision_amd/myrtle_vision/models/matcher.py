"""Hungarian matching between YOLOS predictions and targets -- MI355X-native counterpart of the reference
``src/myrtle_vision/models/matcher.py`` (same constructor, assert and return format).

The reference builds one ``[B * Q, sum T]`` cost matrix out of a softmax, a gather, a cdist and a pairwise GIoU, copies it to the
host and reads only its per-image diagonal blocks.  Here ONE kernel (``mv_det_cost``) writes exactly those blocks into a packed
buffer, one device-to-host copy follows, and ``scipy.optimize.linear_sum_assignment`` runs per image on the host as in the
reference (matcher.py:84-86).
"""
import torch
from scipy.optimize import linear_sum_assignment
from torch import nn

from myrtle_vision.hip import ops


class PackedTargets:
    """The reference's list of ``{"labels": [T_b], "boxes": [T_b, 4]}`` dicts as flat device arrays, packed once per call and
    shared by the matcher and the criterion: ``labels`` int64 [sum T], ``boxes`` fp32 [sum T, 4], ``sizes`` (host list),
    ``offsets`` (host prefix sums), ``toff`` int32 [B + 1] and ``tcount`` int32 [B] on the device."""

    def __init__(self, targets, device):
        self.sizes = [int(len(t["labels"])) for t in targets]
        self.offsets = [0]
        for n in self.sizes:
            self.offsets.append(self.offsets[-1] + n)
        self.total = self.offsets[-1]
        if self.total:
            labels = torch.cat([t["labels"].reshape(-1) for t in targets]).to(device=device, dtype=torch.int64)
            boxes = torch.cat([t["boxes"].reshape(-1, 4) for t in targets]).to(device=device, dtype=torch.float32)
        else:
            labels = torch.zeros(0, dtype=torch.int64, device=device)
            boxes = torch.zeros(0, 4, dtype=torch.float32, device=device)
        self.labels, self.boxes = labels.contiguous(), boxes.contiguous()
        self.toff = torch.tensor(self.offsets, dtype=torch.int32).to(device)
        self.tcount = self.toff[1:] - self.toff[:-1]


class HungarianMatcher(nn.Module):
    """1-to-1 assignment of predictions to targets; unmatched predictions are "no object" (reference matcher.py:15-21).

    ``cost_class`` / ``cost_bbox`` / ``cost_giou``: weights of -softmax(logits)[label], the L1 distance between boxes and
    -GIoU in the matching cost."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1):
        super().__init__()
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"

    @torch.no_grad()
    def cost_blocks(self, outputs, packed):
        """The per-image cost blocks as host tensors: a list of fp32 [Q, T_b]."""
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        ops.require_cuda(logits, boxes)
        Q = logits.shape[1]
        flat = ops.det_cost(logits.detach().float().contiguous(), boxes.detach().float().contiguous(), packed.labels,
                            packed.boxes, packed.toff, packed.total, self.cost_class, self.cost_bbox, self.cost_giou).cpu()
        return [flat[Q * o:Q * (o + n)].view(Q, n) for o, n in zip(packed.offsets, packed.sizes)]

    @torch.no_grad()
    def forward(self, outputs, targets, packed=None):
        """-> a list of (index_i, index_j) int64 CPU tensors per image: the selected predictions and their targets, with
        len(index_i) = len(index_j) = min(num_queries, num_target_boxes).  ``packed``: the targets already packed
        (``PackedTargets``), when the caller shares them."""
        if packed is None:
            packed = PackedTargets(targets, outputs["pred_logits"].device)
        indices = [linear_sum_assignment(c) if c.shape[1] else ([], []) for c in self.cost_blocks(outputs, packed)]
        return [(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in indices]
