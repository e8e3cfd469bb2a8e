"""Hungarian matching between YOLOS predictions and targets -- MI355X-native counterpart of the reference
``src/myrtle_vision/models/matcher.py`` (same constructor, assert and return format).

The reference builds one ``[B * Q, sum T]`` cost matrix out of a softmax, a gather, a cdist and a pairwise GIoU, copies it to the
host and reads only its per-image diagonal blocks.  Here ONE kernel (``mv_det_cost``) writes exactly those blocks into a packed
buffer.  With ``assignment="host"`` (the default) one device-to-host copy follows and
``scipy.optimize.linear_sum_assignment`` runs per image on the host as in the reference (matcher.py:84-86); with
``assignment="device"`` a second kernel (``mv_det_match``) solves every image's assignment where the blocks are, and the
criterion goes from the model's output to the loss scalar without waiting for the host.
"""
import warnings

import numpy as np
import torch
from torch import nn

from myrtle_vision.hip import ops

# scipy.optimize.linear_sum_assignment's two ValueError messages, raised for the same inputs in device mode
_STATUS_MESSAGES = {1: "matrix contains invalid numeric entries", 2: "cost matrix is infeasible"}
_warned_host_fallback = False


def raise_for_status(status):
    """``status``: the per-image codes of ``mv_det_match`` on the host (any sequence of ints).  Raises scipy's ValueError for
    the first image that was not solved."""
    for s in np.asarray(status).reshape(-1).tolist():
        if s != 0:
            raise ValueError(_STATUS_MESSAGES.get(s, f"assignment status {s}"))


def indices_from_match(match, status, Q, offsets):
    """The reference's return format from the device solver's result, on the host: ``match`` int [B * Q] (flat target index
    ``offsets[b] + t`` of every query, or -1), ``status`` int [B], ``offsets`` the B + 1 prefix sums of the target counts ->
    a list of (index_i, index_j) int64 tensors per image, queries ascending (the order scipy returns for a [Q, T] matrix)."""
    raise_for_status(status)
    match = np.asarray(match).reshape(len(offsets) - 1, Q)
    out = []
    for b, row in enumerate(match):
        src = np.nonzero(row >= 0)[0]
        out.append((torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(row[src] - offsets[b], dtype=torch.int64)))
    return out


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
    -GIoU in the matching cost.  ``assignment``: ``"host"`` = scipy on the host after one copy of the cost blocks;
    ``"device"`` = ``mv_det_match`` (up to 1024 queries and 1024 targets per image; a larger batch takes the host path for
    that call, with one warning per process)."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, assignment: str = "host"):
        super().__init__()
        if assignment not in ("host", "device"):
            raise ValueError(f"unknown assignment {assignment!r} (expected 'host' or 'device')")
        self.assignment = assignment
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"

    def _cost_flat(self, outputs, packed):
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        ops.require_cuda(logits, boxes)
        return ops.det_cost(logits.detach().float().contiguous(), boxes.detach().float().contiguous(), packed.labels,
                            packed.boxes, packed.toff, packed.total, self.cost_class, self.cost_bbox, self.cost_giou)

    @torch.no_grad()
    def cost_blocks(self, outputs, packed):
        """The per-image cost blocks as host tensors: a list of fp32 [Q, T_b]."""
        Q = outputs["pred_logits"].shape[1]
        flat = self._cost_flat(outputs, packed).cpu()
        return [flat[Q * o:Q * (o + n)].view(Q, n) for o, n in zip(packed.offsets, packed.sizes)]

    def on_device(self, outputs, packed) -> bool:
        """Whether this call is solved by the kernel: device mode and a batch inside its limit."""
        if self.assignment != "device":
            return False
        if max([outputs["pred_logits"].shape[1]] + packed.sizes) <= ops.DET_MATCH_MAX:
            return True
        global _warned_host_fallback
        if not _warned_host_fallback:
            _warned_host_fallback = True
            warnings.warn(f"HungarianMatcher(assignment='device'): more than {ops.DET_MATCH_MAX} queries or targets per image; "
                          "such batches are assigned on the host")
        return False

    @torch.no_grad()
    def match_device(self, outputs, packed):
        """-> (match int32 [B * Q]: the flat target index of every query or -1, status int32 [B]: 0 solved, 1 NaN / -inf in
        the cost block (or a target count outside [0, max(sizes)], which packed targets never have), 2 infeasible), both on the
        device; nothing is copied to the host."""
        B, Q = outputs["pred_logits"].shape[:2]
        return ops.det_match(self._cost_flat(outputs, packed), packed.toff, B, Q, max(packed.sizes, default=0))

    @torch.no_grad()
    def forward(self, outputs, targets, packed=None):
        """-> a list of (index_i, index_j) int64 CPU tensors per image: the selected predictions and their targets, with
        len(index_i) = len(index_j) = min(num_queries, num_target_boxes).  ``packed``: the targets already packed
        (``PackedTargets``), when the caller shares them."""
        if packed is None:
            packed = PackedTargets(targets, outputs["pred_logits"].device)
        if self.on_device(outputs, packed):
            match, status = self.match_device(outputs, packed)
            both = torch.cat((match, status)).cpu().numpy()                 # one copy: B * (Q + 1) int32
            return indices_from_match(both[:match.numel()], both[match.numel():], outputs["pred_logits"].shape[1], packed.offsets)
        from scipy.optimize import linear_sum_assignment
        indices = [linear_sum_assignment(c) if c.shape[1] else ([], []) for c in self.cost_blocks(outputs, packed)]
        return [(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in indices]
